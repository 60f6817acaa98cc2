"""Read names ranked on the GPU (cutesv_amd/csrc/names.hip.h, csv_name_pool_* / csv_name_ranks):
the ranks of an adversarial name list against Python's sorted(set()) and against `rebuild.name_ranks_host`, the pool's
append / cache / misuse behaviour, and the BAM -> pool -> rebuild chain ordered by name (CSV_RB_RANK_FROM_NAMES) against
`rebuild_pool` fed with host-made ranks of the same names.

The name list is built once (fixed seed): 4097 names = one sort tile of 4096 rows plus one row, two rank tiles of 2048 plus
one; lengths around every word boundary; pairs that differ in one byte only; bytes above 0x7f (a signed compare would order
them first)."""
import ctypes as C
import os

import numpy as np
import pytest

from cutesv_amd import bam, extract, rebuild, synth, _abi, _lib
from cutesv_amd.columns import TYPES
from helpers import load_json
import bam_writer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LEN = {"1": 248956422, "10": 133797422, "2": 242193529, "7": 159345973, "X": 156040895}
N_NAMES = 4097


@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ the adversarial list
def _shapes(rng):
    text = lambda n: bytes(rng.integers(0x21, 0x7F, n, dtype=np.uint8).tolist())                  # noqa: E731
    out = [text(n) for n in (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 254, 255)]
    for at, n in ((7, 20), (8, 20), (253, 254)):              # pairs that differ in one byte only: inside word 0, the first of word 1, the last of 254
        base = bytearray(text(n))
        base[at] = ord("A")
        other = bytearray(base)
        other[at] = ord("B")
        out += [bytes(base), bytes(other)]
    out += [b"read_ext", b"read_extA", b"read_ex"]            # a name, its extension by one byte, its prefix
    for x in (0x01, 0x7F, 0x80, 0xFF):
        out += [bytes([x]), b"sgn" + bytes([x]) + b"tail", b"sgn_pad" + bytes([x]), b"sgn_pad_" + bytes([x])]
    return out


def _generated(rng, k):
    if k & 1:
        h = "%032x" % int.from_bytes(rng.bytes(16), "big")
        return ("%s-%s-%s-%s-%s" % (h[:8], h[8:12], h[12:16], h[16:20], h[20:])).encode()          # an ONT UUID
    return b"m64011_190830_220126/%d/ccs" % int(rng.integers(1, 180_000_000))                       # a HiFi name


def adversarial_names():
    rng = np.random.default_rng(20261017)
    shapes, names, k = _shapes(rng), [], 0
    seen = set()
    while len(names) < N_NAMES:
        if k < len(shapes):
            s = shapes[k]
        else:
            s = _generated(rng, k)
        k += 1
        if s in seen:
            continue
        seen.add(s)
        rem = N_NAMES - len(names)
        rep = rem if rem <= 5 else int(rng.integers(2, 6))
        if rem - rep == 1:
            rep += 1 if rep < 5 else -1
        names += [s] * rep
    assert k > len(shapes) + 500 and len(names) == N_NAMES
    order = rng.permutation(N_NAMES)
    return [names[i] for i in order.tolist()]


NAMES = adversarial_names()


def strided(names, gap=3):
    """the names as (bytes, off, len) with `gap` foreign bytes between them, as a chunk's host image has the bases"""
    blob, off = bytearray(), []
    for s in names:
        blob += b"\xee" * gap
        off.append(len(blob))
        blob += s
    blob += b"\xee" * gap
    return np.frombuffer(bytes(blob), np.uint8), np.asarray(off, np.int64), np.asarray([len(s) for s in names], np.int32)


def python_ranks(names):
    uniq = sorted(set(names))
    at = {s: r for r, s in enumerate(uniq)}
    first = {}
    for i, s in enumerate(names):
        first.setdefault(s, i)
    return np.asarray([at[s] for s in names], np.int32), np.asarray([first[s] for s in uniq], np.int32), uniq


WANT_RANK, WANT_FIRST, UNIQ = python_ranks(NAMES)


def assert_ranks(got, names=NAMES, want=None):
    rank, first, uniq = want or (WANT_RANK, WANT_FIRST, UNIQ)
    assert got["n"] == len(names) and got["n_distinct"] == len(uniq) and got["max_len"] == max(len(s) for s in names)
    assert got["rank"].dtype == np.int32 and np.array_equal(got["rank"], rank)
    assert got["first"].dtype == np.int32 and np.array_equal(got["first"], first)


# ------------------------------------------------------------------------------------------------ CPU
def test_the_list_holds_what_it_must():
    lens = {len(s) for s in NAMES}
    assert {0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 254, 255} <= lens and len(NAMES) == N_NAMES
    counts = {}
    for s in NAMES:
        counts[s] = counts.get(s, 0) + 1
    assert set(counts.values()) <= {2, 3, 4, 5} and len(counts) > 1000
    assert any(s[:1] == b"\xff" for s in NAMES) and any(s[:1] == b"\x01" for s in NAMES)
    assert UNIQ[0] == b"" and UNIQ.index(b"read_ex") + 1 == UNIQ.index(b"read_ext") == UNIQ.index(b"read_extA") - 1


def test_header_declares_the_name_entries_and_the_abi_is_still_9():
    text = open(os.path.join(ROOT, "include", "cutesv_hip.h")).read()
    for sym in ("csv_name_pool_reset", "csv_name_pool_rows", "csv_name_pool_append", "csv_name_ranks", "csv_name_pool_get", "csv_name_struct_size",
                "csv_name_rank_out", "CSV_RB_RANK_FROM_NAMES = 4"):
        assert sym in text, sym
    assert "#define CSV_ABI_VERSION 9" in text
    L = _lib.lib()
    assert _abi.ABI_VERSION == 9 and L.csv_abi_version() == 9 and _abi.RB_RANK_FROM_NAMES == 4
    bound = {n for n, _, _ in _lib.SYMBOLS}
    assert {"csv_name_pool_reset", "csv_name_pool_rows", "csv_name_pool_append", "csv_name_ranks", "csv_name_pool_get", "csv_name_struct_size"} <= bound


def test_name_struct_size_equals_the_mirror():
    L = _lib.lib()
    assert L.csv_name_struct_size(0) == C.sizeof(_abi.NameRankOut) == _abi.NAME_STRUCT_SIZES[0][1]
    assert L.csv_name_struct_size(1) == 0 and L.csv_name_struct_size(-1) == 0
    assert rebuild.NameRankOut is _abi.NameRankOut


def test_name_ranks_host_equals_sorted_set():
    data, off, ln = strided(NAMES)
    rank, first = rebuild.name_ranks_host(data, off, ln)
    assert rank.dtype == np.int32 and first.dtype == np.int32
    assert np.array_equal(rank, WANT_RANK) and np.array_equal(first, WANT_FIRST)
    # edges: nothing, one name, only empty names
    r0, f0 = rebuild.name_ranks_host(b"", [], [])
    assert len(r0) == 0 and len(f0) == 0
    r1, f1 = rebuild.name_ranks_host(b"abc", [0], [3])
    assert r1.tolist() == [0] and f1.tolist() == [0]
    r2, f2 = rebuild.name_ranks_host(b"", [0, 0, 0], [0, 0, 0])
    assert r2.tolist() == [0, 0, 0] and f2.tolist() == [0]
    with pytest.raises(ValueError):
        rebuild.name_ranks_host(b"abc", [1], [3])


def golden_records(case, chrom):
    refs = [(c, REF_LEN[c]) for c in case["chroms"]]
    refid = case["chroms"].index(chrom)
    recs = [dict(d, seq=synth.pseudo_sequence(d["seq_len"], d["seq_key"]), refid=refid, tags=[tuple(t) for t in d["tags"]]) for d in case["reads"]]
    return refs, recs


def test_name_columns_reproduce_chunk_name(tmp_path):
    case = load_json("single_pipe.json.gz")[0]
    chrom = case["task"][0]
    refs, recs = golden_records(case, chrom)
    # names of length 1 and 254 among them (l_read_name counts the NUL: 255 is the format's limit)
    recs = [dict(r, name=("x" if i == 3 else "y" * 254 if i == 5 else r["name"])) for i, r in enumerate(recs)]
    path = str(tmp_path / "n.bam")
    bam_writer.write_bam(path, refs, recs)
    with bam.BamFile(path) as bf:
        chunks = list(bf.chunks(chrom, chunk_records=97))
    assert len(chunks) > 2
    seen = []
    for ch in chunks:
        off, ln = ch.name_columns()
        assert off.dtype == np.int64 and ln.dtype == np.int32 and len(off) == len(ln) == ch.n
        got = [ch.host[o:o + k].tobytes().decode() for o, k in zip(off.tolist(), ln.tolist())]
        assert got == [ch.name(i) for i in range(ch.n)]
        seen += got
    assert seen == [r["name"] for r in recs] and {1, 254} <= {len(s) for s in seen}
    # the host function over a chunk's own image
    ch = chunks[0]
    off, ln = ch.name_columns()
    rank, first = rebuild.name_ranks_host(ch.host, off, ln)
    want = python_ranks([ch.name(i).encode() for i in range(ch.n)])
    assert np.array_equal(rank, want[0]) and np.array_equal(first, want[1])


# ------------------------------------------------------------------------------------------------ GPU
def fill(ctx, names, cuts=()):
    rebuild.name_pool_reset(ctx)
    data, off, ln = strided(names)
    bounds = [0] + list(cuts) + [len(names)]
    firsts = [rebuild.name_pool_append(ctx, data, off[a:b], ln[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
    assert firsts == bounds[:-1] and rebuild.name_pool_rows(ctx) == len(names)


@pytest.mark.gpu
def test_gpu_ranks_of_the_list_in_one_append(ctx):
    fill(ctx, NAMES)
    got = rebuild.name_ranks(ctx)
    assert_ranks(got)
    data, off, ln = strided(NAMES)
    host_rank, host_first = rebuild.name_ranks_host(data, off, ln)
    assert np.array_equal(got["rank"], host_rank) and np.array_equal(got["first"], host_first)
    assert 0 < got["n_passes"] <= 255 and got["ms_device"] > 0
    # the cached ranks: nothing runs, the same answer
    again = rebuild.name_ranks(ctx)
    assert_ranks(again)
    assert again["n_passes"] == got["n_passes"] and again["ms_device"] == got["ms_device"]
    dev_only = rebuild.name_ranks(ctx, host=False)
    assert dev_only["rank"] is None and dev_only["n_distinct"] == len(UNIQ)
    # ids back to text
    assert rebuild.name_pool_get(ctx, got["first"], raw=True) == UNIQ
    assert rebuild.name_pool_get(ctx, [5, 5, 0], raw=True) == [NAMES[5], NAMES[5], NAMES[0]] and rebuild.name_pool_get(ctx, []) == []
    rebuild.name_pool_reset(ctx)


@pytest.mark.gpu
def test_gpu_ranks_after_several_appends_and_a_stale_cache(ctx):
    fill(ctx, NAMES, cuts=(1, 2048))                          # 1 + 2047 + 2049 names
    assert_ranks(rebuild.name_ranks(ctx))
    more = [b"zz_late_%d" % k for k in range(8)] + [NAMES[0], b""]
    data, off, ln = strided(more)
    assert rebuild.name_pool_append(ctx, data, off, ln) == N_NAMES
    every = NAMES + more
    got = rebuild.name_ranks(ctx)
    assert got["n"] == N_NAMES + 10
    assert_ranks(got, every, python_ranks(every))
    rebuild.name_pool_reset(ctx)


@pytest.mark.gpu
def test_gpu_edge_pools(ctx):
    rebuild.name_pool_reset(ctx)
    got = rebuild.name_ranks(ctx)
    assert got["n"] == 0 and got["n_distinct"] == 0 and len(got["rank"]) == 0 and len(got["first"]) == 0 and got["n_passes"] == 0
    fill(ctx, [b"only"])
    got = rebuild.name_ranks(ctx)
    assert got["rank"].tolist() == [0] and got["first"].tolist() == [0] and got["n_distinct"] == 1 and got["n_passes"] == 0 and got["max_len"] == 4
    fill(ctx, [b"m64011_190830_220126/1234/ccs"] * 3000)
    got = rebuild.name_ranks(ctx)
    assert got["n_passes"] == 0 and not got["rank"].any() and got["first"].tolist() == [0] and got["n_distinct"] == 1
    # 254 bytes, equal up to the last one: one pass, not 254
    rng = np.random.default_rng(7)
    last = rng.integers(0x21, 0x7F, 3000)
    names = [b"q" * 253 + bytes([x]) for x in last.tolist()]
    fill(ctx, names)
    got = rebuild.name_ranks(ctx)
    assert got["n_passes"] == 1 and got["max_len"] == 254
    assert_ranks(got, names, python_ranks(names))
    # only empty names
    fill(ctx, [b""] * 70)
    got = rebuild.name_ranks(ctx)
    assert got["n_passes"] == 0 and got["max_len"] == 0 and not got["rank"].any() and got["n_distinct"] == 1
    rebuild.name_pool_reset(ctx)


@pytest.mark.gpu
def test_gpu_misuse_leaves_the_pool_and_the_context_usable(ctx):
    from cutesv_amd.engine import CsvError
    fill(ctx, NAMES)
    L = _lib.lib()
    data = np.frombuffer(b"0123456789" * 30, np.uint8)
    first = C.c_int64(-1)
    for off, ln in (([0, 295], [5, 6]), ([0, 2], [3, 256]), ([0, -1], [3, 1]), ([0, 301], [3, 0]), ([0, 1], [3, -1])):
        o, k = np.asarray(off, np.int64), np.asarray(ln, np.int32)
        assert L.csv_name_pool_append(ctx._h, 2, data.ctypes.data, len(data), o.ctypes.data, k.ctypes.data, C.byref(first)) == _abi.E_INVALID, (off, ln)
        assert rebuild.name_pool_rows(ctx) == N_NAMES
    with pytest.raises(CsvError) as e:
        rebuild.name_pool_append(ctx, data, [0], [256])
    assert e.value.code == _abi.E_INVALID and rebuild.name_pool_rows(ctx) == N_NAMES
    with pytest.raises(CsvError) as e:
        rebuild.name_pool_get(ctx, [0, N_NAMES])
    assert e.value.code == _abi.E_INVALID
    # a pool row whose read has no name
    zeros = np.zeros(2, np.uint8)
    rebuild.pool_reset(ctx)
    rebuild.pool_append(ctx, [0, 1, 1], [10, 20, 30], [5, 5, 5], [3, N_NAMES - 1, N_NAMES], [0, 0, 0])
    with pytest.raises(CsvError) as e:
        rebuild.rebuild_pool_by_name(ctx, zeros, keep_on_device=False)
    assert e.value.code == _abi.E_INVALID
    # ... the same rows without it go through, by name
    rebuild.pool_reset(ctx)
    rebuild.pool_append(ctx, [0, 1, 1], [10, 20, 20], [5, 5, 5], [3, N_NAMES - 1, 7], [0, 0, 0])
    r = rebuild.rebuild_pool_by_name(ctx, zeros, keep_on_device=False)
    by_name = sorted([int(WANT_RANK[N_NAMES - 1]), int(WANT_RANK[7])])
    assert r["read_id"].tolist() == [int(WANT_RANK[3])] + by_name and r["a"].tolist() == [10, 20, 20]
    rebuild.pool_reset(ctx)
    # an empty name pool has no rank for any row
    rebuild.name_pool_reset(ctx)
    rebuild.pool_append(ctx, [0], [10], [5], [0], [0])
    with pytest.raises(CsvError) as e:
        rebuild.rebuild_pool_by_name(ctx, zeros, keep_on_device=False)
    assert e.value.code == _abi.E_INVALID
    rebuild.pool_reset(ctx)
    fill(ctx, NAMES)
    assert_ranks(rebuild.name_ranks(ctx))
    rebuild.name_pool_reset(ctx)


# ---- end to end: BAM -> pool + name pool -> rebuilt columns
def pipe_args(p):
    return (p["sv"], p["min_mapq"], p["parts"], p["min_read_len"], p["min_siglength"], p["md"], p["mi"], p["max_size"])


def segments_of(case):
    n_chrom = len(case["chroms"])
    seg_of = lambda t, ci: TYPES.index(t) * n_chrom + ci                        # noqa: E731
    major = np.zeros(len(TYPES) * n_chrom, np.uint8); nodedup = np.zeros(len(TYPES) * n_chrom, np.uint8)
    for t in ("INV", "TRA"):
        major[seg_of(t, 0):seg_of(t, 0) + n_chrom] = 1
    nodedup[seg_of("INS", 0):seg_of("INS", 0) + n_chrom] = 1
    return seg_of, [seg_of(t, 0) for t in ("DEL", "INS", "DUP", "INV", "TRA")], major, nodedup


def fill_from_bam(ctx, case, path, passes):
    """`passes` x task_to_pool(name_pool=True, read_base=None) of the case's task into one pool and one name pool"""
    p, (chrom, t0, t1) = case["params"], case["task"]
    rank = {c: i for i, c in enumerate(case["chroms"])}
    seg_of, seg_base, _, _ = segments_of(case)
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)
    out = []
    with bam.BamFile(path) as bf:
        for _ in range(passes):
            out.append(extract.task_to_pool(ctx, bf, chrom, t0, t1, rank, *pipe_args(p), seg_of("INS", rank[chrom]), seg_of("DEL", rank[chrom]), seg_base, None,
                                            bed_regions=case["bed"], name_pool=True))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(load_json("single_pipe.json.gz"))))
def test_gpu_bam_to_rebuilt_columns_by_name(ctx, tmp_path, which):
    case = load_json("single_pipe.json.gz")[which]
    p, (chrom, t0, t1) = case["params"], case["task"]
    crank = {c: i for i, c in enumerate(case["chroms"])}
    _, _, major, nodedup = segments_of(case)
    refs, recs = golden_records(case, chrom)
    path = str(tmp_path / "e.bam")
    bam_writer.write_bam(path, refs, recs)
    # one pass, for the row counts after de-duplication
    (one,) = fill_from_bam(ctx, case, path, 1)
    single = rebuild.rebuild_pool_by_name(ctx, major, nodedup, keep_on_device=False)
    n_pool_one = rebuild.pool_rows(ctx)
    # two passes into one pool and one name pool: every name occurs under two indices
    res = fill_from_bam(ctx, case, path, 2)
    with bam.BamFile(path) as bf:
        ch = bf.records(chrom, t0, t1)
        _, reads_info = extract.single_pipe_bam(ctx, bf, chrom, t0, t1, crank, *pipe_args(p), bed_regions=case["bed"])
    n = ch.n
    assert [r["name_base"] for r in res] == [0, n] and rebuild.name_pool_rows(ctx) == 2 * n and rebuild.pool_rows(ctx) == 2 * n_pool_one
    assert all(r["n_flagged"] == 0 for r in res) and n_pool_one > 50
    names = [ch.name(i) for i in range(n)] * 2
    off, ln = ch.name_columns()
    host_rank, host_first = rebuild.name_ranks_host(np.concatenate([ch.host, ch.host]), np.concatenate([off, off + len(ch.host)]), np.concatenate([ln, ln]))
    got = rebuild.rebuild_pool_by_name(ctx, major, nodedup, keep_on_device=False)
    want = rebuild.rebuild_pool(ctx, host_rank, major, nodedup, keep_on_device=False)
    for k in ("seg_id", "a", "b", "read_id", "aux", "src_row", "seg_count"):
        assert np.array_equal(got[k], want[k]), k
    # equal names got equal ids: the second pass's rows are duplicates wherever duplicates are dropped
    dedup = nodedup == 0
    assert np.array_equal(got["seg_count"][dedup], single["seg_count"][dedup]) and single["seg_count"][dedup].sum() > 20
    assert np.array_equal(got["seg_count"][~dedup], 2 * single["seg_count"][~dedup])
    sel = dedup[got["seg_id"]]
    assert np.array_equal(got["read_id"][sel], single["read_id"][dedup[single["seg_id"]]])
    # ranks, ids back to text, and the reads table's ids in the same id space
    ranks = rebuild.name_ranks(ctx)
    uniq = sorted(set(names))
    assert np.array_equal(ranks["rank"], host_rank) and np.array_equal(ranks["first"], host_first) and ranks["n_distinct"] == len(uniq)
    assert rebuild.name_pool_get(ctx, ranks["first"]) == uniq
    for r in res:
        ids = ranks["rank"][r["name_base"] + r["reads_index"]]
        assert [uniq[i] for i in ids.tolist()] == [x[3] for x in reads_info] and len(ids) > 10
    # a read_base that is not the name pool's row count: refused before a row or a name is appended
    with bam.BamFile(path) as bf:
        with pytest.raises(ValueError):
            extract.task_to_pool(ctx, bf, chrom, t0, t1, crank, *pipe_args(p), 0, 1, [0] * 5, 5, name_pool=True)
        with pytest.raises(ValueError):
            extract.task_to_pool(ctx, bf, chrom, t0, t1, crank, *pipe_args(p), 0, 1, [0] * 5, None)
    assert rebuild.name_pool_rows(ctx) == 2 * n and rebuild.pool_rows(ctx) == 2 * n_pool_one
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)


def device_to_host(address, count, dtype):
    """`count` items of `dtype` at a device address, copied with the HIP runtime the library is linked with"""
    hip = None
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = C.CDLL(name)
            break
        except OSError:
            continue
    assert hip is not None, "the HIP runtime library was not found"
    out = np.empty(count, dtype)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data, address, out.nbytes, 2) == 0                 # hipMemcpyDeviceToHost
    return out


@pytest.mark.gpu
def test_gpu_rebuilt_device_columns_feed_the_clustering_stage(ctx, tmp_path):
    case = load_json("single_pipe.json.gz")[0]
    chrom = case["task"][0]
    n_chrom = len(case["chroms"])
    _, _, major, nodedup = segments_of(case)
    refs, recs = golden_records(case, chrom)
    path = str(tmp_path / "d.bam")
    bam_writer.write_bam(path, refs, recs)
    fill_from_bam(ctx, case, path, 2)
    host = rebuild.rebuild_pool_by_name(ctx, major, nodedup, keep_on_device=False)
    dev = rebuild.rebuild_pool_by_name(ctx, major, nodedup, keep_on_device=True)
    assert dev["n_out"] == len(host["a"]) > 50 and np.array_equal(dev["src_row"], host["src_row"]) and np.array_equal(dev["seg_count"], host["seg_count"])
    assert np.array_equal(device_to_host(dev["dev"]["read_id"], dev["n_out"], np.int32), host["read_id"])
    assert np.array_equal(device_to_host(dev["dev"]["a"], dev["n_out"], np.int64), host["a"])
    off = np.r_[0, np.cumsum(dev["seg_count"])]
    segs = [_abi.make_segment(TYPES[s // n_chrom], s % n_chrom, int(off[s]), int(off[s + 1]), 200 if TYPES[s // n_chrom] == "DEL" else 100, 2, diff_ratio=0.3,
                              sv_size=30, max_size=100000, min_support_reads=2) for s in range(len(major)) if dev["seg_count"][s]]
    segs = np.array(segs, dtype=_abi.SEGMENT_DTYPE)
    res_dev = ctx.cluster_batch(_abi.HostBatch.on_device(segs, dev["dev"], dev["n_out"], n_chrom=n_chrom, keep=ctx)).trimmed()
    res_host = ctx.cluster_batch(_abi.HostBatch(segs, host["a"], host["b"], host["read_id"], host["aux"], n_chrom=n_chrom)).trimmed()
    for k in ("call_seg", "bp1", "bp2", "support", "support_off", "support_sig"):
        assert np.array_equal(res_dev[k], res_host[k]), k
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)


# ---- one context through the whole chain, three times: every stage's buffers grow, are reused smaller, are reused at size
def host_rebuilt(case, path, t0, t1):
    """The region's rebuilt columns with nothing run on the device: single_pipe_bam's host path (decode_host + the oracle's
    CIGAR / split engines), its candidate tuples as pool rows (the mapping test_oracle_golden checks), read ids from
    name_ranks_host over the names of the region's records, then the rebuild's contract in numpy: lexsort by (segment,
    [aux where it is major], a, b, read id) and adjacent de-duplication outside the INS segments.  Rows that tie on the
    whole key are ordered by aux here (the device keeps them in pool order).  -> (columns, rank, first)"""
    from cutesv_amd.columns import BND_CODE
    from oracle import oracle
    p, chrom = case["params"], case["task"][0]
    crank = {c: i for i, c in enumerate(case["chroms"])}
    seg_of, _, major, nodedup = segments_of(case)
    with bam.BamFile(path) as bf:
        ch = bf.records(chrom, t0, t1)
        cand, _ = extract.single_pipe_bam((oracle.cigar_signatures, oracle.split_signatures), bf, chrom, t0, t1, crank, *pipe_args(p), bed_regions=case["bed"])
    off, ln = ch.name_columns()
    rank, first = rebuild.name_ranks_host(ch.host, off, ln)
    rank_of = {ch.name(i): int(rank[i]) for i in range(ch.n)}
    rows = []
    for t, lst in cand.items():
        for x in lst:
            seg = seg_of(t, crank[x[-1]])
            if t in ("DEL", "DUP"):
                a, b, aux = x[0], x[1], 0
            elif t == "INS":
                a, b, aux = int(x[0]), x[1], len(x[3])
            elif t == "INV":
                a, b, aux = x[1], x[2], {"++": 0, "--": 1}[x[0]]
            else:
                a, b, aux = x[1], x[3], crank[x[2]] * 8 + BND_CODE[x[0]]
            rows.append((seg, aux if major[seg] else 0, a, b, rank_of[x[2] if t == "INS" else x[-3]], aux))
    rows = np.array(sorted(rows), np.int64).reshape(-1, 6)
    same = np.r_[False, (rows[1:, :5] == rows[:-1, :5]).all(axis=1)]
    rows = rows[~(same & (nodedup[rows[:, 0]] == 0))]
    cols = dict(seg_id=rows[:, 0].astype(np.int32), a=rows[:, 2], b=rows[:, 3], read_id=rows[:, 4].astype(np.int32), aux=rows[:, 5].astype(np.int32),
                seg_count=np.bincount(rows[:, 0], minlength=len(major)).astype(np.int64))
    return cols, rank, first


@pytest.mark.gpu
def test_gpu_one_context_through_growing_shrinking_and_refilled_stages(ctx, tmp_path):
    from cutesv_amd.columns import Params
    from oracle import oracle
    case = load_json("single_pipe.json.gz")[0]
    p, chrom = case["params"], case["task"][0]
    crank = {c: i for i, c in enumerate(case["chroms"])}
    seg_of, seg_base, major, nodedup = segments_of(case)
    refs, recs = golden_records(case, chrom)
    path = str(tmp_path / "g.bam")
    bam_writer.write_bam(path, refs, recs)
    sizes = []
    for k, (t0, t1) in enumerate(((0, 3000000), (0, 220000), (0, 3000000))):
        if k == 2:
            # the rebuild counted into the engine's counter block and cleared `uploaded`: the engine comes back clean
            st = synth.small_mixed(seed=2026, n_sites=24)
            hb = st.host_batch(st.tasks(), Params.ont(genotype=True))
            got = ctx.cluster_batch(hb, per_sig=True).trimmed()
            want = oracle.cluster_batch(hb, per_sig=True).trimmed()
            assert got["n_clusters"] == want["n_clusters"]
            for key in ("call_seg", "call_cluster", "bp1", "bp2", "support", "cipos", "cilen", "search_pos", "seq_pick", "dr", "dv", "gl_idx",
                        "support_off", "support_sig", "cluster_id", "allele_id"):
                assert np.array_equal(got[key], want[key]), key
        rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)
        with bam.BamFile(path) as bf:
            res = extract.task_to_pool(ctx, bf, chrom, t0, t1, crank, *pipe_args(p), seg_of("INS", crank[chrom]), seg_of("DEL", crank[chrom]), seg_base, None,
                                       bed_regions=case["bed"], name_pool=True)
        got = rebuild.rebuild_pool_by_name(ctx, major, nodedup, keep_on_device=False)
        want, rank, first = host_rebuilt(case, path, t0, t1)
        assert res["n_flagged"] == 0 and res["n_records"] == len(rank) == rebuild.name_pool_rows(ctx)
        ranks = rebuild.name_ranks(ctx)
        assert np.array_equal(ranks["rank"], rank) and np.array_equal(ranks["first"], first)
        for key in ("seg_id", "a", "b", "read_id", "seg_count"):
            assert np.array_equal(got[key], want[key]), (k, key)
        auxk = np.where(major[got["seg_id"]] != 0, got["aux"], 0)
        tie_order = np.lexsort((got["aux"], got["read_id"], got["b"], got["a"], auxk, got["seg_id"]))
        assert np.array_equal(got["aux"][tie_order], want["aux"]), k
        sizes.append((res["n_records"], len(got["a"])))
    assert sizes[0] == sizes[2] and sizes[0][0] > 250 and 10 < sizes[1][0] < 40 and sizes[1][1] > 0
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)
