"""The genotyping reads table in device memory (cutesv_amd/csrc/reads.hip.h, cutesv_amd/reads.py).

CPU: the interface (header, exports, bindings, NULL context), reads.table_host against the construction call_bam used inline,
the options of call_bam, its command line and HostBatch.on_device.  GPU: the append against the numpy cut on chunks around every
size at which the kernels change path, the gates column as the keep source, several appends across two growths, the rank gather,
the engine fed from device memory against the same columns from the host, every refusal, and call_bam with reads_table="device"
byte for byte against reads_table="host" - the path the other test files pin to the reference."""
import os
import re

import numpy as np
import pytest

from cutesv_amd import _abi, _lib, bam, bed, call, engine, extract, reads, rebuild
from cutesv_amd.columns import Params, TYPES
import bed_helpers as bh
import call_helpers
import reads_helpers as rh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("csv_reads_reset", "csv_reads_rows", "csv_reads_append_decoded", "csv_reads_append", "csv_reads_get", "csv_reads_batch_columns", "csv_reads_timing")
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ CPU: the interface
def test_header_declares_and_lib_exports_and_binds_the_entries():
    with open(os.path.join(ROOT, "include", "cutesv_hip.h")) as f:
        header = f.read()
    for proto in (r"int csv_reads_reset\(csv_ctx\* ctx, int32_t n_chrom\);", r"int csv_reads_rows\(const csv_ctx\* ctx, int64_t\* n\);",
                  r"int csv_reads_append_decoded\(csv_ctx\* ctx, int32_t chrom, int64_t n_records, const uint8_t\* keep[^,]*, int64_t name_base, int64_t\* n_appended\);",
                  r"int csv_reads_append\(csv_ctx\* ctx, int32_t chrom, int64_t n, const int32_t\* start, const int32_t\* end, const uint8_t\* primary, const int32_t\* id\);",
                  r"int csv_reads_get\(csv_ctx\* ctx, int64_t first, int64_t n, int32_t\* start, int32_t\* end, uint8_t\* primary, int32_t\* id\);",
                  r"int csv_reads_batch_columns\(csv_ctx\* ctx, int32_t flags, int32_t n_chrom, int64_t\* reads_off[^,]*, csv_reads_dev\* out\);",
                  r"int csv_reads_timing\(const csv_ctx\* ctx, float\* ms_append, float\* ms_columns\);"):
        assert re.search(r"^" + proto, header, re.M), proto
    assert re.search(r"CSV_IN_READS_DEVICE = 128\b", header) and re.search(r"CSV_RD_RANK_FROM_NAMES = 1\b", header)
    assert re.search(r"#define CSV_ABI_VERSION 9\b", header) and "} csv_reads_dev;" in header
    bound = {n for n, _, _ in _lib.SYMBOLS}
    L = _lib.lib()
    for name in ENTRIES:
        assert name in bound and hasattr(L, name), name
    assert L.csv_abi_version() == _abi.ABI_VERSION == 9
    assert (_abi.IN_READS_DEVICE, _abi.RD_RANK_FROM_NAMES, reads.RANK_FROM_NAMES) == (128, 1, 1)
    # the flag is the next free bit of csv_batch_in.flags
    assert _abi.IN_READS_DEVICE == 2 * max(_abi.IN_PER_SIG, _abi.IN_READS_SORTED, _abi.IN_SIG_I32, _abi.IN_READS_I32, _abi.IN_DEVICE_COLUMNS, _abi.IN_SIG_DELTA16,
                                           _abi.IN_READS_DELTA16)
    assert L.csv_reads_struct_size(0) == _abi.READS_STRUCT_SIZES[0][1] == 40 and L.csv_reads_struct_size(1) == -1
    for fn in (reads.reset, reads.rows, reads.append_decoded, reads.append, reads.get, reads.batch_columns, reads.timing, reads.table_host):
        assert callable(fn)


def test_a_null_context_is_refused_by_every_entry():
    n, off, dev = np.zeros(1, np.int64), np.zeros(4, np.int64), _abi.ReadsDev()
    col = np.zeros(1, np.int32)
    import ctypes as C
    f = C.c_float(0)
    assert rh.raw("csv_reads_reset", None, 3) == _abi.E_INVALID
    assert rh.raw("csv_reads_rows", None, n.ctypes.data_as(C.POINTER(C.c_int64))) == _abi.E_INVALID
    assert rh.raw("csv_reads_append_decoded", None, 0, 0, None, 0, None) == _abi.E_INVALID
    assert rh.raw("csv_reads_append", None, 0, 1, col.ctypes.data, col.ctypes.data, col.ctypes.data, col.ctypes.data) == _abi.E_INVALID
    assert rh.raw("csv_reads_get", None, 0, 0, None, None, None, None) == _abi.E_INVALID
    assert rh.raw("csv_reads_batch_columns", None, 0, 3, off.ctypes.data, C.byref(dev)) == _abi.E_INVALID
    assert rh.raw("csv_reads_timing", None, C.byref(f), C.byref(f)) == _abi.E_INVALID


def test_table_host_is_the_inline_construction_of_call_bam():
    tasks, ranks = rh.hand_made_tasks()
    got, want = reads.table_host(tasks, ranks, 3), rh.inline_table(tasks, ranks, 3)
    assert set(got) == set(want) == {"reads_off", "r_start", "r_end", "r_primary", "r_id"}
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    # the contract, spelled out: blocks by chromosome, the tasks' order kept inside a block, ids through the rank column
    assert got["reads_off"].tolist() == [0, 5, 5, 8]
    assert got["r_start"].tolist() == [7000, 6500, 8000, 20, 9000, 500, 100, 100]
    assert got["r_end"].tolist() == [7010, 6520, 8030, 5020, 9001, 550, 100, 1000]
    assert got["r_primary"].tolist() == [1, 1, 0, 0, 1, 1, 0, 1]
    assert got["r_id"].tolist() == ranks[[11, 12, 19, 25, 39, 0, 3, 4]].tolist()
    assert reads.table_host([], ranks, 3) == {}
    # decoded_rows: the cut append_decoded makes, with the end saturating
    cols = dict(ref_start=np.array([5, 7, 2 ** 31 - 10], np.int64), ref_end=np.array([9, 7, 2 ** 31 + 5], np.int64), cls=np.array([1, 0, 2], np.uint8))
    d = reads.decoded_rows(cols, [1, 0, 1], 100)
    assert d["start"].tolist() == [5, 2 ** 31 - 10] and d["end"].tolist() == [9, INT32_MAX] and d["primary"].tolist() == [1, 0] and d["id"].tolist() == [100, 102]
    assert [d[k].dtype for k in ("start", "end", "primary", "id")] == [np.int32, np.int32, np.uint8, np.int32]


def test_call_bam_refuses_an_unknown_reads_table_and_the_command_line_takes_the_option(monkeypatch, tmp_path):
    with pytest.raises(ValueError, match="reads_table"):
        call.call_bam("no_such.bam", {}, Params.ont(), reads_table="bogus")
    assert call.DEFAULT_READS_TABLE in ("host", "device")
    seen = []
    monkeypatch.setattr(call, "call_bam", lambda *a, **k: (seen.append(k["reads_table"]), (b"", np.zeros(5, np.int64)))[1])
    from cutesv_amd import fasta
    monkeypatch.setattr(fasta, "Reference", lambda path: path)
    out = str(tmp_path / "o.vcf")
    assert call.main(["a.bam", "ref.fa", "-o", out, "--genotype", "--reads_table", "device"]) == 0
    assert call.main(["a.bam", "ref.fa", "-o", out, "--reads_table", "host"]) == 0
    assert call.main(["a.bam", "ref.fa", "-o", out]) == 0
    assert seen == ["device", "host", None]
    with pytest.raises(SystemExit):
        call.main(["a.bam", "ref.fa", "-o", out, "--reads_table", "bogus"])
    with pytest.raises(ValueError):
        extract.task_to_pool(None, None, "c", 0, 1, {}, 30, 20, 7, 500, 10, 0, 100, 100000, 0, 0, [0] * 5, 0, reads="bogus")
    with pytest.raises(ValueError):
        extract.task_to_pool(None, None, "c", 0, 1, {}, 30, 20, 7, 500, 10, 0, 100, 100000, 0, 0, [0] * 5, 0, reads="device")      # (needs the name pool)


def test_on_device_takes_host_reads_or_device_reads_and_not_both():
    segs = np.zeros(0, _abi.SEGMENT_DTYPE)
    dev = dict(a=0, b=0, read_id=0, aux=0)
    rd = dict(reads_off=np.array([0, 2, 2], np.int64), r_start=4096, r_end=8192, r_primary=12288, r_id=16384, n_reads=2)
    hb = _abi.HostBatch.on_device(segs, dev, 0, n_chrom=2, reads_dev=rd, contig_len=[10, 20])
    assert hb.c.flags == _abi.IN_DEVICE_COLUMNS | _abi.IN_READS_DEVICE | _abi.IN_READS_I32
    assert (hb.c.n_reads, hb.c.r_start, hb.c.r_end, hb.c.r_primary, hb.c.r_id) == (2, 4096, 8192, 12288, 16384)
    assert hb.c.reads_off == hb.reads_off.ctypes.data and hb.c.contig_len == hb.contig_len.ctypes.data
    host = dict(reads_off=np.array([0, 2, 2], np.int64), r_start=np.zeros(2, np.int32), r_end=np.ones(2, np.int32), r_primary=np.ones(2, np.uint8), r_id=np.zeros(2, np.int32))
    assert not _abi.HostBatch.on_device(segs, dev, 0, n_chrom=2, **host).c.flags & _abi.IN_READS_DEVICE
    with pytest.raises(ValueError, match="not both"):
        _abi.HostBatch.on_device(segs, dev, 0, n_chrom=2, reads_dev=rd, **host)
    with pytest.raises(ValueError):
        _abi.HostBatch.on_device(segs, dev, 0, n_chrom=3, reads_dev=rd)                   # reads_off has n_chrom + 1 entries


# ------------------------------------------------------------------------------------------------ GPU: the append against the twin
def _assert_rows(got, want, what):
    for k in ("start", "end", "primary", "id"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("n", rh.CHUNK_SIZES)
def test_gpu_append_decoded_equals_the_numpy_cut(ctx, tmp_path, n):
    chunk, cols = rh.decode_chunk(ctx, tmp_path, n)
    if n >= 255:
        assert {0, 1, 2} <= set(cols["cls"].tolist()) and int(cols["mapq"].min()) == 0 and bool(np.any(cols["ref_end"] == cols["ref_start"]))
    reads.reset(ctx, 2)
    total = 0
    for k, (name, keep) in enumerate(rh.keep_masks(n)):
        base = 1000 * k + 7
        m = reads.append_decoded(ctx, 1, n, base, keep=keep)
        want = reads.decoded_rows(cols, keep, base)
        assert m == int((keep != 0).sum()) == len(want["id"]), name
        assert reads.rows(ctx) == total + m
        _assert_rows(reads.get(ctx, total, m), want, name)
        # the cut, once more in the issue's words
        idx = np.flatnonzero(keep)
        assert want["start"].tolist() == cols["ref_start"][idx].tolist() and want["primary"].tolist() == (cols["cls"][idx] == 1).astype(int).tolist()
        total += m
    rd = reads.batch_columns(ctx, 2)
    assert rd["reads_off"].tolist() == [0, 0, total] and rd["n_reads"] == total
    assert reads.timing(ctx)[0] > 0


@pytest.mark.gpu
def test_gpu_keep_from_the_gates_column_with_and_without_a_bed(ctx, tmp_path):
    n = 1100
    chunk, cols = rh.decode_chunk(ctx, tmp_path, n)
    reads.reset(ctx, 1)
    seen = 0
    for name, regions in (("none", None), ("one", [(bh.B0, bh.B1)]), ("nested", [(40000, 60000), (41000, 42000)]), ("empty", np.zeros((0, 2), np.int64))):
        bits = extract.task_gates(ctx, n, bh.T0, bh.MIN_LEN, bh.MIN_MAPQ, regions)
        assert np.array_equal(bits, extract.gate_bits_host(cols, bh.T0, regions, bh.MIN_LEN, bh.MIN_MAPQ))
        keep = (bits & _abi.GATE_READS) != 0
        first = reads.rows(ctx)
        m_dev = reads.append_decoded(ctx, 0, n, 50)                       # keep=None: the gates column
        m_host = reads.append_decoded(ctx, 0, n, 50, keep=keep)
        assert m_dev == m_host == int(keep.sum()), name
        want = reads.decoded_rows(cols, keep, 50)
        _assert_rows(reads.get(ctx, first, m_dev), want, name)
        _assert_rows(reads.get(ctx, first + m_dev, m_host), want, name)
        assert (m_dev == 0) == (name == "empty")
        seen += m_dev
    assert seen > 300 and reads.rows(ctx) == 2 * seen


@pytest.mark.gpu
def test_gpu_several_appends_grow_the_table_and_keep_its_rows(tmp_path):
    """three tasks on chromosome 0, none on 1, two on 2: about 10 000 rows behind a first allocation of a few thousand.  A context
    of its own: its table has no capacity from earlier tests.  The first append of about 2 080 rows allocates its bytes plus a half
    plus 4 KB (room for about 4 140 rows of a four-byte column); the second append needs 4 160 rows and grows it to about 7 260, the
    fourth needs 8 310 and grows it again: two growths by copying under rows that must survive"""
    ctx = engine.Context(0)
    try:
        _several_appends(ctx, tmp_path)
    finally:
        ctx.close()


def _several_appends(ctx, tmp_path):
    reads.reset(ctx, 3)
    n = 2100
    want = {k: [] for k in ("start", "end", "primary", "id")}
    off = np.zeros(4, np.int64)
    for t, chrom in enumerate((0, 0, 0, 2, 2)):
        _, cols = rh.decode_chunk(ctx, tmp_path, n, seed=21 + t)
        keep = np.ones(n, np.uint8)
        keep[t::97] = 0                                               # (nearly all)
        m = reads.append_decoded(ctx, chrom, n, 10000 * t, keep=keep)
        rows = reads.decoded_rows(cols, keep, 10000 * t)
        assert m == len(rows["id"]) == int(keep.sum())
        for k in want:
            want[k].append(rows[k])
        off[chrom + 1:] += m
        rd = reads.batch_columns(ctx, 3)
        assert rd["reads_off"].tolist() == off.tolist() and rd["n_reads"] == reads.rows(ctx) == int(off[-1])
        got = reads.get(ctx)
        for k in want:
            assert np.array_equal(got[k], np.concatenate(want[k])), (t, k)
        assert np.array_equal(rh.device_to_host(rd["r_start"], rd["n_reads"], np.int32), got["start"])
        assert np.array_equal(rh.device_to_host(rd["r_primary"], rd["n_reads"], np.uint8), got["primary"])
        assert np.array_equal(rh.device_to_host(rd["r_id"], rd["n_reads"], np.int32), got["id"])       # (without the flag: the ids as they are)
    assert reads.rows(ctx) > 10000 and off[1] == off[2]
    # host rows behind them, and an empty append
    reads.append(ctx, 2, [5, 0], [5, INT32_MAX], [3, 0], [1, INT32_MAX])
    reads.append(ctx, 2, [], [], [], [])
    tail = reads.get(ctx, int(off[-1]))
    assert tail["start"].tolist() == [5, 0] and tail["end"].tolist() == [5, INT32_MAX] and tail["primary"].tolist() == [1, 0] and tail["id"].tolist() == [1, INT32_MAX]
    reads.reset(ctx, 3)
    assert reads.rows(ctx) == 0 and reads.batch_columns(ctx, 3)["reads_off"].tolist() == [0, 0, 0, 0]


@pytest.mark.gpu
def test_gpu_rank_column_is_the_name_pools_rank_of_every_id(ctx, tmp_path):
    rebuild.name_pool_reset(ctx)
    reads.reset(ctx, 2)
    n = 700
    ids = []
    for t, seed in enumerate((31, 31, 32)):                           # the first chunk twice: every name occurs in two chunks
        chunk, cols = rh.decode_chunk(ctx, tmp_path, n, seed=seed)
        base = rebuild.name_pool_append_chunk(ctx, chunk)
        keep = (np.arange(n) % 3 != t).astype(np.uint8)
        reads.append_decoded(ctx, min(t, 1), n, base, keep=keep)
        ids.append(base + np.flatnonzero(keep))
    ids = np.concatenate(ids)
    total = len(ids)
    plain = reads.batch_columns(ctx, 2)
    assert np.array_equal(rh.device_to_host(plain["r_id"], total, np.int32), ids)
    rd = reads.batch_columns(ctx, 2, reads.RANK_FROM_NAMES)
    ranks = rebuild.name_ranks(ctx)["rank"]
    assert rd["n_reads"] == total and rd["r_id"] != plain["r_id"]
    got = rh.device_to_host(rd["r_id"], total, np.int32)
    assert np.array_equal(got, ranks[ids])
    assert len(set(got.tolist())) < total                             # duplicate names share a rank
    again = reads.batch_columns(ctx, 2, reads.RANK_FROM_NAMES)
    assert np.array_equal(rh.device_to_host(again["r_id"], total, np.int32), got)
    assert np.array_equal(reads.get(ctx)["id"], ids)                  # the table itself keeps the ids
    # names that sort in front of every other one: the ranks move, and the next call follows
    rebuild.name_pool_append(ctx, b"!a!b", [0, 2], [2, 2])
    moved = reads.batch_columns(ctx, 2, reads.RANK_FROM_NAMES)
    got2 = rh.device_to_host(moved["r_id"], total, np.int32)
    assert np.array_equal(got2, got + 2) and np.array_equal(got2, rebuild.name_ranks(ctx)["rank"][ids])
    assert reads.timing(ctx)[1] > 0
    rebuild.name_pool_reset(ctx)


# ------------------------------------------------------------------------------------------------ GPU: the engine
@pytest.mark.gpu
def test_gpu_engine_takes_the_reads_table_from_device_memory(ctx):
    segs, a, b, rid, aux, contig_len, rd_host = rh.synthetic_batch()
    host = lambda **kw: _abi.HostBatch(segs, a, b, rid, aux, n_chrom=3, contig_len=contig_len, **dict(rd_host, **kw))      # noqa: E731
    want = ctx.cluster_batch(host()).trimmed()
    tra = np.flatnonzero(segs["svtype"] == _abi.TRA)
    in_tra = np.isin(want["call_seg"], tra)
    assert len(want["bp1"]) > 20 and in_tra.any() and (want["gl_idx"] >= 0).any() and (want["dr"] > 0).any()
    reads.reset(ctx, 3)
    o = rd_host["reads_off"]
    for k in range(3):
        s = slice(int(o[k]), int(o[k + 1]))
        reads.append(ctx, k, rd_host["r_start"][s], rd_host["r_end"][s], rd_host["r_primary"][s], rd_host["r_id"][s])
    rd = reads.batch_columns(ctx, 3)
    assert rd["reads_off"].tolist() == o.tolist() and o[1] == o[2] and o[3] - o[2] == 1
    got = ctx.cluster_batch(rh.with_device_reads(host(), rd)).trimmed()
    rh.assert_same_result(got, want)
    # the columns were copied at upload: the table may go, a resident batch still runs on them
    hb = rh.with_device_reads(host(), rd)
    ctx.upload(hb)
    reads.reset(ctx, 3)
    reads.append(ctx, 0, [1], [2], [1], [3])
    ctx.run()
    rh.assert_same_result(ctx.download().trimmed(), want)
    # the forms that read r_start on the host are refused with the flag, and a correct call follows
    reads.reset(ctx, 3)
    for k in range(3):
        s = slice(int(o[k]), int(o[k + 1]))
        reads.append(ctx, k, rd_host["r_start"][s], rd_host["r_end"][s], rd_host["r_primary"][s], rd_host["r_id"][s])
    rd = reads.batch_columns(ctx, 3)
    idp = (rd_host["r_id"].astype(np.uint32) | (rd_host["r_primary"].astype(np.uint32) << 31))
    for kw in (dict(r_delta=_abi.delta16_of(rd_host["r_start"])), dict(r_len16=_abi.len16_of(rd_host["r_start"], rd_host["r_end"])), dict(r_idp=idp)):
        bad = rh.with_device_reads(host(**kw), rd)
        with pytest.raises(engine.CsvError) as e:
            ctx.cluster_batch(bad)
        assert e.value.code == _abi.E_INVALID, kw.keys()
        rh.assert_same_result(ctx.cluster_batch(rh.with_device_reads(host(), rd)).trimmed(), want)
    wide = _abi.HostBatch(segs, a, b, rid, aux, n_chrom=3, contig_len=contig_len, **dict(rd_host, r_start=rd_host["r_start"].astype(np.int64), r_end=rd_host["r_end"].astype(np.int64)))
    wide.c.flags |= _abi.IN_READS_DEVICE                              # without CSV_IN_READS_I32
    with pytest.raises(engine.CsvError) as e:
        ctx.cluster_batch(wide)
    assert e.value.code == _abi.E_INVALID
    rh.assert_same_result(ctx.cluster_batch(host()).trimmed(), want)
    reads.reset(ctx, 3)


def _planted_tasks(ctx, bf, p, reads_mode, gates="device", batch=10_000_000):
    """call_bam's task loop on the planted BAM -> (names, per-task results)"""
    names = sorted(bf.references)
    crank = {c: i for i, c in enumerate(names)}
    length = dict(zip(bf.references, bf.lengths))
    n_chrom = len(names)
    seg_of = {t: ti * n_chrom for ti, t in enumerate(TYPES)}
    seg_base = [seg_of[t] for t in ("DEL", "INS", "DUP", "INV", "TRA")]
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx); reads.reset(ctx, n_chrom)
    out = []
    for c in names:
        for t0, t1 in call.cut_tasks(length[c], batch):
            r = extract.task_to_pool(ctx, bf, c, t0, t1, crank, *p.pipe_args(), seg_of["INS"] + crank[c], seg_of["DEL"] + crank[c], seg_base, None, name_pool=True,
                                     seq_pool=True, gates=gates, reads=reads_mode)
            out.append((crank[c], r))
    return names, out


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = tmp_path_factory.mktemp("readscall")
    path = str(d / "planted.bam")
    ref = call_helpers.write_planted_bam(path)
    bed_path = str(d / "ins.bed")
    with open(bed_path, "w") as f:
        f.write("chrA\t9000\t11000\n")
    return path, ref, bed_path, d


@pytest.mark.gpu
@pytest.mark.parametrize("gates", ["host", "device"])
def test_gpu_tasks_fill_the_table_and_the_planted_batch_clusters_from_it(ctx, planted, gates):
    path = planted[0]
    cp = call.CallParams(Params.ont(min_support=3, genotype=True))
    with bam.BamFile(path) as bf:
        names, host_tasks = _planted_tasks(ctx, bf, cp, "host", gates=gates, batch=7000)
        table = reads.table_host(host_tasks, rebuild.name_ranks(ctx)["rank"], len(names))
        _, dev_tasks = _planted_tasks(ctx, bf, cp, "device", gates=gates, batch=7000)
    for (_, h), (_, d) in zip(host_tasks, dev_tasks):
        assert not [k for k in d if k.startswith("reads_")] and d["n_reads_rows"] == len(h["reads_index"])
        assert {k: d[k] for k in ("n_records", "n_sig_ins", "n_sig_del", "n_split", "name_base")} == {k: h[k] for k in ("n_records", "n_sig_ins", "n_sig_del", "n_split", "name_base")}
    n_chrom = len(names)
    rd = reads.batch_columns(ctx, n_chrom, reads.RANK_FROM_NAMES)
    total = len(table["r_id"])
    assert total == rd["n_reads"] > 40 and np.array_equal(rd["reads_off"], table["reads_off"])
    # the planted tasks arrive grouped by chromosome and in file order: the device table IS the host table, row for row
    for k, dt in (("r_start", np.int32), ("r_end", np.int32), ("r_primary", np.uint8), ("r_id", np.int32)):
        assert np.array_equal(rh.device_to_host(rd[k], total, dt), table[k]), k
    _, _, major, nodedup = rebuild._segments(names, True)
    rb = rebuild.rebuild_pool_by_name(ctx, major, nodedup, keep_on_device=True, ties="seqs")
    p = Params.ont(min_support=3, genotype=True, genotype_tra=True)
    off = np.r_[0, np.cumsum(rb["seg_count"])]
    from cutesv_amd.columns import segment_record
    order = rebuild._segments(names, True)[0]
    segs = np.array([segment_record(TYPES[s // n_chrom], order[s % n_chrom], int(off[s]), int(off[s + 1]), p) for s in np.flatnonzero(rb["seg_count"]).tolist()],
                    dtype=_abi.SEGMENT_DTYPE)
    contig_len = np.array([dict(call_helpers.CONTIGS)[c] for c in names], np.int64)
    rd = reads.batch_columns(ctx, n_chrom, reads.RANK_FROM_NAMES)     # (after the rebuild: the addresses of this call are the valid ones)
    got = ctx.cluster_batch(_abi.HostBatch.on_device(segs, rb["dev"], rb["n_out"], n_chrom=n_chrom, keep=ctx, reads_dev=rd, contig_len=contig_len)).trimmed()
    narrow = dict(table, r_start=table["r_start"].astype(np.int32), r_end=table["r_end"].astype(np.int32))
    for t in (table, narrow):                                          # int64 columns (call_bam's host path) and int32 ones
        want = ctx.cluster_batch(_abi.HostBatch.on_device(segs, rb["dev"], rb["n_out"], n_chrom=n_chrom, keep=ctx, contig_len=contig_len, **t)).trimmed()
        rh.assert_same_result(got, want)
    assert len(got["bp1"]) >= 5 and (got["gl_idx"] >= 0).any()
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx); reads.reset(ctx, n_chrom)


# ------------------------------------------------------------------------------------------------ GPU: refusals
def refused(fn, *a, **kw):
    with pytest.raises(engine.CsvError) as e:
        fn(*a, **kw)
    assert e.value.code == _abi.E_INVALID, e.value


@pytest.mark.gpu
def test_gpu_every_refusal_leaves_the_table_as_it_was(tmp_path):
    c = engine.Context(0)
    try:
        n = 257
        # no csv_reads_reset yet
        refused(reads.append, c, 0, [1], [2], [1], [0])
        refused(reads.batch_columns, c, 0)
        refused(reads.append_decoded, c, 0, 0, 0, keep=np.zeros(0, np.uint8))
        reads.reset(c, 3)
        refused(reads.reset, c, -1)
        # no decode
        refused(reads.append_decoded, c, 0, n, 0, keep=np.ones(n, np.uint8))
        chunk, cols = rh.decode_chunk(c, tmp_path, n)
        keep = (np.arange(n) % 5 != 0).astype(np.uint8)
        want = reads.decoded_rows(cols, keep, 40)

        def works(first):
            """a correct append on chromosome 1 lands behind `first` rows"""
            assert reads.rows(c) == first
            assert reads.append_decoded(c, 1, n, 40, keep=keep) == len(want["id"])
            _assert_rows(reads.get(c, first), want, first)
            assert reads.batch_columns(c, 3)["reads_off"].tolist() == [0, 0, first + len(want["id"]), first + len(want["id"])]
            return first + len(want["id"])
        rows = works(0)
        refused(reads.append_decoded, c, 1, n, 40)                                           # keep=None, no gates on this decode
        rows = works(rows)
        for chrom in (3, -1, 0):                                                            # outside the table; below the last row's
            refused(reads.append_decoded, c, chrom, n, 40, keep=keep)
            refused(reads.append, c, chrom, [1], [2], [1], [0])
            rows = works(rows)
        for bad_n in (n - 1, n + 1, 0):                                                     # not the decode's
            refused(reads.append_decoded, c, 1, bad_n, 40, keep=np.ones(bad_n, np.uint8))
        rows = works(rows)
        for base in (-1, INT32_MAX - n + 1, 2 ** 40):
            refused(reads.append_decoded, c, 1, n, base, keep=keep)
        assert reads.append_decoded(c, 1, n, INT32_MAX - n, keep=np.r_[np.zeros(n - 1, np.uint8), 1]) == 1      # the largest id there is
        assert reads.get(c, rows)["id"].tolist() == [INT32_MAX - 1]
        rows = works(rows + 1)
        for row in (([-1], [5], [1], [0]), ([6], [5], [1], [0]), ([1], [5], [1], [-1])):
            refused(reads.append, c, 1, *row)
            refused(reads.append, c, 1, *[[3] + v for v in row])                            # (behind a good row: nothing of the call lands)
        rows = works(rows)
        for first, cnt in ((-1, 1), (0, rows + 1), (rows + 1, 0), (rows, 1)):
            refused(reads.get, c, first, cnt)
        assert len(reads.get(c, rows, 0)["id"]) == 0
        refused(reads.batch_columns, c, 2)
        refused(reads.batch_columns, c, 4)
        refused(reads.batch_columns, c, 3, 2)
        refused(reads.batch_columns, c, 3, reads.RANK_FROM_NAMES | 4)
        rows = works(rows)
        # ranks: an id at or beyond the name pool's row count (the pool is empty; then one name short)
        rebuild.name_pool_reset(c)
        refused(reads.batch_columns, c, 3, reads.RANK_FROM_NAMES)
        rebuild.name_pool_append_chunk(c, chunk)
        refused(reads.batch_columns, c, 3, reads.RANK_FROM_NAMES)                            # (ids reach 40 + n - 1 and INT32_MAX - 1)
        rows = works(rows)
        reads.reset(c, 3)
        reads.append_decoded(c, 1, n, 0, keep=keep)
        ranks = rebuild.name_ranks(c)["rank"]
        rd = reads.batch_columns(c, 3, reads.RANK_FROM_NAMES)
        assert np.array_equal(rh.device_to_host(rd["r_id"], rd["n_reads"], np.int32), ranks[np.flatnonzero(keep)])
        reads.append(c, 2, [1], [2], [0], [n])                                              # one beyond the pool
        refused(reads.batch_columns, c, 3, reads.RANK_FROM_NAMES)
        assert reads.batch_columns(c, 3)["n_reads"] == int(keep.sum()) + 1
        # the gates belong to their decode: after a second decode keep=None is refused until task_gates ran again
        reads.reset(c, 3)
        bits = extract.task_gates(c, n, bh.T0, bh.MIN_LEN, bh.MIN_MAPQ)
        m = reads.append_decoded(c, 0, n, 0)
        assert m == int(((bits & _abi.GATE_READS) != 0).sum()) > 0
        chunk2, cols2 = rh.decode_chunk(c, tmp_path, n, seed=12)
        refused(reads.append_decoded, c, 0, n, 0)
        assert reads.rows(c) == m
        bits2 = extract.task_gates(c, n, bh.T0, bh.MIN_LEN, bh.MIN_MAPQ)
        assert reads.append_decoded(c, 0, n, 0) == int(((bits2 & _abi.GATE_READS) != 0).sum())
        _assert_rows(reads.get(c, m), reads.decoded_rows(cols2, (bits2 & _abi.GATE_READS) != 0, 0), "second decode")
        # an empty chunk: nothing to launch, either way
        with bam.BamFile(str(tmp_path / ("reads%d_12.bam" % n))) as bf:
            empty = bf.records("7", 190000, 190001)
        assert empty.n == 0
        bam.decode(c, empty, host_outputs=False)
        before = reads.rows(c)
        assert reads.append_decoded(c, 0, 0, 0, keep=np.zeros(0, np.uint8)) == 0
        extract.task_gates(c, 0, 0, 0, 0)
        assert reads.append_decoded(c, 0, 0, 0) == 0 and reads.rows(c) == before
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ GPU: end to end
def _records(text):
    return [ln.split("\t") for ln in text.splitlines()]


@pytest.mark.gpu
@pytest.mark.parametrize("gates", ["host", "device"])
@pytest.mark.parametrize("tra_gt", ["alignments", "reads_table", "off"])
@pytest.mark.parametrize("batch", [10_000_000, 2000])
def test_gpu_call_bam_with_the_device_table_is_byte_identical(ctx, planted, batch, tra_gt, gates):
    path, ref = planted[0], planted[1]
    cp = call.CallParams(Params.ont(min_support=3, genotype=True))
    with bam.BamFile(path) as bf:
        for report_readid in (False, True):
            kw = dict(ctx=ctx, batch=batch, report_readid=report_readid, tra_gt=tra_gt, gates=gates)
            want, svid_w = call.call_bam(bf, ref, cp, reads_table="host", **kw)
            got, svid = call.call_bam(bf, ref, cp, reads_table="device", **kw)
            assert got == want and svid.tolist() == svid_w.tolist()
            recs = _records(want)
            kinds = [re.search(r"SVTYPE=(\w+)", r[7]).group(1) for r in recs]
            assert {"INS", "DEL", "DUP", "BND"} <= set(kinds)
            gts = [r[9].split(":")[0] for r, k in zip(recs, kinds) if k != "BND"]
            assert any(g not in ("./.", "0/0") for g in gts)                  # genotypes were made from the table
            bnd = [r[9].split(":")[0] for r, k in zip(recs, kinds) if k == "BND"]
            assert bnd and (all(g == "./." for g in bnd) if tra_gt == "off" else tra_gt != "alignments" or any(g != "./." for g in bnd))
    assert reads.rows(ctx) > 40                                               # the device call left its table in the context


@pytest.mark.gpu
def test_gpu_call_bam_device_table_with_a_bed_one_contig_and_without_genotype(ctx, planted, tmp_path):
    path, ref, bed_path, d = planted
    cp = call.CallParams(Params.ont(min_support=3, genotype=True))
    at = lambda text: [r for r in _records(text) if r[0] == "chrA" and abs(int(r[1]) - 10000) <= 5]      # noqa: E731
    support = lambda rec: int(re.search(r"RE=(\d+)", rec[7]).group(1))                                   # noqa: E731
    with bam.BamFile(path) as bf:
        kw = dict(ctx=ctx, tra_gt="reads_table")
        full, _ = call.call_bam(bf, ref, cp, reads_table="device", **kw)
        rows_full = reads.rows(ctx)
        out, rows = {}, {}
        for batch in (10_000_000, 2000):
            want, _ = call.call_bam(bf, ref, cp, reads_table="host", include_bed=bed_path, batch=batch, **kw)
            out[batch], _ = call.call_bam(bf, ref, cp, reads_table="device", include_bed=bed_path, batch=batch, **kw)
            rows[batch] = reads.rows(ctx)
            assert out[batch] == want and len(at(want)) == 1
            assert call.call_bam(bf, ref, cp, reads_table="device", include_bed=bed_path, batch=batch, gates="host", **kw)[0] == want
        # fewer rows with the BED; the task cut drops reads that start in the task in front of the region's
        assert 0 < rows[2000] < rows[10_000_000] < rows_full
        assert support(at(out[2000])[0]) < support(at(out[10_000_000])[0]) == support(at(full)[0])
        assert at(out[10_000_000])[0][9].split(":")[0] not in ("./.", "0/0")
        # a leading chromosome without rows (chrA < chrB in name order)
        only_b = call.call_bam(bf, ref, cp, reads_table="device", chroms=["chrB"], **kw)
        assert only_b[0] == call.call_bam(bf, ref, cp, reads_table="host", chroms=["chrB"], **kw)[0]
        off_b = reads.batch_columns(ctx, 2)["reads_off"].tolist()
        assert off_b[0] == off_b[1] == 0 and off_b[2] == reads.rows(ctx) >= 8
        # without genotype the option does nothing: no table is made
        plain = call.CallParams(Params.ont(min_support=3))
        reads.reset(ctx, 2)
        assert call.call_bam(bf, ref, plain, ctx=ctx, reads_table="device")[0] == call.call_bam(bf, ref, plain, ctx=ctx, reads_table="host")[0] != ""
        assert reads.rows(ctx) == 0
        # an empty BED: nothing on either side
        empty = str(d / "empty.bed")
        open(empty, "w").close()
        assert call.call_bam(bf, ref, cp, reads_table="device", include_bed=empty, **kw)[0] == "" == call.call_bam(bf, ref, cp, reads_table="host", include_bed=empty, **kw)[0]
        want_cli, _ = call.call_bam(bf, ref, call.CallParams(Params.ont(min_support=3, genotype=True)), ctx=ctx, reads_table="host", tra_gt="alignments", as_bytes=True)
    # the command line writes the same file
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as f:
        for c, s in ref.items():
            f.write(">%s\n" % c + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")
    files = {}
    for mode in ("device", "host"):
        files[mode] = str(tmp_path / (mode + ".body.vcf"))
        assert call.main([path, fa, "-o", files[mode], "--preset", "ont", "--min_support", "3", "--genotype", "--reads_table", mode]) == 0
    with open(files["device"], "rb") as f, open(files["host"], "rb") as g:
        body = f.read()
        assert body == g.read() == want_cli and body.count(b"\n") >= 5
