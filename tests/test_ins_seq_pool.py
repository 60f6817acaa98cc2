"""The INS sequence pool (cutesv_amd/csrc/seqs.hip.h): the inserted bases of every INS pool row cut out
of the reads' 4-bit sequences on the GPU, the rebuild's INS tie groups settled from them on the device, bases by pool row.

CPU: the host checker `extract.pool_ins_sequences_host` against the strings the reference recorded (parse_reads / single_pipe /
split_sigs goldens), `Chunk.sequence_columns` against `Chunk.sequence`, the argument checks.  GPU: the kernels against the
checker, `task_to_pool(seq_pool=True)` against `single_pipe_bam`, `ties="seqs"` against the reference's order and against
`rebuild.tie_callback`, misuse, device memory."""
import ctypes as C

import numpy as np
import pytest

from cutesv_amd import bam, extract, rebuild, synth, _abi, _lib
from cutesv_amd.columns import TYPES
from helpers import load_json, split_case_inputs, StubRecord, rebuild_case_inputs, rebuild_expected
import bam_writer
from seq_pool_helpers import rebuild_case_pool

REF_LEN = {"1": 248956422, "10": 133797422, "2": 242193529, "7": 159345973, "X": 156040895}
CODES = "=ACMGRSVTWYHKDBN"
_PACK = bytes.maketrans(CODES.encode(), bytes(range(16)))


def _oracle():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def pack4(seqs):
    """test-local: sequences -> (uint8 image, off int64[n], l_seq int32[n]) in the BAM 4-bit encoding, high nibble first"""
    parts, off, at = [], [], 0
    for s in seqs:
        codes = s.encode().translate(_PACK) + b"\0"
        p = bytes(hi << 4 | lo for hi, lo in zip(codes[0:len(s):2], codes[1:len(s) + 1:2]))
        parts.append(p); off.append(at); at += len(p)
    return np.frombuffer(b"".join(parts) + b"\0", np.uint8), np.asarray(off, np.int64), np.asarray([len(s) for s in seqs], np.int32)


def revcomp(s):
    return s.translate(extract._COMP)[::-1]


def pipe_args(p):
    return (p["sv"], p["min_mapq"], p["parts"], p["min_read_len"], p["min_siglength"], p["md"], p["mi"], p["max_size"])


def golden_records(case, chrom):
    refs = [(c, REF_LEN[c]) for c in case["chroms"]]
    refid = case["chroms"].index(chrom)
    return refs, [dict(d, seq=synth.pseudo_sequence(d["seq_len"], d["seq_key"]), refid=refid, tags=[tuple(t) for t in d["tags"]]) for d in case["reads"]]


# ------------------------------------------------------------------------------------------------ CPU: the checker, CIGAR side
def cigar_cases():
    """(name, the reads parse_read sees in order, params, golden INS tuples) of the five parse_reads / single_pipe cases"""
    out = []
    for case in load_json("parse_reads.json.gz"):
        out.append((case["name"], [StubRecord(d) for d in case["reads"]], case["params"], case["INS"]))
    for case in load_json("single_pipe.json.gz"):
        recs = [r for r in (StubRecord(d) for d in case["reads"]) if r.flag not in (256, 272)]
        start = np.asarray([r.reference_start for r in recs], np.int64)
        keep = start >= case["task"][1]
        if case["bed"] is not None:
            keep &= extract._in_bed(start, np.asarray([r.reference_end for r in recs], np.int64), case["bed"])
        out.append((case["name"], [r for r, k in zip(recs, keep.tolist()) if k], case["params"], case["INS"]))
    return out


def test_checker_equals_the_golden_ins_sequences_of_the_cigar_scan():
    counts, multi = [], []
    for name, recs, p, golden in cigar_cases():
        keep = [r for r in recs if r.query_length >= p["min_read_len"]]
        off, flat = extract.encode_cigars([r.cigartuples for r in keep])
        sig = _oracle().cigar_signatures(off, flat, np.asarray([r.reference_start for r in keep], np.int64),
                                         np.asarray([1 if r.mapq >= p["min_mapq"] else 0 for r in keep], np.uint8),
                                         min_siglength=p["min_siglength"], merge_ins_threshold=p["mi"], merge_del_threshold=p["md"])
        got = extract.pool_ins_sequences_host([r.query_sequence for r in keep], [r.flag == 16 for r in keep], sig, None)
        assert [b.decode() for b, _ in got] == [x[3] for x in golden], name
        assert all(h == 0 for _, h in got) and all(type(x[0]) is int for x in golden), name       # (no split-read INS in these cases)
        counts.append(len(got)); multi.append(int((sig["ins_npiece"] > 1).sum()))
        assert int(sig["ins_npiece"].max()) <= 8
    assert counts == [285, 1266, 135, 96, 50], counts
    assert multi == [27, 393, 27, 9, 5], multi                     # multi-piece rows (27 .. 393 in the parse_reads cases, 9 and 5 in the two task regions)


# ------------------------------------------------------------------------------------------------ CPU: the checker, split side
def test_checker_equals_the_golden_ins_sequences_of_the_split_analysis():
    cases = load_json("split_sigs.json.gz")
    assert len(cases) == 9
    total, by_aux, clipped = 0, [0, 0, 0, 0], 0
    for case in cases:
        enc, _, queries, _, kw = split_case_inputs(case)
        ssig = _oracle().split_signatures(enc, **kw)
        want = [(x[3], int(x[0] != int(x[0]))) for x in case["INS"]]
        # the golden queries are what parse_read hands on; stored as they are (flag 0), and stored reverse-complemented (flag 16)
        for stored, rev in ((queries, [0] * len(queries)), ([revcomp(q) for q in queries], [1] * len(queries))):
            got = extract.pool_ins_sequences_host(stored, rev, None, ssig)
            assert [(b.decode(), h) for b, h in got] == want, case["name"]
        ins = ssig["kind"] == 1
        total += int(ins.sum())
        for v in range(4):
            by_aux[v] += int(((ssig["aux"][ins] & 3) == v).sum())
        ql = np.asarray([len(q) for q in queries], np.int64)[ssig["read"][ins]]
        clipped += int(((ssig["d"][ins] > ql) | (ssig["c"][ins] > ql) | (ssig["d"][ins] <= ssig["c"][ins])).sum())
        # the pool rows' aux is the length of these strings
        rows = extract.pool_rows_of_split(ssig, [0] * 5, 0, [len(q) for q in queries])
        assert rows["aux"][ins].tolist() == [len(s) for s, _ in want], case["name"]
    assert total == 414 and by_aux == [87, 60, 213, 54] and clipped == 4, (total, by_aux, clipped)


# ------------------------------------------------------------------------------------------------ CPU: Chunk.sequence_columns
def test_sequence_columns_reproduce_chunk_sequence(tmp_path):
    rng = np.random.default_rng(5)
    seqs = ["", "G", "TN", CODES, CODES[::-1] + "A", "".join(CODES[i] for i in rng.integers(0, 16, 301)), "".join(CODES[i] for i in rng.integers(0, 16, 1000))]
    recs = [dict(name="r%d" % i + "x" * i, flag=0, mapq=60, start=100 + 10 * i, cigar=[(0, max(1, len(s)))], seq=s, tags=[], refid=0) for i, s in enumerate(seqs)]
    path = str(tmp_path / "s.bam")
    bam_writer.write_bam(path, [("1", 10 ** 6)], recs)
    with bam.BamFile(path) as bf:
        (ch,) = list(bf.chunks("1"))
    off, l_seq = ch.sequence_columns()
    assert off.dtype == np.int64 and l_seq.dtype == np.int32 and len(off) == len(l_seq) == ch.n == len(seqs)
    assert l_seq.tolist() == [len(s) for s in seqs]
    for i, s in enumerate(seqs):
        packed = ch.host[off[i]:off[i] + (l_seq[i] + 1) // 2]
        both = np.stack([packed >> 4, packed & 15], 1).ravel()[:l_seq[i]]
        assert "".join(CODES[k] for k in both.tolist()) == s == ch.sequence(i), i
    assert set("".join(seqs)) == set(CODES)


# ------------------------------------------------------------------------------------------------ CPU: the interface
def test_abi_has_the_sequence_entries_and_is_still_9():
    names = {n for n, _, _ in _lib.SYMBOLS}
    assert {"csv_seq_reads_upload", "csv_seq_query_reverse", "csv_seq_pool_rows", "csv_seq_pool_put", "csv_seq_pool_get", "csv_seq_pool_half", "csv_seq_info_get",
            "csv_seq_struct_size"} <= names
    L = _lib.lib()
    assert L.csv_abi_version() == _abi.ABI_VERSION == 9
    assert [L.csv_seq_struct_size(i) for i in range(len(_abi.SEQ_STRUCT_SIZES) + 1)] == [s for _, s in _abi.SEQ_STRUCT_SIZES] + [-1]
    assert _abi.CG_SEQ_TO_POOL == 8 and _abi.RB_TIES_FROM_SEQS == 8
    assert _abi.CG_SEQ_TO_POOL & (_abi.CG_TO_POOL | _abi.CG_FROM_BAM | _abi.SP_FROM_BAM) == 0
    # a NULL context is refused before anything else is looked at
    assert L.csv_seq_reads_upload(None, 0, None, 0, None, None, None) == _abi.E_INVALID
    assert L.csv_seq_pool_get(None, 0, None, None, 0, None) == _abi.E_INVALID


def test_the_new_options_are_refused_where_they_make_no_sense():
    major = np.zeros(2, np.uint8)
    cb = rebuild.tie_callback(lambda r: "", lambda r: 0)
    with pytest.raises(ValueError):
        rebuild.rebuild_pool(None, [0], major, major, ties="seqs", tie_order=cb)          # ... excludes a callback
    with pytest.raises(ValueError):
        rebuild.rebuild_pool(None, [0], major, None, ties="seqs")                         # ... needs seg_nodedup
    with pytest.raises(ValueError):
        rebuild.rebuild_pool_by_name(None, major, major, ties="host")
    with pytest.raises(ValueError):
        rebuild._rebuild(None, 0, dict(), None, major, major, False, None, ties="seqs")   # ... needs the pool
    with pytest.raises(ValueError):
        extract.upload_read_sequences(None, b"\x12", [0], [1, 1])
    with pytest.raises(ValueError):
        extract.upload_read_sequences(None, b"\x12", [0], [1], want=[1, 0])
    with pytest.raises(ValueError):
        rebuild.seq_pool_put(None, [0, 1], ["A"])


# ------------------------------------------------------------------------------------------------ GPU: gather edges
def all_codes(n, key):
    rng = np.random.default_rng(key)
    return "".join(CODES[i] for i in rng.integers(0, 16, n))


def edge_batch():
    """hand-built CIGARs -> (cigartuples per read, sequences).  min_siglength 1, merge threshold 0 unless a read says otherwise."""
    lens = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257]
    reads, seqs = [], []
    # every length at an even and at an odd query offset (30M / 31M in front), far enough apart not to merge
    for lead in (30, 31):
        cig, q = [(0, lead)], lead
        for ln in lens:
            cig += [(1, ln), (0, 500)]; q += ln + 500
        reads.append(cig); seqs.append(all_codes(q, 10 + lead))
    # a piece that ends at the last base of an odd-length read
    reads.append([(0, 40), (1, 61)]); seqs.append(all_codes(101, 3))
    # eight pieces merged into one signature (2M between them), odd and even offsets
    reads.append([(0, 11)] + [x for k in range(8) for x in ((1, 3 + k), (0, 2))]); seqs.append(all_codes(11 + sum(3 + k for k in range(8)) + 16, 4))
    # a piece clipped by the query length: the CIGAR claims 50 inserted bases, the sequence ends after 20 of them
    reads.append([(0, 25), (1, 50), (0, 10)]); seqs.append(all_codes(45, 5))
    # a read without a sequence (l_seq = 0): empty pieces
    reads.append([(0, 10), (1, 12), (0, 10)]); seqs.append("")
    return reads, seqs


@pytest.mark.gpu
def test_gpu_gather_edges(ctx):
    reads, seqs = edge_batch()
    assert set("".join(seqs)) == set(CODES)
    off, flat = extract.encode_cigars(reads)
    start = 1000 * np.arange(len(reads), dtype=np.int64)
    kw = dict(min_siglength=1, merge_ins_threshold=2, merge_del_threshold=0)
    want_sig = _oracle().cigar_signatures(off, flat, start, None, **kw)
    assert int(want_sig["ins_npiece"].max()) == 8
    want = extract.pool_ins_sequences_host(seqs, None, want_sig, None)
    assert {len(b) for b, _ in want} >= {0, 1, 2, 3, 4, 5, 20, 61, 63, 64, 65, 255, 256, 257}
    img, s_off, l_seq = pack4(seqs)
    rebuild.pool_reset(ctx)
    rebuild.pool_append(ctx, [7], [1], [1], [0], [0])                       # a row in front: pool rows and new rows are not the same numbers
    extract.upload_read_sequences(ctx, img, s_off, l_seq)
    sig = extract.cigar_signatures(ctx, off, flat, start, pool=dict(seg_ins=0, seg_del=1, read_base=0, query_len=l_seq, seqs=True), **kw)
    n_ins = sig["n_sig_ins"]
    assert n_ins == len(want) == 2 * 11 + 4 and rebuild.pool_rows(ctx) == 1 + n_ins + sig["n_sig_del"]
    rows = 1 + np.arange(n_ins)
    got = rebuild.seq_pool_get(ctx, rows, raw=True)
    for k, (g, (w, _)) in enumerate(zip(got, want)):
        assert g == w, (k, len(g), len(w))
    assert not rebuild.seq_pool_half(ctx, rows).any()
    assert rebuild.seq_pool_rows(ctx) == (n_ins, sum(len(b) for b, _ in want))
    assert rebuild.seq_pool_get(ctx, rows[::-1][:5]) == [b.decode() for b, _ in want[::-1][:5]]
    rebuild.pool_reset(ctx)
    assert rebuild.seq_pool_rows(ctx) == (0, 0)
    # without query_len the pieces are clipped to the uploaded l_seq: the same rows, the same bases
    sig = extract.cigar_signatures(ctx, off, flat, start, pool=dict(seg_ins=0, seg_del=1, read_base=0, seqs=True), host_outputs=False, **kw)
    assert sig["n_sig_ins"] == n_ins and rebuild.seq_pool_get(ctx, np.arange(n_ins), raw=True) == [b for b, _ in want]
    assert pool_columns(ctx, 2)["aux"][:n_ins].tolist() == [len(b) for b, _ in want]
    rebuild.pool_reset(ctx)


# ------------------------------------------------------------------------------------------------ GPU: split path
@pytest.mark.gpu
@pytest.mark.parametrize("reverse", (0, 1))
def test_gpu_split_candidates_get_their_bases_and_half_flags(ctx, reverse):
    for case in load_json("split_sigs.json.gz"):
        enc, _, queries, _, kw = split_case_inputs(case)
        stored = [revcomp(q) for q in queries] if reverse else queries
        rev = np.full(len(queries), reverse, np.uint8)
        img, s_off, l_seq = pack4(stored)
        rebuild.pool_reset(ctx)
        extract.upload_read_sequences(ctx, img, s_off, l_seq)
        ssig = extract.split_signatures(ctx, enc, pool=dict(seg_base=[0, 4, 8, 12, 16], read_base=0, query_len=l_seq, seqs=True, query_reverse=rev), **kw)
        want = extract.pool_ins_sequences_host(stored, rev, None, ssig)
        assert [(b.decode(), h) for b, h in want] == [(x[3], int(x[0] != int(x[0]))) for x in case["INS"]], case["name"]
        rows = np.flatnonzero(ssig["kind"] == 1)
        assert rebuild.pool_rows(ctx) == len(ssig["kind"])
        assert rebuild.seq_pool_get(ctx, rows, raw=True) == [b for b, _ in want], case["name"]
        assert rebuild.seq_pool_half(ctx, rows).tolist() == [h for _, h in want], case["name"]
        assert rebuild.seq_pool_rows(ctx)[0] == len(rows)
    rebuild.pool_reset(ctx)


# ------------------------------------------------------------------------------------------------ GPU: task_to_pool(seq_pool=True)
def segments_of(n_chrom):
    seg_of = lambda t, ci: TYPES.index(t) * n_chrom + ci                        # noqa: E731
    return seg_of, [seg_of(t, 0) for t in ("DEL", "INS", "DUP", "INV", "TRA")]


def pool_columns(ctx, n_seg):
    """the pool's rows in pool order, through a rebuild that keeps every row"""
    n = rebuild.pool_rows(ctx)
    ident = np.arange(1 << 16, dtype=np.int32)
    r = rebuild.rebuild_pool(ctx, ident, np.zeros(n_seg, np.uint8), np.ones(n_seg, np.uint8), keep_on_device=False)
    assert r["n_out"] == n
    back = np.argsort(r["src_row"], kind="stable")
    return {k: r[k][back] for k in ("seg_id", "a", "b", "read_id", "aux")}


@pytest.mark.gpu
@pytest.mark.parametrize("which", (0, 1))
def test_gpu_task_to_pool_with_sequences(ctx, tmp_path, which):
    case = load_json("single_pipe.json.gz")[which]
    p, (chrom, t0, t1) = case["params"], case["task"]
    rank = {c: i for i, c in enumerate(case["chroms"])}
    n_chrom = len(case["chroms"])
    seg_of, seg_base = segments_of(n_chrom)
    refs, recs = golden_records(case, chrom)
    path = str(tmp_path / "t.bam")
    bam_writer.write_bam(path, refs, recs)
    args = (chrom, t0, t1, rank, *pipe_args(p), seg_of("INS", rank[chrom]), seg_of("DEL", rank[chrom]), seg_base, 0)
    with bam.BamFile(path) as bf:
        rebuild.pool_reset(ctx)
        extract.task_to_pool(ctx, bf, *args, bed_regions=case["bed"])
        plain = pool_columns(ctx, len(TYPES) * n_chrom)
        rebuild.pool_reset(ctx)
        res = extract.task_to_pool(ctx, bf, *args, bed_regions=case["bed"], seq_pool=True)
        with_seq = pool_columns(ctx, len(TYPES) * n_chrom)
        cand, _ = extract.single_pipe_bam(ctx, bf, chrom, t0, t1, rank, *pipe_args(p), bed_regions=case["bed"])
        ch = bf.records(chrom, t0, t1)
    for k in plain:
        assert np.array_equal(plain[k], with_seq[k]), k
    is_ins = (with_seq["seg_id"] >= seg_base[1]) & (with_seq["seg_id"] < seg_base[1] + n_chrom)
    rows = np.flatnonzero(is_ins)
    assert res["n_seq_rows"] == len(rows) == len(cand["INS"]) > 40 and res["n_flagged"] == 0
    got = rebuild.seq_pool_get(ctx, rows)
    half = rebuild.seq_pool_half(ctx, rows)
    # pool order is CIGAR rows, then split rows; single_pipe's list is in read order: compare as (read, pos, len, seq, half) sets with counts
    names = [ch.name(i) for i in range(ch.n)]
    mine = sorted((names[with_seq["read_id"][r]], int(with_seq["a"][r]), int(with_seq["b"][r]), s, int(h)) for r, s, h in zip(rows.tolist(), got, half.tolist()))
    theirs = sorted((x[2], int(x[0]), int(x[1]), x[3], int(x[0] != int(x[0]))) for x in cand["INS"])
    assert mine == theirs
    assert res["n_seq_bytes"] == sum(len(s) for s in got)
    rebuild.pool_reset(ctx)


@pytest.mark.gpu
def test_gpu_flagged_calls_ins_rows_get_their_sequences_from_the_host(ctx, tmp_path):
    """one SA value outside the strict grammar (a leading '+' on the position) on a read whose split analysis yields an INS:
    its rows are appended on the host and their sequences put beside them"""
    case = next(c for c in load_json("split_sigs.json.gz") if c["name"] == "mixture")
    enc, _, queries, chroms, kw = split_case_inputs(case)
    ssig = _oracle().split_signatures(enc, **kw)
    ins_reads = sorted(set(ssig["read"][ssig["kind"] == 1].tolist()))
    picks = [r for r in ins_reads if case["reads"][r]["primary"] and case["reads"][r]["primary"][4] == "1"][:6]
    assert len(picks) >= 2
    rank = {c: i for i, c in enumerate(chroms)}
    recs = []
    for k, r in enumerate(picks):
        d = case["reads"][r]
        c0, c1, f0, f1, _, strand = d["primary"]
        left, right = (c0, d["qlen"] - c1) if strand == "+" else (d["qlen"] - c1, c0)
        q_span, r_span = c1 - c0, f1 - f0                                   # the aligned part: one gap in the middle makes both spans come out
        m = min(q_span, r_span)
        gap = [(2, r_span - q_span)] if r_span > q_span else [(1, q_span - r_span)] if q_span > r_span else []
        cig = ([(4, left)] if left else []) + [(0, m // 2)] + gap + [(0, m - m // 2)] + ([(4, right)] if right else [])
        assert sum(n for o, n in cig if o in (0, 1, 4)) == d["qlen"] and sum(n for o, n in cig if o in (0, 2)) == r_span
        sa = d["sa"] if k else d["sa"].replace(",", ",+", 1)                 # the first read's tag: "chr,+pos,..." - int() takes it, the device flags it
        stored = queries[r] if strand == "+" else revcomp(queries[r])
        recs.append(dict(name=d["name"], flag=0 if strand == "+" else 16, mapq=60, start=f0, cigar=cig, seq=stored, tags=[("SA", sa)], refid=chroms.index("1")))
    recs.sort(key=lambda x: x["start"])
    path = str(tmp_path / "f.bam")
    bam_writer.write_bam(path, [(c, REF_LEN[c]) for c in chroms], recs)
    p = case["params"]
    seg_of, seg_base = segments_of(len(chroms))
    args = ("1", 0, 1 << 40, rank, p["sv"], p["min_mapq"], p["parts"], 0, 10, 0, 100, p["max_size"], seg_of("INS", rank["1"]), seg_of("DEL", rank["1"]), seg_base, 0)
    with bam.BamFile(path) as bf:
        rebuild.pool_reset(ctx)
        res = extract.task_to_pool(ctx, bf, *args, seq_pool=True)
        cand, _ = extract.single_pipe_bam(ctx, bf, *args[:12])
        ch = bf.records("1", 0, 1 << 40)
    assert res["n_flagged"] == 1 and res["n_split_host"] > 0
    cols = pool_columns(ctx, len(TYPES) * len(chroms))
    rows = np.flatnonzero((cols["seg_id"] >= seg_base[1]) & (cols["seg_id"] < seg_base[1] + len(chroms)))
    host_rows = rows[rows >= rebuild.pool_rows(ctx) - res["n_split_host"]]
    assert len(host_rows) > 0 and res["n_seq_rows"] == len(rows) == len(cand["INS"])
    names = [ch.name(i) for i in range(ch.n)]
    got, half = rebuild.seq_pool_get(ctx, rows), rebuild.seq_pool_half(ctx, rows)
    mine = sorted((names[cols["read_id"][r]], int(cols["a"][r]), int(cols["b"][r]), s, int(h)) for r, s, h in zip(rows.tolist(), got, half.tolist()))
    assert mine == sorted((x[2], int(x[0]), int(x[1]), x[3], int(x[0] != int(x[0]))) for x in cand["INS"])
    rebuild.pool_reset(ctx)


# ------------------------------------------------------------------------------------------------ GPU: ties
@pytest.mark.gpu
def test_gpu_ties_from_seqs_give_the_reference_order(ctx):
    tie_rows = 0
    for case in load_json("rebuild_order.json.gz"):
        flat, ident, major, nodedup, seqs, halves = rebuild_case_pool(ctx, case)
        got = rebuild.rebuild_pool(ctx, ident, major, nodedup, keep_on_device=False, ties="seqs")
        cb = rebuild.tie_callback(seqs.__getitem__, halves.__getitem__)
        ref = rebuild.rebuild_pool(ctx, ident, major, nodedup, keep_on_device=False, tie_order=cb)
        assert got["n_ins_ties"] == 0 and ref["n_ins_ties"] == 0
        assert (got["n_tie_rows"], got["n_tie_dropped"]) == (ref["n_tie_rows"], ref["n_tie_dropped"]), case["name"]
        tie_rows += got["n_tie_rows"]
        order = {}
        for sr in got["src_row"].tolist():
            t, x = flat[sr]
            order.setdefault((t, x[-1]), []).append(tuple([int(x[0])] + list(x[1:])) if t in ("DEL", "INS", "DUP") else tuple(x))
        want = rebuild_expected(case)
        assert set(order) == set(want), case["name"]
        for k, rows in want.items():
            assert order[k] == rows, (case["name"], k)
    assert tie_rows > 0
    rebuild.pool_reset(ctx)


@pytest.mark.gpu
def test_gpu_ties_from_seqs_equal_the_callback_on_large_groups(ctx):
    rng = np.random.default_rng(11)
    seg, a, rd, seqs, halves = [], [], [], [], []
    stem = all_codes(300, 1).replace("=", "A")
    for g, size in enumerate((2, 3, 64, 65, 130)):
        for k in range(size):
            kind = k % 5
            s = (stem[:200] if kind == 0 else stem[:200] if kind == 1 else stem[:150] if kind == 2 else stem[:199] + "ACGT"[k % 4] if kind == 3
                 else stem[:200 - k % 7])
            seg.append(0); a.append(1000 * (g + 1)); rd.append(g); seqs.append(s); halves.append(int(rng.integers(0, 2)))
    n = len(seqs)
    perm = rng.permutation(n)                                    # (groups are found by the sort, not by adjacency in the pool)
    seg, a, rd = [seg[i] for i in perm], [a[i] for i in perm], [rd[i] for i in perm]
    seqs, halves = [seqs[i] for i in perm], [halves[i] for i in perm]
    # two groups with fixed half patterns over one sequence, their rows interleaved but each group's in this order (equal sequences
    # keep their input order): 0, 1, 0 drops nothing; 0, 0, 1 drops the second row
    for k in range(3):
        for g, pat in ((10, (0, 1, 0)), (11, (0, 0, 1))):
            seg.append(0); a.append(1000 * (g + 1)); rd.append(g); seqs.append(stem[:40]); halves.append(pat[k])
    n = len(seqs)
    seg, a, rd = np.asarray(seg), np.asarray(a), np.asarray(rd)
    rebuild.pool_reset(ctx)
    rebuild.pool_append(ctx, seg, a, np.full(n, 50), rd, [len(s) for s in seqs])
    rebuild.seq_pool_put(ctx, np.arange(n), seqs, halves)
    ident, one = np.arange(16, dtype=np.int32), np.ones(1, np.uint8)
    got = rebuild.rebuild_pool(ctx, ident, np.zeros(1, np.uint8), one, keep_on_device=False, ties="seqs")
    ref = rebuild.rebuild_pool(ctx, ident, np.zeros(1, np.uint8), one, keep_on_device=False, tie_order=rebuild.tie_callback(seqs.__getitem__, halves.__getitem__))
    for k in ("seg_id", "a", "b", "read_id", "aux", "src_row", "seg_count"):
        assert np.array_equal(got[k], ref[k]), k
    assert got["n_tie_rows"] == ref["n_tie_rows"] == n and got["n_tie_dropped"] == ref["n_tie_dropped"] > 0 and got["n_ins_ties"] == 0
    kept = {g: [halves[r] for r in got["src_row"].tolist() if rd[r] == g] for g in (10, 11)}
    assert kept == {10: [0, 1, 0], 11: [0, 1]}
    rebuild.pool_reset(ctx)


# ------------------------------------------------------------------------------------------------ GPU: misuse
@pytest.mark.gpu
def test_gpu_misuse_leaves_the_pools_and_the_context_usable(ctx):
    from cutesv_amd.engine import CsvError
    reads = [[(0, 20), (1, 15), (0, 20)], [(0, 30), (1, 12), (0, 500), (2, 40), (0, 30)]]
    seqs = [all_codes(55, 1), all_codes(572, 2)]
    off, flat = extract.encode_cigars(reads)
    start = np.asarray([100, 5000], np.int64)
    img, s_off, l_seq = pack4(seqs)
    pool = dict(seg_ins=0, seg_del=1, read_base=0, query_len=l_seq, seqs=True)

    def refused(fn, *a, **k):
        before = (rebuild.pool_rows(ctx), rebuild.seq_pool_rows(ctx))
        with pytest.raises(CsvError) as e:
            fn(*a, **k)
        assert e.value.code == _abi.E_INVALID, e.value
        assert (rebuild.pool_rows(ctx), rebuild.seq_pool_rows(ctx)) == before
    from cutesv_amd import engine
    with engine.Context(0) as fresh:                                           # the bit without an upload
        with pytest.raises(CsvError) as e:
            extract.cigar_signatures(fresh, off, flat, start, pool=pool)
        assert e.value.code == _abi.E_INVALID and rebuild.pool_rows(fresh) == 0 and rebuild.seq_pool_rows(fresh) == (0, 0)
        extract.upload_read_sequences(fresh, img, s_off, l_seq)
        assert extract.cigar_signatures(fresh, off, flat, start, pool=pool)["n_sig_ins"] == 2 and rebuild.seq_pool_rows(fresh) == (2, 27)
    rebuild.pool_reset(ctx)
    # ranges that leave the image: refused, and the previous upload stays
    extract.upload_read_sequences(ctx, img, s_off, l_seq)
    L = _lib.lib()
    for o, l in (([0, len(img)], [55, 2]), ([0, -1], [55, 2]), ([0, 28], [55, -3]), ([0, 28], [55, 2 * len(img)])):
        oo, ll = np.asarray(o, np.int64), np.asarray(l, np.int32)
        assert L.csv_seq_reads_upload(ctx._h, 2, img.ctypes.data, len(img), oo.ctypes.data, ll.ctypes.data, None) == _abi.E_INVALID, (o, l)
    extract.cigar_signatures(ctx, off, flat, start, pool=pool)
    assert rebuild.pool_rows(ctx) == 3 and rebuild.seq_pool_rows(ctx) == (2, 27)
    # a read left out by `want`
    extract.upload_read_sequences(ctx, img, s_off, l_seq, want=[1, 0])
    refused(extract.cigar_signatures, ctx, off, flat, start, pool=pool)
    # the bit without CSV_CG_TO_POOL
    cin = extract.CigarIn(n_reads=2, cig_off=off.ctypes.data, cigar=flat.ctypes.data, ref_start=start.ctypes.data, flags=_abi.CG_SEQ_TO_POOL, min_siglength=10)
    assert L.csv_cigar_signatures(ctx._h, C.byref(cin), C.byref(extract.CigarOut())) == _abi.E_INVALID
    sin = extract.SplitIn(n_reads=0, flags=_abi.CG_SEQ_TO_POOL)
    assert L.csv_split_signatures(ctx._h, C.byref(sin), C.byref(extract.SplitOut())) == _abi.E_INVALID
    # put: a wrong length, a row that has a sequence, a row out of range, a row named twice
    rebuild.pool_append(ctx, [0, 0], [7, 7], [9, 9], [1, 1], [4, 4])           # rows 3 and 4: INS rows made on the host
    refused(rebuild.seq_pool_put, ctx, [3], ["ACG"])
    refused(rebuild.seq_pool_put, ctx, [0], [rebuild.seq_pool_get(ctx, [0])[0]])
    refused(rebuild.seq_pool_put, ctx, [5], ["ACGT"])
    refused(rebuild.seq_pool_put, ctx, [3, 3], ["ACGT", "ACGT"])
    # get: a DEL row, a row out of range
    refused(rebuild.seq_pool_get, ctx, [2])
    refused(rebuild.seq_pool_get, ctx, [0, 9])
    # ties from sequences with a callback, and with a group row that has no sequence (rows 3 and 4 tie)
    ident, zero, one = np.arange(4, dtype=np.int32), np.zeros(2, np.uint8), np.asarray([1, 0], np.uint8)
    rin = rebuild.RebuildIn(n_seg=2, flags=_abi.RB_FROM_POOL | _abi.RB_TIES_FROM_SEQS, seg_aux_major=zero.ctypes.data, seg_nodedup=one.ctypes.data,
                            read_rank=ident.ctypes.data, n_rank=4, tie_order=C.cast(rebuild.tie_callback(lambda r: "", lambda r: 0), C.c_void_p))
    assert L.csv_rebuild_signatures(ctx._h, C.byref(rin), C.byref(rebuild.RebuildOut())) == _abi.E_INVALID
    rin = rebuild.RebuildIn(n=1, n_seg=2, flags=_abi.RB_TIES_FROM_SEQS, seg_aux_major=zero.ctypes.data, seg_nodedup=one.ctypes.data)
    assert L.csv_rebuild_signatures(ctx._h, C.byref(rin), C.byref(rebuild.RebuildOut())) == _abi.E_INVALID
    rebuild.seq_pool_put(ctx, [3], ["ACGT"], [1])
    refused(rebuild.rebuild_pool, ctx, ident, zero, one, keep_on_device=False, ties="seqs")
    # ... and the next correct calls work
    rebuild.seq_pool_put(ctx, [4], ["ACGT"], [1])
    r = rebuild.rebuild_pool(ctx, ident, zero, one, keep_on_device=False, ties="seqs")
    assert (r["n_tie_rows"], r["n_tie_dropped"], r["n_out"]) == (2, 1, 4)
    want = extract.pool_ins_sequences_host(seqs, None, _oracle().cigar_signatures(off, flat, start, None), None)
    assert rebuild.seq_pool_get(ctx, [0, 1, 3, 4], raw=True) == [b for b, _ in want] + [b"ACGT", b"ACGT"]
    assert rebuild.seq_pool_half(ctx, [0, 3, 2]).tolist() == [0, 1, 0]
    rebuild.pool_reset(ctx)


# ------------------------------------------------------------------------------------------------ GPU: device memory
def device_memory_free():
    """free bytes of the current device, asked of the HIP runtime the library itself is linked with"""
    hip = None
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = C.CDLL(name)
            break
        except OSError:
            continue
    assert hip is not None, "the HIP runtime library was not found"
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)


@pytest.mark.gpu
def test_gpu_a_seq_pool_task_holds_the_bases_the_blob_and_the_row_arrays(tmp_path):
    """What task_to_pool(seq_pool=True) holds beyond task_to_pool.  (1) By the library's own account (csv_seq_info.device_bytes, the
    capacities of every buffer of the sequence pool): the uploaded bases (packed image + 12 bytes per record), the blob, 9 bytes per
    row the pool has room for (it reserves rows + rows / 2 + 4096), and the scratch of one attach (16 bytes per new row plus its
    scan tables) - each buffer at most half again as large as asked plus 4 KiB (the growth rules of reserve / grow_keep), eleven
    buffers.  Neither the host image (names, qualities) nor a second copy of the blob fits under that.  (2) By the runtime's free
    memory, against a task without sequences in a context of its own: the accounted bytes rounded to the allocator's 2 MiB granule
    per buffer, plus 64 MiB for other processes on a shared card (test_bam_split.py allows 8 GiB for that)."""
    from cutesv_amd import engine
    case = load_json("single_pipe.json.gz")[0]
    p, (chrom, t0, t1) = case["params"], case["task"]
    rank = {c: i for i, c in enumerate(case["chroms"])}
    refs, recs = golden_records(case, chrom)
    path = str(tmp_path / "m.bam")
    bam_writer.write_bam(path, refs, recs)
    held = {}
    for seq_pool in (False, True):
        with engine.Context(0) as c2, bam.BamFile(path) as bf:
            ch = bf.records(chrom, t0, 1 << 40)
            bam.decode(c2, ch, host_outputs=False)                # (the context's first allocations are behind it)
            before = device_memory_free()
            res = extract.task_to_pool(c2, bf, chrom, t0, 1 << 40, rank, *pipe_args(p), 5, 0, [0, 5, 10, 15, 20], 0, seq_pool=seq_pool)
            held[seq_pool] = before - device_memory_free()
            if seq_pool:
                info, n_rows = extract.seq_info(c2), rebuild.pool_rows(c2)
            rebuild.pool_reset(c2)
    pool_room = n_rows + n_rows // 2 + 4096
    asked = info["bytes_uploaded"] + res["n_seq_bytes"] + 9 * pool_room + 16 * (n_rows + 1) + 24 * (n_rows // 1024 + 1) + 1024
    print("accounted %d, asked %d, uploaded %d, blob %d, pool rows %d, host image %d, held %s" % (info["device_bytes"], asked, info["bytes_uploaded"], res["n_seq_bytes"],
                                                                                                 n_rows, len(ch.host), held))
    assert res["n_seq_rows"] > 40 and info["packed"] == 1 and info["bytes_uploaded"] < len(ch.host)
    assert 0 < info["device_bytes"] <= asked + asked // 2 + 11 * 4096, (info, asked)
    assert held[True] - held[False] <= info["device_bytes"] + 11 * (2 << 20) + (64 << 20), (held, info)
