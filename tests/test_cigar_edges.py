"""The per-read CIGAR scan (cigar.hip.h) at its thresholds and at the seams of its 64-operation step.

tests/golden/cigar_edges.json.gz holds what the reference's parse_read made of crafted reads - one family per rule, one quantity
moved across the rule's threshold (tests/cigar_helpers.py places the pieces, tests/golden/make_golden_cigar.py records) - and of
3 x 3 000 dense random reads (recorded as digests: the seed of the reads, a digest of the two lists and one per read).  The
oracle, extract.candidates and the host glue are compared with it on the CPU, the kernel on the GPU; a lane sweep moves every
merge family across all 64 lanes and two step boundaries and ties the result to the recorded one."""
import hashlib
import json

import numpy as np
import pytest

from cutesv_amd import bam, extract, rebuild, synth
from cutesv_amd.columns import TYPES
from helpers import load_json, cigar_case_inputs, assert_cigar_case, StubRecord
import bam_writer
import cigar_helpers as ch

_CACHE = {}


def _oracle():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def cases():
    if "cases" not in _CACHE:
        _CACHE["cases"] = [ch.expand_case(c) for c in load_json("cigar_edges.json.gz")]
    return _CACHE["cases"]


def crafted():
    return [c for c in cases() if "dense" not in c]


def assert_case(case, scan):
    """the scan's arrays -> candidate lists == what the reference recorded (a dense case: its digests); -> the arrays"""
    if "dense" not in case:
        return assert_cigar_case(case, scan)
    off, flat, start, use, names, seqs, kw = cigar_case_inputs(case)
    sig = scan(off, flat, start, use, **kw)
    ins, dele = extract.candidates(sig, names, seqs, "chr7")
    ins, dele = [list(x) for x in ins], [list(x) for x in dele]
    assert (len(ins), len(dele)) == (case["n_ins"], case["n_del"]), case["name"]
    mine, theirs = ch.per_read_digests(case["reads"], ins, dele), case["per_read"]
    bad = [case["reads"][k]["name"] for k in range(len(case["reads"])) if mine[8 * k:8 * k + 8] != theirs[8 * k:8 * k + 8]]
    assert not bad, (case["name"], len(bad), bad[:5])
    sha = lambda rows: hashlib.sha256(json.dumps(rows, separators=(",", ":")).encode()).hexdigest()      # noqa: E731
    assert sha(ins) == case["sha_ins"] and sha(dele) == case["sha_del"], case["name"]
    return sig


def sweep_bases(case):
    """the reads of the merge and seam families (a leading H cannot take a prefix: it would stop being the first operation)"""
    return [r for r in case["reads"] if ch.kind_of(r["family"]) in ch.MERGE_FAMILIES and r["cigar"][0][0] != ch.H]


def sweep_inputs(case):
    key = "sweep_" + case["name"]
    if key not in _CACHE:
        base = sweep_bases(case)
        _CACHE[key] = (base,) + ch.sweep_batch(base)
    return _CACHE[key]


def sweep_expected(case):
    """what the sweep batch of `case` must give, for the oracle and for the kernel alike: the oracle's arrays of the UNPREFIXED reads -
    checked here to be the rows the reference recorded for those reads - repeated per k with positions and piece offsets + k"""
    key = "sweep_want_" + case["name"]
    if key not in _CACHE:
        base, off, flat, start, which, kk = sweep_inputs(case)
        b_off, b_flat, b_start = ch.batch_arrays(base)
        plain = _oracle().cigar_signatures(b_off, b_flat, b_start, None, **scan_kw(case))
        names = {r["name"] for r in base}
        ins, dele = extract.candidates(plain, [r["name"] for r in base], [synth.pseudo_sequence(r["seq_len"], r["seq_key"]) for r in base], "chr7")
        assert [list(x) for x in ins] == [x for x in case["INS"] if x[2] in names] and [list(x) for x in dele] == [x for x in case["DEL"] if x[2] in names]
        _CACHE[key] = ch.shifted(ch.tile_sig(plain, which, len(base)), len(which), kk)
    return _CACHE[key]


def scan_kw(case):
    p = case["params"]
    return dict(min_siglength=p["min_siglength"], merge_ins_threshold=p["mi"], merge_del_threshold=p["md"])


# ------------------------------------------------------------------------------------------------ CPU
def test_oracle_and_candidates_equal_the_reference_on_every_case():
    n = 0
    for case in cases():
        sig = assert_case(case, _oracle().cigar_signatures)
        n += len(sig["ins_read"]) + len(sig["del_read"])
    assert len(cases()) == 9 and n > 100000


def test_parse_reads_equals_the_host_families():
    """the gates that are the caller's: mapq and query length at their thresholds, every flag class"""
    o = _oracle()
    seen = 0
    for case in crafted():
        p = case["params"]
        if not case["name"].startswith("host_"):
            continue
        cand = extract.parse_reads([StubRecord(dict(d, tags=[])) for d in case["reads"]], "chr7", {"chr7": 0}, 30, p["min_mapq"], 7, p["min_read_len"],
                                   p["min_siglength"], p["md"], p["mi"], 100000, o.cigar_signatures, o.split_signatures)
        assert [list(x) for x in cand["INS"]] == case["INS"] and [list(x) for x in cand["DEL"]] == case["DEL"], case["name"]
        assert not cand["DUP"] and not cand["INV"] and not cand["TRA"]
        by = {}
        for x in case["INS"]:
            by[x[2]] = by.get(x[2], 0) + 1
        name = lambda fam, step: "%s/%s/%s" % (case["name"][5:], fam, step)       # noqa: E731
        assert name("host_mapq", p["min_mapq"] - 1) not in by and by[name("host_mapq", p["min_mapq"])] == 1
        assert name("host_qlen", p["min_read_len"] - 1) not in by and by[name("host_qlen", p["min_read_len"])] == 1
        assert all(by[name("host_flag", f)] == 1 for f in (0, 16, 256, 2048, 2064))
        seen += 1
    assert seen == len(ch.PARAM_SETS)


def test_pool_ins_sequences_host_equals_the_recorded_strings():
    n_cut = n_empty = n_multi = 0
    for case in crafted():
        off, flat, start, use, names, seqs, kw = cigar_case_inputs(case)
        sig = _oracle().cigar_signatures(off, flat, start, use, **kw)
        got = extract.pool_ins_sequences_host(seqs, None, sig, None)
        assert [b.decode() for b, _ in got] == [x[3] for x in case["INS"]], case["name"]
        assert all(h == 0 for _, h in got)
        n_cut += sum(0 < len(x[3]) < x[1] for x in case["INS"]); n_empty += sum(x[3] == "" for x in case["INS"])
        n_multi += int((sig["ins_npiece"] > 1).sum())
    assert n_cut >= 6 and n_empty >= 6 and n_multi >= 30, (n_cut, n_empty, n_multi)


def test_fixture_covers_every_family_and_every_decision():
    # every family of every parameter set is there and shows, in the recorded rows, what it is there to show (names and bases left out)
    for c in crafted():
        expect = ch.expectations(ch.PARAM_SETS[c["name"].split("_", 1)[1]]) if c["name"].startswith("edges_") else ch.HOST_EXPECTATIONS
        ch.check_families(c["reads"], ch.rows_per_read(c["reads"], c["INS"], c["DEL"]), expect)
    with pytest.raises(AssertionError, match="does not change"):            # the check can fail: host_flag decides nothing
        c = crafted()[1]
        ch.check_families(c["reads"], ch.rows_per_read(c["reads"], c["INS"], c["DEL"]), dict(ch.HOST_EXPECTATIONS, host_flag="change"))
    present = {(ch.kind_of(r["family"]), c["name"].split("_", 1)[1]) for c in crafted() for r in c["reads"]}
    for kind in ch.FAMILY_KINDS + ("host",):
        for s in ch.PARAM_SETS:
            assert (kind, s) in present, (kind, s)
    for c in crafted():
        # the generator's own reads, regenerated: the fixture holds exactly these
        s = c["name"].split("_", 1)[1]
        k = list(ch.PARAM_SETS).index(s)
        make = ch.families(s, ch.PARAM_SETS[s], 7000000 + 10000 * k) if c["name"].startswith("edges_") else ch.host_family(s, ch.PARAM_SETS[s], 7500000 + 10000 * k)
        assert make == [{k: v for k, v in r.items() if k != "seq"} for r in c["reads"]], c["name"]       # (cigar_case_inputs adds "seq")
        print(c["name"], len(c["reads"]), "reads;", ch.counters(c["reads"], c["params"]))
    gaps = {r["family"] for c in crafted() for r in c["reads"] if r["family"].startswith("ins_gap_")}
    assert gaps == {"ins_gap_" + k for k in ch.GAP_KINDS}
    # the seam families put the deciding pair where they say: both pieces at the operation indices of the step name
    n_seam = 0
    for c in crafted():
        ms = c["params"]["min_siglength"]
        for r in c["reads"]:
            if r["family"].startswith("seam_") and "_at" in r["step"]:
                a, b = (int(x) for x in r["step"].split("_at")[1].split("_"))
                pieces = [k for k, (op, ln) in enumerate(r["cigar"]) if op in (ch.I, ch.D) and ln >= ms]
                assert pieces[-2:] == [a, b], r["name"]
                n_seam += 1
            elif r["family"].startswith("seam_adjacent"):
                a, b = (int(x) for x in r["step"].split("_"))
                pieces = [k for k, (op, ln) in enumerate(r["cigar"]) if op in (ch.I, ch.D) and ln >= ms]
                assert pieces[-2:] == [a, b] and b == a + 1, r["name"]
                n_seam += 1
            elif r["family"].startswith("seam_empty_step"):
                pieces = [k for k, (op, ln) in enumerate(r["cigar"]) if op in (ch.I, ch.D) and ln >= ms]
                assert pieces[-1] - pieces[-2] > 100 and pieces[-2] < 64 and pieces[-1] >= 64 + 40, r["name"]
                n_seam += 1
    assert n_seam > 150
    for c in cases():
        if "dense" in c:
            cnt = ch.counters(c["reads"], c["params"])
            print(c["name"], cnt)
            assert cnt == c["counters"] and all(v >= 100 for v in cnt.values()), (c["name"], cnt)
            assert sorted({len(r["cigar"]) for r in c["reads"]}) == sorted(ch.DENSE_COUNTS)


def test_lane_sweep_oracle_equals_the_recorded_output_shifted():
    """k = 0..130 single-base M operations in front of every merge and seam family: each piece visits every lane and crosses two
    step boundaries.  The output must be the unprefixed one - which the reference recorded - with positions and piece offsets + k."""
    n = 0
    for case in crafted():
        if not case["name"].startswith("edges_"):
            continue
        base, off, flat, start, which, kk = sweep_inputs(case)
        assert len(base) >= 60
        got = _oracle().cigar_signatures(off, flat, start, None, **scan_kw(case))
        ch.assert_sig_equal(got, sweep_expected(case), case["name"])
        n += len(which)
    assert n > 3 * 60 * 131


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_gpu_every_case_equals_the_reference_and_the_oracle(ctx):
    for case in cases():
        got = assert_case(case, lambda *a, **k: extract.cigar_signatures(ctx, *a, **k))
        off, flat, start, use, _, _, kw = cigar_case_inputs(case)
        ch.assert_sig_equal(got, _oracle().cigar_signatures(off, flat, start, use, **kw), case["name"])


@pytest.mark.gpu
def test_gpu_lane_sweep_equals_the_oracle(ctx):
    for case in crafted():
        if not case["name"].startswith("edges_"):
            continue
        base, off, flat, start, which, kk = sweep_inputs(case)
        got = extract.cigar_signatures(ctx, off, flat, start, None, **scan_kw(case))
        ch.assert_sig_equal(got, sweep_expected(case), case["name"])
        assert len(got["ins_read"]) > 1000 and len(got["del_read"]) > 1000


DENSE_GPU_SETS = tuple((d["min_siglength"], d["mi"], d["md"]) for d in ch.DENSE_SETS) + ((1, 0, 0), (3, 8, 0))


def dense_gpu_batch():
    if "dense_gpu" not in _CACHE:
        reads = ch.dense_reads(8200, 20000) + ch.long_reads(8201)
        _CACHE["dense_gpu"] = ch.batch_arrays(reads) + (np.diff(ch.batch_arrays(reads)[0]),)
    return _CACHE["dense_gpu"]


@pytest.mark.gpu
@pytest.mark.parametrize("ms,mi,md", DENSE_GPU_SETS)
def test_gpu_dense_batch_equals_the_oracle(ctx, ms, mi, md):
    off, flat, start, n_ops = dense_gpu_batch()
    assert {4095, 4096, 4097, 8193} <= set(n_ops.tolist()) and len(start) == 20004
    kw = dict(min_siglength=ms, merge_ins_threshold=mi, merge_del_threshold=md)
    got = extract.cigar_signatures(ctx, off, flat, start, None, **kw)
    want = _oracle().cigar_signatures(off, flat, start, None, **kw)
    ch.assert_sig_equal(got, want, str((ms, mi, md)))
    assert len(got["ins_read"]) > 50000 and len(got["del_read"]) > 50000 and int(got["ins_npiece"].max()) > 3


def pipe_args(p):
    return (30, p["min_mapq"], 7, p["min_read_len"], p["min_siglength"], p["md"], p["mi"], 100000)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(ch.PARAM_SETS)))
def test_gpu_families_as_bam_records_three_routes(ctx, tmp_path, which):
    """the crafted reads written as BAM records: decode + scan on the device columns, single_pipe_bam, task_to_pool(seq_pool=True)"""
    from test_ins_seq_pool import pool_columns, segments_of
    case = [c for c in crafted() if c["name"].startswith("edges_")][which]
    p = case["params"]
    seqs = [synth.pseudo_sequence(r["seq_len"], r["seq_key"]) for r in case["reads"]]
    recs = [dict(name=r["name"], flag=r["flag"], mapq=r["mapq"], start=r["start"], cigar=r["cigar"], seq=s, refid=0, tags=[]) for r, s in zip(case["reads"], seqs)]
    path = str(tmp_path / "fam.bam")
    bam_writer.write_bam(path, [("chr7", 159345973)], recs)
    rank = {"chr7": 0}
    seg_of, seg_base = segments_of(1)
    assert any(len(x[3]) < x[1] for x in case["INS"]) and any(x[1] > 2 * p["min_siglength"] + 4 for x in case["INS"])
    with bam.BamFile(path) as bf:
        (chunk,) = list(bf.chunks("chr7"))
        # route 1: the decode's columns, scanned where they are
        cols = bam.decode(ctx, chunk)
        use = ((cols["mapq"] >= p["min_mapq"]) & (cols["query_len"] >= p["min_read_len"])).astype(np.uint8)
        sig = extract.cigar_signatures(ctx, None, None, None, use, from_bam=cols, **scan_kw(case))
        ins, dele = extract.candidates(sig, [r["name"] for r in recs], seqs, "chr7")
        assert [list(x) for x in ins] == case["INS"] and [list(x) for x in dele] == case["DEL"]
        # route 2
        cand, _ = extract.single_pipe_bam(ctx, bf, "chr7", 0, 1 << 40, rank, *pipe_args(p))
        assert [list(x) for x in cand["INS"]] == case["INS"] and [list(x) for x in cand["DEL"]] == case["DEL"]
        assert not cand["DUP"] and not cand["INV"] and not cand["TRA"]
        # route 3
        rebuild.pool_reset(ctx)
        res = extract.task_to_pool(ctx, bf, "chr7", 0, 1 << 40, rank, *pipe_args(p), seg_of("INS", 0), seg_of("DEL", 0), seg_base, 0, seq_pool=True)
        rows = pool_columns(ctx, len(TYPES))
    n_ins, n_del = len(case["INS"]), len(case["DEL"])
    assert res["n_sig_ins"] == n_ins and res["n_sig_del"] == n_del and rebuild.pool_rows(ctx) == n_ins + n_del
    names = [r["name"] for r in recs]
    assert rows["seg_id"].tolist() == [seg_of("INS", 0)] * n_ins + [seg_of("DEL", 0)] * n_del
    assert [[int(a), int(b), names[r]] for a, b, r in zip(rows["a"][:n_ins], rows["b"][:n_ins], rows["read_id"][:n_ins])] == [x[:3] for x in case["INS"]]
    assert [[int(a), int(b), names[r]] for a, b, r in zip(rows["a"][n_ins:], rows["b"][n_ins:], rows["read_id"][n_ins:])] == [x[:3] for x in case["DEL"]]
    assert rows["aux"][:n_ins].tolist() == [len(x[3]) for x in case["INS"]]
    assert rebuild.seq_pool_get(ctx, np.arange(n_ins)) == [x[3] for x in case["INS"]]
    rebuild.pool_reset(ctx)
