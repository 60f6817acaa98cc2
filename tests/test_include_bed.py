"""--include_bed end to end (cutesv_amd/bed.py) and the task gates on the device (csv_bam_task_gates,
cutesv_amd/csrc/gates.hip.h).

CPU: bed.load_bed / Regions.for_task against the reference's recorded load_bed answers (include_bed.json.gz), parse errors,
single_pipe_bam over three tasks against the reference's recorded single_pipe with its per-task lists, the numpy twin
gate_bits_host against _gates, the interface.  GPU: the kernel against the twin on crafted and random records and region tables,
the consumers (use / sel read from the gates column) against the host-gated path and the reference, every refusal, and call_bam
with a BED against the BED-aware route through the store."""
import os
import re

import numpy as np
import pytest

from cutesv_amd import _abi, _lib, bam, bed, call, extract, rebuild
from cutesv_amd.columns import Params
from helpers import load_json
import bam_writer
import bed_helpers as bh
import call_helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES5 = ("DEL", "INS", "DUP", "INV", "TRA")


def _oracle():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    return load_json("include_bed.json.gz")


def _write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return str(path)


# ------------------------------------------------------------------------------------------------ CPU: bed.py
def test_load_bed_and_for_task_reproduce_the_reference(golden, tmp_path):
    cases = golden["load_bed"] + [golden["multi_task"]]
    assert {c["name"] for c in cases} == {"edges", "seam", "one_task", "random", "multi_task"}
    n_regions = 0
    for case in cases:
        regions = bed.load_bed(_write(tmp_path / (case["name"] + ".bed"), case["bed"]))
        for (chrom, t0, t1), want in zip(case["tasks"], case["regions"]):
            got = regions.for_task(chrom, t0, t1)
            assert got.dtype == np.int64 and got.shape == (len(want), 2), (case["name"], chrom, t0)
            assert got.tolist() == want, (case["name"], chrom, t0)
            n_regions += len(want)
    assert n_regions > 40
    edges = {c["name"]: c for c in cases}["edges"]
    by_task = {(c, t0): r for (c, t0, _), r in zip(edges["tasks"], edges["regions"])}
    assert [20000, 23000] not in by_task[("c1", 10000)] and [20000, 23000] in by_task[("c1", 20000)]      # a padded start on a task's end
    assert all([7500, 22500] in by_task[("c1", t0)] for t0 in (0, 10000, 20000))                         # across two boundaries
    assert by_task[("c1", 0)][0] == [-500, 1700] and by_task[("c2", 0)] == [] and by_task[("c2", 10000)] == []
    seam = {c["name"]: c for c in cases}["seam"]
    assert seam["regions"] == [[], [[4000, 7000]]]                                                     # the cut matters


def test_for_task_answers_an_absent_chromosome_with_an_empty_array_and_from_intervals_pads():
    r = bed.Regions.from_intervals({"c1": [(5000, 6000), (100, 200), (5000, 5500)]})
    assert r.by_chrom["c1"].tolist() == [[-900, 1200], [4000, 6500], [4000, 7000]] and len(r) == 3
    none = r.for_task("other", 0, 1000)
    assert none is not None and none.shape == (0, 2) and none.dtype == np.int64
    assert bed.Regions.from_intervals({"c1": [(10, 20)]}, pad=0).for_task("c1", 0, 100).tolist() == [[10, 20]]
    assert bed.Regions.from_intervals({}).for_task("c1", 0, 100).shape == (0, 2)


def test_load_bed_skips_comments_and_names_file_and_line_of_a_bad_one(tmp_path):
    path = _write(tmp_path / "a.bed", "# comment\ntrack name=x\nbrowser position c1:1-2\n\nc1\t5000\t6000\textra\tfields\n   \nc1\t100\t200\n")
    assert bed.load_bed(path).by_chrom["c1"].tolist() == [[-900, 1200], [4000, 7000]]
    assert bed.load_bed(path, pad=0).by_chrom["c1"].tolist() == [[100, 200], [5000, 6000]]
    assert len(bed.load_bed(_write(tmp_path / "empty.bed", ""))) == 0
    for text, line in (("c1\t1\t2\nc1\t5\n", 2), ("c1 1 2\n", 1), ("#x\nc1\t1\t2\nc1\tone\t2\n", 3), ("c1\t1\t2.5\n", 1)):
        path = _write(tmp_path / "bad.bed", text)
        with pytest.raises(ValueError, match=re.escape("%s:%d:" % (path, line))):
            bed.load_bed(path)


def _multi_task_bam(golden, tmp_path):
    case = golden["multi_task"]
    refs, recs = bh.golden_records(case, case["chrom"], {case["chrom"]: case["contig_len"]})
    path = str(tmp_path / "multi_task.bam")
    bam_writer.write_bam(path, refs, recs)
    return case, path, {c: i for i, c in enumerate(case["chroms"])}


def _assert_multi_task(case, path, rank, fns, **kw):
    regions = bed.load_bed(_write(os.path.join(os.path.dirname(path), "multi_task.bed"), case["bed"]))
    n_rows = 0
    with bam.BamFile(path) as bf:
        for (chrom, t0, t1), want in zip(case["tasks"], case["out"]):
            cand, reads_info = extract.single_pipe_bam(fns, bf, chrom, t0, t1, rank, *bh.pipe_args(case["params"]), bed_regions=regions.for_task(chrom, t0, t1), **kw)
            for t in TYPES5:
                assert [list(x) for x in cand[t]] == want[t], (t0, t)
            assert [list(x) for x in reads_info] == want["reads_table"], t0
            n_rows += len(reads_info)
    assert n_rows >= 30


def test_single_pipe_bam_over_three_tasks_equals_the_reference(golden, tmp_path):
    """the CPU path (decode_host and the oracle's scans) with for_task lists == the reference's single_pipe with its load_bed lists"""
    case, path, rank = _multi_task_bam(golden, tmp_path)
    o = _oracle()
    _assert_multi_task(case, path, rank, (o.cigar_signatures, o.split_signatures))
    # the fixture shows the rule: planted reads the reference dropped would pass against the chromosome's full list
    assert len(case["dropped"]) >= 3
    in_table = {row[3] for out in case["out"] for row in out["reads_table"]}
    assert not in_table & set(case["dropped"])
    with bam.BamFile(path) as bf:
        chrom, t0, t1 = case["tasks"][0]
        _, full = extract.single_pipe_bam((o.cigar_signatures, o.split_signatures), bf, chrom, t0, t1, rank, *bh.pipe_args(case["params"]), bed_regions=case["full"])
    assert {r[3] for r in full} & set(case["dropped"])
    with pytest.raises(ValueError):
        with bam.BamFile(path) as bf:
            extract.single_pipe_bam((o.cigar_signatures, o.split_signatures), bf, chrom, t0, t1, rank, *bh.pipe_args(case["params"]), gates="device")


def test_gate_bits_host_is_gates_bit_for_bit(tmp_path):
    n = 0
    for case in load_json("single_pipe.json.gz"):
        chrom, t0, _ = case["task"]
        refs, recs = bh.golden_records(case, chrom)
        path = str(tmp_path / (case["name"] + ".bam"))
        bam_writer.write_bam(path, refs, recs)
        p = case["params"]
        with bam.BamFile(path) as bf:
            cols = bam.decode_host(bf.records(chrom, 0, 1 << 40))
        for regions in (case["bed"], None, []):
            gate, parsed, use, sel = extract._gates(cols, t0, regions, p["min_read_len"], p["min_mapq"])
            bits = extract.gate_bits_host(cols, t0, regions, p["min_read_len"], p["min_mapq"])
            assert bits.dtype == np.uint8 and len(bits) == len(gate)
            for mask, want in ((_abi.GATE_TASK, gate), (_abi.GATE_PARSED, parsed), (_abi.GATE_USE, use != 0), (_abi.GATE_SEL, sel),
                               (_abi.GATE_READS, gate & (cols["mapq"] >= p["min_mapq"]))):
                assert np.array_equal((bits & mask) != 0, want), (case["name"], mask)
            assert not (bits & ~np.uint8(31)).any()
            n += int(gate.sum())
            if regions == []:
                assert not bits.any()
    assert n > 300


def test_header_declares_and_lib_binds_the_gates_entry():
    with open(os.path.join(ROOT, "include", "cutesv_hip.h")) as f:
        header = f.read()
    assert re.search(r"^int csv_bam_task_gates\(csv_ctx\* ctx, int64_t n_records, int64_t task_start, int32_t min_read_len, int32_t min_mapq, int32_t flags,", header, re.M)
    assert re.search(r"CSV_CG_USE_FROM_GATES = 16\b", header) and re.search(r"CSV_SA_SEL_FROM_GATES = 1\b", header) and re.search(r"CSV_GT_BED = 1\b", header)
    assert re.search(r"CSV_GATE_TASK = 1, CSV_GATE_PARSED = 2, CSV_GATE_USE = 4, CSV_GATE_SEL = 8, CSV_GATE_READS = 16", header)
    assert "csv_bam_task_gates" in {n for n, _, _ in _lib.SYMBOLS}
    assert (_abi.CG_USE_FROM_GATES, _abi.SA_SEL_FROM_GATES, _abi.GT_BED) == (16, 1, 1)
    assert (_abi.GATE_TASK, _abi.GATE_PARSED, _abi.GATE_USE, _abi.GATE_SEL, _abi.GATE_READS) == (1, 2, 4, 8, 16)
    L = _lib.lib()
    assert L.csv_abi_version() == _abi.ABI_VERSION == 9
    assert bh.raw_task_gates(None, 0, 0, 0, 0, 0, 0, None, None) == _abi.E_INVALID


def test_the_command_line_takes_both_spellings(monkeypatch, tmp_path):
    seen = []
    monkeypatch.setattr(call, "call_bam", lambda *a, **k: (seen.append(k["include_bed"]), (b"", np.zeros(5, np.int64)))[1])
    from cutesv_amd import fasta
    monkeypatch.setattr(fasta, "Reference", lambda path: path)
    out = str(tmp_path / "o.vcf")
    for spelling in ("--include_bed", "-include_bed"):
        assert call.main(["a.bam", "ref.fa", "-o", out, spelling, "panel.bed"]) == 0
    assert call.main(["a.bam", "ref.fa", "-o", out]) == 0
    assert seen == ["panel.bed", "panel.bed", None]


# ------------------------------------------------------------------------------------------------ GPU: the kernel against the twin
def _decode(ctx, tmp_path, n, seed=11):
    path = str(tmp_path / ("gates%d_%d.bam" % (n, seed)))
    bam_writer.write_bam(path, bh.GATE_REFS, bh.gate_records(n, seed))
    with bam.BamFile(path) as bf:
        chunk = bf.records("7", 0, 1 << 40)
    assert chunk.n == n
    return chunk, bam.decode(ctx, chunk, host_outputs=False)


@pytest.mark.gpu
@pytest.mark.parametrize("n", bh.CHUNK_SIZES)
def test_gpu_task_gates_equal_the_twin(ctx, tmp_path, n):
    chunk, cols = _decode(ctx, tmp_path, n)
    seen = 0
    for name, regions in bh.region_tables():
        for t0, min_len, min_mapq in ((bh.T0, bh.MIN_LEN, bh.MIN_MAPQ), (0, 0, 0), (bh.B1, bh.MIN_LEN + 1, 61)):
            want = extract.gate_bits_host(cols, t0, regions, min_len, min_mapq)
            got = extract.task_gates(ctx, n, t0, min_len, min_mapq, regions)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (name, t0, np.flatnonzero(got != want)[:5].tolist())
            seen |= int(np.bitwise_or.reduce(want)) if n else 0
        if name == "empty":
            assert not got.any()
    if n >= 64:
        assert seen == 31
    if n >= 65:                                               # the crafted records sit where they were meant to
        names = [chunk.name(i) for i in range(n)]
        bits = dict(zip(names, extract.task_gates(ctx, n, bh.T0, bh.MIN_LEN, bh.MIN_MAPQ, [(bh.B0, bh.B1), (bh.B1, bh.B1 + 1000), (40000, 60000), (41000, 42000)]).tolist()))
        assert bits["end_at_b0"] == 0 and bits["end_b0_plus1"] == 31 and bits["start_b1_minus1"] == 1 | 2 | 4 | 16 and bits["inside"] == 31
        assert bits["start_at_b1"] != 0                       # (the second region begins there)
        assert bits["seam_zero"] == 0 and bits["seam_zero_sa"] == 0 and bits["zero_inside"] != 0 and bits["behind_short"] == 31 and bits["far"] == 0
        plain = dict(zip(names, extract.task_gates(ctx, n, bh.T0, bh.MIN_LEN, bh.MIN_MAPQ).tolist()))
        assert plain["t_below"] == 0 and plain["t_at"] == 1 | 2 | 4 | 16 and plain["len_below"] == 1 | 16 and plain["len_at"] == 1 | 2 | 4 | 16
        assert plain["mq_below"] == 1 | 2 | 8 and plain["mq_at"] == 31 and plain["short_lowmq"] == 1 and plain["seam_zero"] != 0
        assert [plain["cls%02d" % k] for k in range(10)] == [0, 0, 23, 31, 23, 31, 23, 23, 23, 23]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", (1, 2, 3))
def test_gpu_task_gates_random(ctx, tmp_path, seed):
    rng = np.random.default_rng(100 + seed)
    n = 2000
    _, cols = _decode(ctx, tmp_path, n, seed=seed)
    seen = 0
    for k in range(6):
        regions = bh.random_regions(rng, int(rng.choice([1, 2, 7, 64, 300])))
        t0, min_len, min_mapq = int(rng.integers(0, 60000)), int(rng.integers(0, 2500)), int(rng.choice([0, 20, 21]))
        want = extract.gate_bits_host(cols, t0, regions, min_len, min_mapq)
        got = extract.task_gates(ctx, n, t0, min_len, min_mapq, regions[rng.permutation(len(regions))] if k == 5 else regions)
        assert np.array_equal(got, want), (seed, k)
        seen |= int(np.bitwise_or.reduce(want))
    assert seen == 31                                         # (a single table may pass nothing; the six together set every bit)


# ------------------------------------------------------------------------------------------------ GPU: the consumers
def _consumer_cases(golden):
    """(case, chrom, [(t0, t1, regions of the task, recorded output or None)])"""
    out = []
    for case in load_json("single_pipe.json.gz"):
        chrom, t0, t1 = case["task"]
        far = max(t1, max(d["start"] for d in case["reads"]) + 1)        # (as test_bam_reader._single_pipe_bam_case: the recorded fetch ignored the end)
        out.append((case, chrom, None, [(t0, far, case["bed"], case)]))
    mt = golden["multi_task"]
    out.append((mt, mt["chrom"], {mt["chrom"]: mt["contig_len"]}, [(t0, t1, r, o) for (_, t0, t1), r, o in zip(mt["tasks"], mt["regions"], mt["out"])]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(3))
def test_gpu_consumers_read_the_gates_in_place(ctx, golden, tmp_path, which):
    case, chrom, lengths, tasks = _consumer_cases(golden)[which]
    refs, recs = bh.golden_records(case, chrom, lengths)
    path = str(tmp_path / "case.bam")
    bam_writer.write_bam(path, refs, recs)
    rank = {c: i for i, c in enumerate(case["chroms"])}
    n_chrom = len(rank)
    seg_base = [k * n_chrom for k in range(5)]
    seg_ins, seg_del = 5 * n_chrom, 5 * n_chrom + 1
    ins_segs = [seg_ins] + list(range(seg_base[1], seg_base[1] + n_chrom))
    args = bh.pipe_args(case["params"])
    n_rows = 0
    with bam.BamFile(path) as bf:
        for t0, t1, regions, want in tasks:
            # single_pipe_bam: device gates == the reference's recorded output
            cand, reads_info = extract.single_pipe_bam(ctx, bf, chrom, t0, t1, rank, *args, bed_regions=regions, sa="device", gates="device")
            for t in TYPES5:
                assert [list(x) for x in cand[t]] == want[t], (case["name"], t0, t)
            assert [list(x) for x in reads_info] == want["reads_table"], (case["name"], t0)
            host = extract.single_pipe_bam(ctx, bf, chrom, t0, t1, rank, *args, bed_regions=regions, sa="host", gates="device")
            assert host[0] == cand and host[1] == reads_info
            # task_to_pool: the same pool rows, sequence-pool rows and reads rows as with host gates
            images = {}
            for gates in ("host", "device"):
                rebuild.pool_reset(ctx)
                res = extract.task_to_pool(ctx, bf, chrom, t0, t1, rank, *args, seg_ins, seg_del, seg_base, 0, bed_regions=regions, seq_pool=True, gates=gates)
                img = bh.pool_image(ctx, 5 * n_chrom + 2, res["n_records"], ins_segs)
                img.update({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in res.items()})
                images[gates] = img
            assert images["host"].keys() == images["device"].keys()
            for k in images["host"]:
                assert images["host"][k] == images["device"][k], (case["name"], t0, k)
            assert len(images["device"]["reads_index"]) == len(want["reads_table"])
            n_rows += images["device"]["n"]
    assert n_rows > 20
    rebuild.pool_reset(ctx)


# ------------------------------------------------------------------------------------------------ GPU: refusals
@pytest.mark.gpu
def test_gpu_refusals_leave_the_context_usable(tmp_path):
    from cutesv_amd import engine
    L = _lib.lib()
    beg, end = np.array([10, 20, 30], np.int64), np.array([15, 25, 35], np.int64)
    with engine.Context(0) as c:
        n = 65
        assert bh.raw_task_gates(c, n, 0, 0, 0, 0, 0, None, None) == _abi.E_INVALID                    # no decode in the context
        cin, cout = bh.cigar_in_out(n, _abi.CG_FROM_BAM | _abi.CG_USE_FROM_GATES)
        assert L.csv_cigar_signatures(c._h, bh.byref(cin), bh.byref(cout)) == _abi.E_INVALID
        chunk, cols = _decode(c, tmp_path, n)
        want = extract.gate_bits_host(cols, bh.T0, [(bh.B0, bh.B1)], bh.MIN_LEN, bh.MIN_MAPQ)
        assert want.any()

        def works():
            assert np.array_equal(extract.task_gates(c, n, bh.T0, bh.MIN_LEN, bh.MIN_MAPQ, [(bh.B0, bh.B1)]), want)
        # the flags before any gates exist
        assert L.csv_cigar_signatures(c._h, bh.byref(cin), bh.byref(cout)) == _abi.E_INVALID
        sin, sout, _keep = bh.sa_in_out(n, _abi.SA_SEL_FROM_GATES)
        assert L.csv_bam_split_inputs(c._h, bh.byref(sin), bh.byref(sout)) == _abi.E_INVALID
        works()
        bad = [(n + 1, 0, 0, None, None),                                    # n_records is not the decode's
               (n, _abi.GT_BED, -1, beg, end),                              # n_regions < 0
               (n, 0, 3, beg, end),                                         # regions without CSV_GT_BED
               (n, _abi.GT_BED, 3, None, end), (n, _abi.GT_BED, 3, beg, None),      # CSV_GT_BED with regions and a NULL array
               (n, _abi.GT_BED, 3, beg[::-1].copy(), end),                   # region_beg decreasing
               (n, 2, 0, None, None)]                                       # an unknown flag
        for nn, flags, nr, b, e in bad:
            assert bh.raw_task_gates(c, nn, bh.T0, bh.MIN_LEN, bh.MIN_MAPQ, flags, nr, b, e) == _abi.E_INVALID, (nn, flags, nr)
            assert "csv_bam_task_gates" in L.csv_last_error(c._h).decode()
            # the gates the context holds are those of the last good call: a consumer still reads them
            sig = extract.cigar_signatures(c, None, None, None, "gates", from_bam=cols)
            ref = extract.cigar_signatures(c, None, None, None, (want & _abi.GATE_USE) != 0, from_bam=cols)
            assert all(np.array_equal(sig[k], ref[k]) for k, _, _ in _abi.CIGAR_OUT)
            works()
        # end < beg is no error, 0 regions pass nothing, n_records == 0 is fine on an empty decode
        assert bh.raw_task_gates(c, n, 0, 0, 0, _abi.GT_BED, 3, beg, end[::-1].copy()) == _abi.OK
        assert not extract.task_gates(c, n, 0, 0, 0, []).any()
        # a flag together with a pointer
        works()
        one = np.ones(n, np.uint8)
        cin, cout = bh.cigar_in_out(n, _abi.CG_FROM_BAM | _abi.CG_USE_FROM_GATES, use=one)
        assert L.csv_cigar_signatures(c._h, bh.byref(cin), bh.byref(cout)) == _abi.E_INVALID
        cin, cout = bh.cigar_in_out(n, _abi.CG_USE_FROM_GATES)                # ... and without CSV_CG_FROM_BAM
        assert L.csv_cigar_signatures(c._h, bh.byref(cin), bh.byref(cout)) == _abi.E_INVALID
        sin, sout, _keep = bh.sa_in_out(n, _abi.SA_SEL_FROM_GATES, sel=one)
        assert L.csv_bam_split_inputs(c._h, bh.byref(sin), bh.byref(sout)) == _abi.E_INVALID
        with pytest.raises(ValueError):
            extract.cigar_signatures(c, None, None, None, "gates")
        works()
        # a second decode without new gates: the column belongs to the first
        cols = bam.decode(c, chunk, host_outputs=False)
        with pytest.raises(engine.CsvError) as e:
            extract.cigar_signatures(c, None, None, None, "gates", from_bam=cols)
        assert e.value.code == _abi.E_INVALID
        with pytest.raises(engine.CsvError) as e:
            extract.split_inputs_bam(c, chunk, cols, "gates", {"7": 0}, "7", bh.MIN_MAPQ, gate_bits=want)
        assert e.value.code == _abi.E_INVALID
        works()
        sig = extract.cigar_signatures(c, None, None, None, "gates", from_bam=cols)
        ref = extract.cigar_signatures(c, None, None, None, (want & _abi.GATE_USE) != 0, from_bam=cols)
        assert all(np.array_equal(sig[k], ref[k]) for k, _, _ in _abi.CIGAR_OUT)
        si = extract.split_inputs_bam(c, chunk, cols, "gates", {"7": 0}, "7", bh.MIN_MAPQ, gate_bits=want)
        ref = extract.split_inputs_bam(c, chunk, cols, (want & _abi.GATE_SEL) != 0, {"7": 0}, "7", bh.MIN_MAPQ)
        assert si["n_calls"] == ref["n_calls"] > 0 and all(np.array_equal(si[k], ref[k]) for k, _, _ in _abi.SA_CALL + _abi.SA_ENT)
        # an empty chunk
        with bam.BamFile(str(tmp_path / ("gates%d_11.bam" % n))) as bf:
            empty = bf.records("7", 190000, 190001)
        assert empty.n == 0
        bam.decode(c, empty, host_outputs=False)
        assert len(extract.task_gates(c, 0, 0, 0, 0, [(1, 2)])) == 0


# ------------------------------------------------------------------------------------------------ GPU: end to end
@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = tmp_path_factory.mktemp("bedcall")
    path = str(d / "planted.bam")
    ref = call_helpers.write_planted_bam(path)
    return path, ref, _write(d / "ins.bed", "chrA\t9000\t11000\nchrZ\t5\t500\n"), d


def _records(text):
    return [ln.split("\t") for ln in text.splitlines()]


def _kinds(text):
    return [re.search(r"SVTYPE=(\w+)", r[7]).group(1) for r in _records(text)]


def _support(rec):
    return int(re.search(r"RE=(\d+)", rec[7]).group(1))


@pytest.mark.gpu
@pytest.mark.parametrize("genotype,report_readid,batch", [(False, False, 10_000_000), (True, False, 10_000_000), (True, True, 10_000_000), (False, False, 2000),
                                                           (True, True, 2000)])
def test_gpu_call_bam_with_a_bed_is_the_bed_aware_route(ctx, planted, monkeypatch, genotype, report_readid, batch):
    monkeypatch.setenv("CUTESV_AMD_TRA_GT", "reads_table")
    path, ref, bed_path, _ = planted
    cp = call.CallParams(Params.ont(min_support=3, genotype=genotype))
    regions = bed.load_bed(bed_path)
    with bam.BamFile(path) as bf:
        want = bh.bed_route(ctx, bf, ref, cp, regions, batch=batch, report_readid=report_readid)
        got, svid = call.call_bam(bf, ref, cp, ctx=ctx, batch=batch, report_readid=report_readid, include_bed=bed_path)
        again, _ = call.call_bam(bf, ref, cp, ctx=ctx, batch=batch, report_readid=report_readid, include_bed=regions, gates="host")
    assert got == want and again == got
    kinds = _kinds(got)
    assert kinds.count("INS") >= 1 and not {"DEL", "DUP", "BND"} & set(kinds)
    ins = [r for r in _records(got) if r[0] == "chrA" and abs(int(r[1]) - 10000) <= 5]
    assert len(ins) == 1 and len(ins[0][4]) > 100
    assert int(svid.sum()) == len(kinds)


@pytest.mark.gpu
def test_gpu_the_cut_matters_with_a_bed_and_not_without(ctx, planted, monkeypatch):
    monkeypatch.setenv("CUTESV_AMD_TRA_GT", "reads_table")
    path, ref, bed_path, _ = planted
    cp = call.CallParams(Params.ont(min_support=3))
    with bam.BamFile(path) as bf:
        one, _ = call.call_bam(bf, ref, cp, ctx=ctx, include_bed=bed_path)
        cut, _ = call.call_bam(bf, ref, cp, ctx=ctx, include_bed=bed_path, batch=2000)
        # without a BED nothing changed: the parent's route, whichever side evaluates the gates
        want = call_helpers.parent_route(ctx, bf, ref, cp)
        assert call.call_bam(bf, ref, cp, ctx=ctx)[0] == want
        assert call.call_bam(bf, ref, cp, ctx=ctx, gates="device")[0] == want
        assert call.call_bam(bf, ref, cp, ctx=ctx, gates="host", batch=2000)[0] == call.call_bam(bf, ref, cp, ctx=ctx, gates="device", batch=2000)[0]
    at = lambda text: [r for r in _records(text) if r[0] == "chrA" and abs(int(r[1]) - 10000) <= 5]      # noqa: E731
    assert len(at(one)) == 1 and len(at(cut)) == 1
    assert _support(at(cut)[0]) < _support(at(one)[0]) == _support(at(want)[0])


@pytest.mark.gpu
def test_gpu_tra_genotyping_from_alignments_is_not_gated(ctx, planted):
    path, ref, _, d = planted
    cp = call.CallParams(Params.ont(min_support=3, genotype=True))
    with bam.BamFile(path) as bf:
        full, _ = call.call_bam(bf, ref, cp, ctx=ctx, tra_gt="alignments")
        part, _ = call.call_bam(bf, ref, cp, ctx=ctx, tra_gt="alignments", include_bed=_write(d / "tra.bed", "chrA\t24000\t26000\n"))
    bnd = lambda text: [ln for ln in text.splitlines() if "SVTYPE=BND" in ln]      # noqa: E731
    assert len(bnd(full)) >= 1 and bnd(part) == bnd(full)
    assert bnd(full)[0].split("\t")[9].split(":")[0] != "./."
    assert "DEL" in _kinds(full) and "DEL" not in _kinds(part)


@pytest.mark.gpu
def test_gpu_empty_outcomes_and_the_command_line(ctx, planted, tmp_path):
    path, ref, bed_path, d = planted
    cp = call.CallParams(Params.ont(min_support=3))
    with bam.BamFile(path) as bf:
        assert call.call_bam(bf, ref, cp, ctx=ctx, include_bed=_write(d / "empty.bed", ""))[0] == ""
        assert call.call_bam(bf, ref, cp, ctx=ctx, include_bed=_write(d / "unknown.bed", "chrZ\t1\t100000\nchrQ\t5\t9\n"))[0] == ""
        assert call.call_bam(bf, ref, cp, ctx=ctx, include_bed=bed.Regions.from_intervals({}), as_bytes=True)[0] == b""
        text, _ = call.call_bam(bf, ref, cp, ctx=ctx, include_bed=bed_path)
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as f:
        for c, s in ref.items():
            f.write(">%s\n" % c + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")
    out = str(tmp_path / "out.body.vcf")
    assert call.main([path, fa, "-o", out, "--preset", "ont", "--min_support", "3", "--include_bed", bed_path]) == 0
    with open(out) as f:
        assert f.read() == text and text
