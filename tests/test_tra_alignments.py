"""TRA genotyping from every alignment (cutesv_amd/aln.py, csrc/aln.hip.h): the device-resident
alignment table, its append from a decoded BAM chunk, the walk of call_gt / count_coverage over it, and call_bam's
`alignments` mode.

CPU: the host twin (aln.tra_genotype_host, built on tra_bam.window_status) against the reference's recorded call_gt rows; the
mode switch; the interface.  GPU: the kernels against the twin - the golden cases, a crafted table that holds every edge of
the walk, random tables - the append against the BAM writer's own record list, the refusals, and call_bam end to end against
tra_bam.call_gt over a stub fetch of the records that were written."""
import os
import re
import types

import numpy as np
import pytest

from cutesv_amd import _abi, _lib, aln, bam, call, engine, extract, rebuild, tra_bam
from cutesv_amd.columns import Params, TYPES
from cutesv_amd.genotype import gl_fields, gl_index
from helpers import load_json, store_from_json
import bam_writer
import call_helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("csv_aln_reset", "csv_aln_rows", "csv_aln_append_decoded", "csv_aln_append", "csv_aln_get", "csv_aln_layout", "csv_aln_timing", "csv_aln_tra_genotype")


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ the golden cases, as tables and calls
def golden_case(case):
    """a case of tra_genotype.json.gz -> (per-chromosome table columns, calls dict, the recorded rows, contig_len, params): the table
    is the case's reads table with flag 0 for primary and 2048 otherwise (the stand-in the recorded rows were made with)"""
    st = store_from_json(case["store"])
    name_id = {st.names[i]: i for i in range(len(st.names))}
    per = []
    for c in range(len(st.chroms)):
        r0, r1 = int(st.reads_off[c]), int(st.reads_off[c + 1])
        per.append((st.r_start[r0:r1], st.r_end[r0:r1], st.r_primary[r0:r1] == 1, st.r_id[r0:r1]))
    calls = dict(chrom1=[], pos1=[], chrom2=[], pos2=[], support_off=[0], support=[])
    rows = []
    for t, _, rs in case["rows"]:
        if t != "TRA":
            continue
        for r in rs:
            calls["chrom1"].append(st.chroms.index(r[0])); calls["pos1"].append(int(r[2]))
            calls["chrom2"].append(st.chroms.index(r[3])); calls["pos2"].append(int(r[4]))
            calls["support"].extend(name_id[q] for q in r[11].split(","))
            calls["support_off"].append(len(calls["support"]))
            rows.append(r)
    return per, calls, rows, st.contig_len, case["params"]


def check_recorded(case_name, rows, calls, dr, status):
    """(dr, status) of the calls against the recorded rows: DR and the genotype fields via gl_fields"""
    for k, r in enumerate(rows):
        dv = len(set(r[11].split(",")))
        assert dv == calls["support_off"][k + 1] - calls["support_off"][k] == int(r[5]), (case_name, k)
        if r[6] == ".":
            assert status[k] == -1 and dr[k] == -1, (case_name, k)
            assert r[7:11] == ["./.", ".,.,.", ".", "."]
        else:
            assert status[k] != -1 and int(dr[k]) == int(r[6]), (case_name, k, int(dr[k]), r[6])
            assert list(gl_fields(gl_index(int(dr[k]), dv))) == r[7:11], (case_name, k)


def test_host_twin_reproduces_the_recorded_call_gt_rows():
    n = 0
    seen = set()
    for case in load_json("tra_genotype.json.gz"):
        per, calls, rows, contig_len, p = golden_case(case)
        dr, status = aln.tra_genotype_host(aln.Table.from_chroms(per), contig_len=contig_len, bias=p["max_cluster_bias_TRA"], gt_round=p["gt_round"], **calls)
        check_recorded(case["name"], rows, calls, dr, status)
        n += len(rows)
        seen.update(status.tolist())
    assert n > 20 and seen == {0, 1, -1}


def test_tra_gt_modes_accept_alignments_and_refuse_bam(monkeypatch):
    monkeypatch.setenv("CUTESV_AMD_TRA_GT", "alignments")
    assert call.tra_gt_mode(True) == "alignments" and call.tra_gt_mode(False) == "off"
    assert call.tra_gt_mode(True, "reads_table") == "reads_table"              # (the keyword goes before the environment)
    monkeypatch.setenv("CUTESV_AMD_TRA_GT", "bam")
    assert call.tra_gt_mode(True, "alignments") == "alignments"
    with pytest.raises(ValueError) as e:
        call.tra_gt_mode(True)
    assert all(w in str(e.value) for w in ("alignments", "reads_table", "off"))
    with pytest.raises(ValueError):
        call.tra_gt_mode(True, "bam")
    monkeypatch.delenv("CUTESV_AMD_TRA_GT")
    with pytest.raises(ValueError):                                             # (unset means resolve's default, bam)
        call.tra_gt_mode(True)


def test_abi_is_still_9_and_the_new_entries_are_bound():
    with open(os.path.join(ROOT, "include", "cutesv_hip.h")) as f:
        header = f.read()
    assert re.search(r"^#define CSV_ABI_VERSION 9$", header, re.M)
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    L = _lib.lib()
    assert L.csv_abi_version() == _abi.ABI_VERSION == 9
    for entry in NEW_SYMBOLS:
        m = re.search(r"^int %s\(([^;]*)\);" % entry, header, re.M | re.S)
        assert m, entry
        res, args = bound[entry]
        assert res is _lib.C.c_int and len(args) == m.group(1).count(",") + 1, entry       # one ctypes argument per declared parameter
        assert getattr(L, entry).argtypes == args
    one = np.zeros(1, np.int64)
    assert L.csv_aln_reset(None, 1) == _abi.E_INVALID and L.csv_aln_rows(None, None) == _abi.E_INVALID
    assert L.csv_aln_tra_genotype(None, 0, None, None, None, None, one.ctypes.data, None, 0, 0, None, 0, 0, None, None) == _abi.E_INVALID
    assert (_abi.ALN_FROM_KEPT_REBUILD, _abi.ALN_SUPPORT_I32) == (1, 2)
    assert re.search(r"CSV_ALN_FROM_KEPT_REBUILD = 1, CSV_ALN_SUPPORT_I32 = 2", header)


def test_decoded_end_rule():
    got = aln.decoded_end([10, 10, 10, 10, 2 ** 31 - 5], [0, 7, 7, -3, 100], [0, 4, 16, 0, 0])
    assert got.tolist() == [11, 11, 17, 11, 2 ** 31 - 1]


# ------------------------------------------------------------------------------------------------ GPU: helpers
def fill(ctx, per):
    aln.reset(ctx, len(per))
    for c, (s, e, p, i) in enumerate(per):
        aln.append(ctx, c, s, e, p, i)
    return aln.Table.from_chroms(per)


def both(ctx, table, calls, contig_len, bias, gt_round):
    """the kernel's answer, checked against the twin's"""
    dr, status = aln.tra_genotype(ctx, contig_len=contig_len, bias=bias, gt_round=gt_round, **calls)
    hdr, hstatus = aln.tra_genotype_host(table, contig_len=contig_len, bias=bias, gt_round=gt_round, **calls)
    assert status.tolist() == hstatus.tolist(), (bias, gt_round)
    assert dr.tolist() == hdr.tolist(), (bias, gt_round)
    return dr, status


@pytest.mark.gpu
def test_gpu_golden_cases_in_plain_id_mode(ctx):
    names = set()
    for case in load_json("tra_genotype.json.gz"):
        per, calls, rows, contig_len, p = golden_case(case)
        if not rows:
            continue
        table = fill(ctx, per)
        assert aln.rows(ctx) == len(table.start)
        dr, status = both(ctx, table, calls, contig_len, p["max_cluster_bias_TRA"], p["gt_round"])
        check_recorded(case["name"], rows, calls, dr, status)
        names.add(case["name"])
    assert {"tra_round8_dark", "tra_lowsup_upbound", "tra_deep"} <= names


# ------------------------------------------------------------------------------------------------ GPU: the crafted table
CRAFT_LEN = [100_000, 50_000, 10_000]          # contig 2 has no rows


def crafted():
    """-> (per-chromosome columns, calls, notes).  Contig 0: row 0 is a 90 000-base secondary record that sets maxlen, so every
    window's walk starts at row 0 and a row's lane is its index mod 64; rows 1 .. 62 end before any window; row 63 is the first
    row of region A (window [4200, 5800) for pos 5000, bias 800)."""
    A = [(10, 90_010, 2048, 900)] + [(20 + i, 70 + i, 0, 1000 + i) for i in range(62)]
    A += [
        (4000, 5801, 0, 1),          # row 63 (lane 63): spans [4200, 5800), not [4201, 5801)
        (4001, 6000, 16, 2),         # row 64 (lane 0 of the next step): spans both
        (4002, 6001, 0, 1),          # name 1 again, across steps
        (4003, 6002, 0, 2),          # name 2 again, inside the step
        (4004, 6000, 256, 3), (4005, 6000, 272, 4), (4006, 6000, 2048, 5), (4007, 6000, 2064, 6),      # counted, never primary
        (4010, 6500, 0, 50),         # a spanning name that supports the calls
        (4100, 4200, 0, 8),          # end == s: not fetched
        (4150, 5800, 0, 9),          # end == e: fetched, does not span
        (4200, 7000, 0, 10),         # start == s: does not span
        (4250, 7000, 0, 11),         # (a primary with MAPQ 0: the table does not know the MAPQ)
        (4300, 4301, 4, 7),          # placed-unmapped: end = start + 1, counted
        (5799, 5900, 0, 12),         # start == e - 1: fetched
        (5800, 5900, 0, 13),         # start == e: not fetched
    ]
    A += [(6000 + 7 * i, 6400 + 7 * i, 0 if i % 3 else 256, 2000 + i % 40) for i in range(130)]          # further steps on the way to region C
    A += [(9000 - 300 + i, 9000 + 400 + i, 0, 3000 + i % 25) for i in range(60)]                          # region C at 9000: 60 spanning rows, 25 names, for bias 50
    B = [(2100 + i, 4000, 256, 4000 + i) for i in range(10)]                                            # region B at 3000: ten secondaries first
    B += [(2150, 4000, 0, 70), (2160, 4100, 0, 71), (2170, 4100, 16, 50), (2180, 3500, 0, 72)]
    B += [(49_000, 50_010, 0, 60), (49_500, 49_600, 0, 61)]                                            # at the end of the contig
    per = []
    for rows in (A, B, []):
        rows = sorted(rows, key=lambda r: r[0])
        per.append((np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int32), np.array([r[2] in (0, 16) for r in rows], np.uint8),
                    np.array([r[3] for r in rows], np.int32)))
    assert per[0][0][63] == 4000 and per[0][0][64] == 4001 and sum(len(x[0]) for x in per) > 280
    big = list(range(100_000, 103_499)) + [50]
    call_list = [
        (0, 5000, 1, 3000, [50, 51, 52]),        # 0
        (0, 5000, 2, 500, []),                   # 1: no supports -> up_bound 0: exit A at the first spanning row, row 63
        (0, 5001, 2, 500, []),                   # 2: ... at row 64
        (1, 3000, 2, 500, [50]),                 # 3: chrom2 without rows
        (0, 300, 1, 3000, [1]),                  # 4: clamped at 0
        (1, 49_900, 0, 5000, [2]),               # 5: clamped at contig_len
        (1, 50_900, 0, 5000, [3]),               # 6: empty after the clamp; window 2 is walked
        (0, 5000, 1, 3000, big),                 # 7: 3 500 supports: the global-set pass
        (1, 3000, 0, 5000, [50, 51]),            # 8
        (0, 9000, 1, 3000, [3001]),              # 9: one support -> up_bound 20, reached in region C
        (2, 500, 2, 600, [5]),                   # 10: both windows on the empty contig
    ]
    calls = dict(chrom1=[c[0] for c in call_list], pos1=[c[1] for c in call_list], chrom2=[c[2] for c in call_list], pos2=[c[3] for c in call_list],
                 support_off=np.r_[0, np.cumsum([len(c[4]) for c in call_list])], support=[x for c in call_list for x in c[4]])
    return per, calls


@pytest.mark.gpu
def test_gpu_crafted_table_against_the_twin(ctx):
    per, calls = crafted()
    table = fill(ctx, per)
    off, maxlen = aln.layout(ctx, 3)
    assert off.tolist() == table.off.tolist() and maxlen.tolist() == [90_000, 1940, 0]
    back = aln.get(ctx)
    for k, name in enumerate(("start", "end", "primary", "id")):
        assert back[name].tolist() == np.concatenate([x[k] for x in per]).tolist(), name
    seen = set()
    for gt_round in (2, 3, 5, 12, 500):
        dr, status = both(ctx, table, calls, CRAFT_LEN, 800, gt_round)
        seen.update(status.tolist())
        if gt_round == 500:
            # exit A on lane 63 and on lane 0 of the next step: one name each, nothing behind the stopping lane is committed
            assert (status[1], dr[1], status[2], dr[2]) == (1, 1, 1, 1)
            # names 1 and 2 count once each, 50 is a support; window 2 adds 70 and 71 (50 again; 72 ends inside the window)
            assert (status[0], dr[0]) == (0, 4)
            assert (status[7], dr[7]) == (0, 4)                     # the same through the global set
            assert (status[3], dr[3]) == (0, 2) and (status[10], dr[10]) == (0, 0)
            assert (status[6], dr[6]) == (0, 3)                     # window 1 empty, window 2 = region A: names 1, 2, 50
        if gt_round == 2:
            assert status[0] == -1 and dr[0] == -1                  # row 63 is the second row of the walk and primary: 1 of 2
        if gt_round == 12:
            assert (status[8], dr[8]) == (1, 2)                     # 10 secondaries, then the second primary: 2 of 12
    assert seen == {0, 1, -1}
    dr, status = both(ctx, table, calls, CRAFT_LEN, 50, 500)
    assert status[9] == 1 and dr[9] == 19                           # up_bound 20 reached at the 20th name; one of them supports


# ------------------------------------------------------------------------------------------------ GPU: random tables
def random_table(rng, n_rows, lens):
    per = []
    for c, n in enumerate(n_rows):
        start = np.sort(rng.integers(0, lens[c], n)).astype(np.int32)
        length = rng.integers(1, 3000, n)
        length[rng.integers(0, n, 3)] = rng.integers(20_000, 40_000, 3)
        flag = rng.choice([0, 16, 256, 272, 2048, 2064, 4], n, p=[.35, .3, .1, .05, .1, .05, .05])
        per.append((start, (start + np.where(flag == 4, 1, length)).astype(np.int32), np.isin(flag, (0, 16)).astype(np.uint8), rng.integers(0, 400, n).astype(np.int32)))
    return per


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2])
def test_gpu_random_tables_against_the_twin(ctx, seed):
    rng = np.random.default_rng(seed)
    lens = [60_000, 45_000]
    per = random_table(rng, [1800, 1200], lens)
    table = fill(ctx, per)
    n = 200
    chrom1, chrom2 = rng.integers(0, 2, n), rng.integers(0, 2, n)
    pos1 = np.array([rng.integers(0, lens[c] + 500) for c in chrom1]); pos2 = np.array([rng.integers(0, lens[c] + 500) for c in chrom2])
    sizes = rng.choice([0, 1, 2, 3, 6, 16, 40], n)
    calls = dict(chrom1=chrom1, pos1=pos1, chrom2=chrom2, pos2=pos2, support_off=np.r_[0, np.cumsum(sizes)], support=rng.integers(0, 450, int(sizes.sum())))
    seen = set()
    for gt_round in (3, 25, 500):
        for bias in (50, 800):
            dr, status = both(ctx, table, calls, lens, bias, gt_round)
            seen.update(status.tolist())
    assert seen == {0, 1, -1}
    # the narrow support list is the same call
    dr32, st32 = aln.tra_genotype(ctx, contig_len=lens, bias=800, gt_round=25, **dict(calls, support=calls["support"].astype(np.int32)))
    dr64, st64 = aln.tra_genotype(ctx, contig_len=lens, bias=800, gt_round=25, **calls)
    assert dr32.tolist() == dr64.tolist() and st32.tolist() == st64.tolist()


# ------------------------------------------------------------------------------------------------ GPU: the append from a decode
DEC_CONTIGS = [("chrB", 9000), ("chrA", 7000)]                      # (header order is not name order)


def decode_records(seed=11):
    rng = np.random.default_rng(seed)
    recs = []
    flags = [0, 16, 256, 272, 2048, 2064, 4]
    k = 0
    for refid, (_, length) in enumerate(DEC_CONTIGS):
        starts = sorted(rng.integers(0, length - 1200, 70).tolist() + [1900, 1999, 2000, 3999, 4000])       # task edges; 1900 crosses one
        for s in starts:
            m = int(rng.integers(300, 1100))
            cigar = [(4, 20), (0, m), (2, 15), (0, 30), (1, 12), (0, 40)] if k % 3 == 0 else [(0, m)]
            if k % 17 == 5:
                cigar = []                                           # a record without CIGAR
            qlen = sum(n for op, n in cigar if op in (0, 1, 4)) or 50
            recs.append(dict(name="r%03d" % (k % 90), flag=flags[k % 7], mapq=int(rng.integers(0, 61)), start=int(s), cigar=cigar,
                             seq="".join("ACGT"[i] for i in rng.integers(0, 4, qlen)), tags=[], refid=refid))
            k += 1
    return recs


def record_end(r):
    span = sum(n for op, n in r["cigar"] if op in (0, 2, 3, 7, 8))
    return int(aln.decoded_end([r["start"]], [span], [r["flag"]])[0])


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [2000, 10_000_000])
def test_gpu_append_from_a_decode_is_the_writers_record_list(ctx, tmp_path, batch):
    recs = decode_records()
    path = str(tmp_path / "dec.bam")
    bam_writer.write_bam(path, DEC_CONTIGS, recs)
    names = sorted(c for c, _ in DEC_CONTIGS)
    crank = {c: i for i, c in enumerate(names)}
    length = dict(DEC_CONTIGS)
    cp = call.CallParams(Params.ont(min_support=3))
    seg_of = {t: ti * 2 for ti, t in enumerate(TYPES)}
    seg_base = [seg_of[t] for t in ("DEL", "INS", "DUP", "INV", "TRA")]
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx); aln.reset(ctx, 2)
    n_rows = 0
    with bam.BamFile(path) as bf:
        for c in names:
            for t0, t1 in call.cut_tasks(length[c], batch):
                r = extract.task_to_pool(ctx, bf, c, t0, t1, crank, *cp.pipe_args(), seg_of["INS"] + crank[c], seg_of["DEL"] + crank[c], seg_base, None,
                                         name_pool=True, aln=True)
                n_rows += r["n_aln_rows"]
                with pytest.raises(ValueError):
                    extract.task_to_pool(ctx, bf, c, t0, t1, crank, *cp.pipe_args(), 0, 0, seg_base, 0, aln=True)         # (needs the name pool)
    want = [r for c in names for r in recs if DEC_CONTIGS[r["refid"]][0] == c]            # by chromosome rank, in file order
    assert n_rows == aln.rows(ctx) == len(want) == len(recs)
    got = aln.get(ctx)
    assert got["start"].tolist() == [r["start"] for r in want]
    assert got["end"].tolist() == [record_end(r) for r in want]
    assert got["primary"].tolist() == [int(r["flag"] in (0, 16)) for r in want]
    assert rebuild.name_pool_get(ctx, got["id"]) == [r["name"] for r in want]             # ids are name-pool indices
    assert len(set(got["id"].tolist())) == len(want) and int(got["id"].max()) < rebuild.name_pool_rows(ctx)
    off, maxlen = aln.layout(ctx, 2)
    n_a = sum(1 for r in want if DEC_CONTIGS[r["refid"]][0] == "chrA")
    assert off.tolist() == [0, n_a, len(want)]
    assert maxlen.tolist() == [max(record_end(r) - r["start"] for r in want[:n_a]), max(record_end(r) - r["start"] for r in want[n_a:])]
    assert {r["flag"] for r in want} == {0, 16, 256, 272, 2048, 2064, 4} and any(not r["cigar"] for r in want)
    assert min(r["mapq"] for r in want) < 5 and max(r["mapq"] for r in want) > 55


# ------------------------------------------------------------------------------------------------ GPU: refusals
def refused(code, fn, *a, **kw):
    with pytest.raises(engine.CsvError) as e:
        fn(*a, **kw)
    assert e.value.code == code, e.value


@pytest.mark.gpu
def test_gpu_refusals_leave_the_table_unchanged():
    """every refusal is a host-side check, or the device's order flag over rows that lie behind the table's count"""
    c = engine.Context(0)
    try:
        refused(_abi.E_INVALID, aln.append_decoded, c, 0, 0, 100, 0)                       # no table, no decode
        aln.reset(c, 3)
        refused(_abi.E_INVALID, aln.append_decoded, c, 0, 0, 100, 0)                       # no decode
        aln.append(c, 1, [100, 200, 200], [150, 900, 260], [1, 0, 1], [5, 6, 7])
        calls = dict(chrom1=[1], pos1=[210], chrom2=[1], pos2=[240], support_off=[0, 1], support=[5])
        lens = [1000, 1000, 1000]

        def works(n):
            assert aln.rows(c) == n
            dr, status = aln.tra_genotype(c, contig_len=lens, bias=20, gt_round=500, **calls)
            assert status.tolist() == [0] and dr.tolist() == [0]
        works(3)
        refused(_abi.E_UNSORTED, aln.append, c, 1, [300, 250], [400, 400], [1, 1], [1, 2])      # inside the append
        works(3)
        refused(_abi.E_UNSORTED, aln.append, c, 1, [199], [400], [1], [1])                      # against the table's last row
        works(3)
        refused(_abi.E_UNSORTED, aln.append, c, 0, [500], [600], [1], [1])                      # a chromosome that was passed
        refused(_abi.E_INVALID, aln.append, c, 3, [500], [600], [1], [1])
        refused(_abi.E_INVALID, aln.append, c, -1, [500], [600], [1], [1])
        refused(_abi.E_INVALID, aln.append, c, 1, [500], [500], [1], [1])                       # end <= start
        refused(_abi.E_INVALID, aln.append, c, 1, [500], [600], [1], [-1])
        works(3)
        aln.append(c, 1, [200], [9000], [0], [9])                                               # an equal start is in order; maxlen follows
        aln.append(c, 2, [0], [10], [1], [1])
        assert aln.layout(c, 3)[0].tolist() == [0, 0, 4, 5] and aln.layout(c, 3)[1].tolist() == [0, 8800, 10]
        works(5)
        # the genotype entry: offsets, supports, chromosomes, the chromosome count
        bad = [dict(calls, support_off=[1, 1]), dict(calls, support_off=[0, 2, 1], chrom1=[1, 1], pos1=[1, 1], chrom2=[1, 1], pos2=[1, 1], support=[5, 5]),
               dict(calls, support=[-1]), dict(calls, support=[2 ** 31]), dict(calls, chrom1=[3]), dict(calls, chrom2=[-1])]
        for kw in bad:
            refused(_abi.E_INVALID, aln.tra_genotype, c, contig_len=lens, bias=20, gt_round=500, **kw)
            works(5)
        refused(_abi.E_INVALID, aln.tra_genotype, c, contig_len=lens[:2], bias=20, gt_round=500, **calls)
        refused(_abi.E_INVALID, aln.tra_genotype, c, contig_len=lens, bias=20, gt_round=500, flags=aln.FROM_KEPT_REBUILD, **calls)     # no kept rebuild
        works(5)
        # rank mode: a kept rebuild by name whose pools are then touched
        rebuild.pool_reset(c); rebuild.name_pool_reset(c)
        rebuild.name_pool_append(c, b"bbaacc", [0, 2, 4], [2, 2, 2])                            # names 0, 1, 2 = bb, aa, cc -> ranks 1, 0, 2
        rebuild.pool_append(c, [0, 0], [10, 20], [5, 5], [2, 0], [0, 0])                        # two DEL rows of reads cc, bb
        aln.reset(c, 1)
        aln.append(c, 0, [100, 110, 120], [900, 900, 900], [1, 1, 1], [0, 1, 2])
        keep = lambda: rebuild.rebuild_pool_by_name(c, np.zeros(1, np.uint8), np.zeros(1, np.uint8), keep_on_device=True)
        rb = keep()
        rk = dict(chrom1=[0], pos1=[500], chrom2=[0], pos2=[500], support_off=[0, 2], support=[0, 1])

        def rank_works():
            dr, status = aln.tra_genotype(c, contig_len=[1000], bias=100, gt_round=500, flags=aln.FROM_KEPT_REBUILD, **rk)
            assert status.tolist() == [0] and dr.tolist() == [1]                                # bb and cc support, aa does not
        assert rb["n_out"] == 2
        rank_works()
        refused(_abi.E_INVALID, aln.tra_genotype, c, contig_len=[1000], bias=100, gt_round=500, flags=aln.FROM_KEPT_REBUILD, **dict(rk, support=[0, 2]))   # a row outside the rebuild
        rank_works()
        for change in (lambda: rebuild.name_pool_append(c, b"zz", [0], [2]), lambda: rebuild.pool_reset(c)):
            change()
            refused(_abi.E_INVALID, aln.tra_genotype, c, contig_len=[1000], bias=100, gt_round=500, flags=aln.FROM_KEPT_REBUILD, **rk)
            assert aln.rows(c) == 3
            if rebuild.pool_rows(c) == 0:
                rebuild.pool_append(c, [0, 0], [10, 20], [5, 5], [2, 0], [0, 0])
            keep()
            rank_works()
        # a table id outside the name pool
        aln.append(c, 0, [130], [140], [1], [99])
        refused(_abi.E_INVALID, aln.tra_genotype, c, contig_len=[1000], bias=100, gt_round=500, flags=aln.FROM_KEPT_REBUILD, **rk)
        dr, status = aln.tra_genotype(c, contig_len=[1000], bias=100, gt_round=500, **rk)       # (plain ids still work)
        assert status.tolist() == [0]
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ GPU: end to end
def planted_with_noise():
    """the planted BAM's records plus, around both TRA breakpoints, what never reaches the reads table: secondary and
    supplementary copies, and MAPQ-0 primaries that span the windows"""
    recs, ref = call_helpers.planted_records()
    refid = {c: i for i, (c, _) in enumerate(call_helpers.CONTIGS)}
    rng = np.random.default_rng(77)

    def add(name, chrom, start, length, flag, mapq):
        recs.append(dict(name=name, flag=flag, mapq=mapq, start=start, cigar=[(0, length)], seq="".join("ACGT"[i] for i in rng.integers(0, 4, length)), tags=[],
                         refid=refid[chrom]))
    for k in range(5):
        add("mq0_%d" % k, "chrA", 23_000 + 40 * k, 4000, 0 if k % 2 else 16, 0)              # span chrA:25000 +- 50 .. 1000
        add("mq0b_%d" % k, "chrB", 10_000 + 40 * k, 4000, 0, 0)
    for k in range(6):
        add("sec%d" % k, "chrA", 24_000 + 100 * k, 1500, (256, 272, 2048, 2064)[k % 4], 60)
        add("secb%d" % k, "chrB", 11_500 + 100 * k, 1500, (256, 2048)[k % 2], 30)
    recs.sort(key=lambda r: (r["refid"], r["start"]))
    return recs, ref


class _Records:
    """pysam.AlignmentFile stand-in over the writer's record list: fetch() yields every record that overlaps, as htslib does"""

    def __init__(self, recs):
        self.recs = recs

    def get_reference_length(self, chrom):
        return dict(call_helpers.CONTIGS)[chrom]

    def fetch(self, chrom, s, e):
        rid = [c for c, _ in call_helpers.CONTIGS].index(chrom)
        for r in self.recs:
            if r["refid"] == rid and r["start"] < e and record_end(r) > s:
                yield types.SimpleNamespace(flag=r["flag"], reference_start=r["start"], reference_end=record_end(r), query_name=r["name"])


def _bnd(text):
    return [ln.split("\t") for ln in text.splitlines() if "SVTYPE=BND" in ln]


@pytest.mark.gpu
@pytest.mark.parametrize("batch,report_readid", [(10_000_000, False), (2000, True)])
def test_gpu_call_bam_genotypes_bnd_records_from_every_alignment(ctx, tmp_path, monkeypatch, batch, report_readid):
    monkeypatch.delenv("CUTESV_AMD_TRA_GT", raising=False)
    recs, ref = planted_with_noise()
    path = str(tmp_path / "noise.bam")
    bam_writer.write_bam(path, call_helpers.CONTIGS, recs)
    p = Params.ont(min_support=3, genotype=True)
    cp = call.CallParams(p)
    timings = {}
    with bam.BamFile(path) as bf:
        table_mode, _ = call.call_bam(bf, ref, cp, ctx=ctx, batch=batch, report_readid=True, tra_gt="reads_table")
        got, svid = call.call_bam(bf, ref, cp, ctx=ctx, batch=batch, report_readid=True, tra_gt="alignments", timings=timings)
        shown, _ = call.call_bam(bf, ref, cp, ctx=ctx, batch=batch, report_readid=report_readid, tra_gt="alignments")
    monkeypatch.setenv("CUTESV_AMD_TRA_GT", "alignments")
    with bam.BamFile(path) as bf:
        assert call.call_bam(bf, ref, cp, ctx=ctx, batch=batch, report_readid=report_readid)[0] == shown          # (the environment selects it, too)
    assert "ms_tra_gt" in timings
    a, b = got.splitlines(), table_mode.splitlines()
    assert len(a) == len(b) == int(svid.sum())
    assert [x for x in a if "SVTYPE=BND" not in x] == [x for x in b if "SVTYPE=BND" not in x]
    bnd, bnd_table = _bnd(got), _bnd(table_mode)
    assert len(bnd) == len(bnd_table) >= 1
    stub = _Records(recs)
    differs = 0
    for r, rt in zip(bnd, bnd_table):
        info = dict(kv.split("=", 1) for kv in r[7].split(";") if "=" in kv)
        m = re.search(r"([\[\]])(\w+):(\d+)[\[\]]", r[4])
        # the row's positions behind POS and the mate (cuteSV_genotype.py:400-458): POS is pos + 1 when the ALT ends in the base, the mate pos + 1 for '['
        pos1 = int(r[1]) - (0 if r[4][0] not in "[]" else 1)
        pos2 = int(m.group(3)) - (1 if m.group(1) == "[" else 0)
        reads = info["RNAMES"].split(",")
        dv, dr, gt, pl, gq, qual = tra_bam.call_gt(stub, pos1, pos2, r[0], m.group(2), reads, p.max_cluster_bias_TRA, p.gt_round)
        fmt = dict(zip(r[8].split(":"), r[9].split(":")))
        assert (fmt["GT"], fmt["DR"], fmt["DV"], fmt["PL"], fmt["GQ"]) == (gt, dr, dv, pl, gq), (r, (dv, dr, gt, pl, gq, qual))
        assert r[5] == qual
        differs += dict(zip(rt[8].split(":"), rt[9].split(":")))["DR"] != fmt["DR"]
    assert differs >= 1                                     # the reads table does not hold what was added: its DR is another
    assert [ln.split("\t")[9] for ln in shown.splitlines()] == [ln.split("\t")[9] for ln in a]          # the same genotypes with and without RNAMES
    if not report_readid:
        # the command line with --genotype and nothing else said: the variable unset, no --tra_gt -> alignments
        monkeypatch.delenv("CUTESV_AMD_TRA_GT")
        fa, out = str(tmp_path / "ref.fa"), str(tmp_path / "out.body.vcf")
        with open(fa, "w") as f:
            for c, seq in ref.items():
                f.write(">%s\n" % c + "\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + "\n")
        assert call.main([path, fa, "-o", out, "--preset", "ont", "--min_support", "3", "--genotype"]) == 0
        with open(out) as f:
            assert f.read() == shown
        assert call.main([path, fa, "-o", out, "--preset", "ont", "--min_support", "3", "--genotype", "--tra_gt", "reads_table"]) == 0
        with open(out) as f:
            assert [ln.split("\t")[9] for ln in f.read().splitlines()] == [ln.split("\t")[9] for ln in b]
