"""Crafted reads tables for the genotype cover search (k_genotype), every tier.

CPU tests (no marker): the brute-force yardstick against the C oracle, against the sweep-line restatement and against the
reference's own overlap_cover (golden/cover_edges.json.gz), and the geometry every table claims, asserted from the table itself.
GPU tests (-m gpu): every table as int64 columns, as page-locked int32 columns and in extraction order, bit for bit against the
oracle and against the brute force; the route through the hash-set tiers from the CSV_DEBUG_COUNTERS line."""
import re

import numpy as np
import pytest

from cutesv_amd import _abi, engine
from helpers import assert_soa_equal, load_json

import cover_helpers as ch


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


def _calls(name):
    """[(call, chromosome, windows, search_pos, walk model of its first window)] of a table's genotyped calls"""
    st, _ = ch.table(name)
    hb, want, brute = ch.expected(name)
    return [(c, chrom, wins, int(want["search_pos"][c]), ch.walk(st, chrom, *wins[0])) for c, chrom, wins in ch.genotyped_calls(ch.PARAMS, hb.segments, want)]


def _dr_at(name, chrom_name, pos):
    st, _ = ch.table(name)
    hb, want, brute = ch.expected(name)
    hit = [i for i, c in enumerate(brute["call"]) if int(want["search_pos"][c]) == pos and st.chroms[int(hb.segments[int(want["call_seg"][c])]["chrom"])] == chrom_name]
    assert len(hit) == 1, (name, chrom_name, pos, hit)
    return int(brute["dr"][hit[0]])


# ------------------------------------------------------------------------------------------------ CPU: the yardsticks agree
@pytest.mark.parametrize("name", ch.ALL)
def test_brute_force_equals_oracle_and_sweep(name):
    """brute_dr == the C oracle's dr / dv / gl_idx on every call of every table; its cover counts == oracle.cover_count (the
    plain C loop) and, on the small tables, == py_restatement.sweep_cover"""
    from oracle import oracle, py_restatement as pr
    st, facts = ch.table(name)
    hb, want, brute = ch.expected(name)
    calls = ch.genotyped_calls(ch.PARAMS, hb.segments, want)
    n_gt = int(((hb.segments["genotype"] != 0) & (hb.segments["svtype"] != _abi.TRA))[want["call_seg"]].sum())
    assert len(brute["call"]) == len(calls) == n_gt == len(want["bp1"]) >= facts["placed"] > 0
    ch.assert_brute_equal(brute, want)
    assert brute["dr"].any() and (brute["dv"] >= 3).all()
    for chrom in sorted(set(c[1] for c in calls)):
        lo, hi = int(st.reads_off[chrom]), int(st.reads_off[chrom + 1])
        mine = [(i, w) for i, c in enumerate(calls) if c[1] == chrom for w in range(len(c[2]))]
        L2 = [calls[i][2][w][0] for i, w in mine]
        R2 = [calls[i][2][w][1] for i, w in mine]
        sizes = [len(brute["cover"][i][w]) for i, w in mine]
        got = oracle.cover_count(st.r_start[lo:hi], st.r_end[lo:hi], st.r_primary[lo:hi], st.r_id[lo:hi], L2, R2)
        assert got.tolist() == sizes, (name, chrom)
        if name in ch.SMALL:
            reads = list(zip(st.r_start[lo:hi].tolist(), st.r_end[lo:hi].tolist(), st.r_primary[lo:hi].tolist(), st.r_id[lo:hi].tolist()))
            sets = pr.sweep_cover([(l / 2, r / 2) for l, r in zip(L2, R2)], reads)
            assert [sorted(x) for x in sets] == [brute["cover"][i][w].tolist() for i, w in mine], (name, chrom)


def test_brute_force_equals_the_reference_overlap_cover():
    """golden/cover_edges.json.gz: the reference's own overlap_cover on the seam, tie and edge tables (make_golden_cover.py).
    The recorded rows are the builders' rows, and the recorded cover sets are brute_dr's."""
    cases = load_json("cover_edges.json.gz")
    assert sorted(set(c["table"] for c in cases)) == ["edge", "seam", "tie"]
    n_win = 0
    for case in cases:
        st, _ = ch.table(case["table"])
        hb, want, brute = ch.expected(case["table"])
        chrom = st.chroms.index(case["chrom"])
        lo, hi = int(st.reads_off[chrom]), int(st.reads_off[chrom + 1])
        for col, key in ((st.r_start, "start"), (st.r_end, "end"), (st.r_primary, "primary"), (st.r_id, "id")):
            assert col[lo:hi].tolist() == case[key], (case["table"], case["chrom"], key)
        calls = ch.genotyped_calls(ch.PARAMS, hb.segments, want)
        mine = [(i, w) for i, c in enumerate(calls) if c[1] == chrom for w in range(len(c[2]))]
        assert [list(calls[i][2][w]) for i, w in mine] == case["windows2"]
        assert [brute["cover"][i][w].tolist() for i, w in mine] == case["cover"], (case["table"], case["chrom"])
        n_win += len(mine)
    tot = sum(len(c[2]) for t in ("seam", "tie", "edge") for c in ch.genotyped_calls(ch.PARAMS, ch.expected(t)[0].segments, ch.expected(t)[1]))
    assert n_win == tot > 40


# ------------------------------------------------------------------------------------------------ CPU: the geometry each table claims
@pytest.mark.parametrize("name", ["walk_span", "walk_nonprimary", "walk_shift"])
def test_walk_tables_walk_down_to_the_first_chunk(name):
    st, facts = ch.table(name)
    w = st.chroms.index("w")
    r0, r1 = int(st.reads_off[w]), int(st.reads_off[w + 1])
    assert r1 - r0 == ch.WALK_N == 10 * 4096 and r0 == 100
    long_row = r0 + int(np.argmax(st.r_end[r0:r1] - st.r_start[r0:r1]))
    assert st.r_start[long_row] == st.r_start[r0:r1].min() and st.r_end[long_row] == st.r_end[r0:r1].max()
    assert st.r_primary[long_row] == (0 if name == "walk_nonprimary" else 1)
    calls = _calls(name)
    steps = {}
    for c, chrom, wins, pos, wk in calls:
        assert chrom == w and wk["closed"] == "c0" and wk["k0"] == 0 and wk["k1"] == 10
        steps[wk["ktop"] - wk["k0"]] = wk["steps2"]
        assert int(np.searchsorted(st.r_start[r0:r1], wins[0][0] >> 1, side="right")) - 1 + r0 in facts["rows"]     # L is the start of the row it names
    # both parities, and the single-block last step of an even distance
    assert steps == {0: 1, 1: 1, 2: 2, 3: 2, 8: 5, 9: 5}
    # rows with R - maxlen <= start <= L: more than three LDS tables' worth for the far windows
    assert max(ch.scan_rows(st, w, *c[2][0]) for c in calls) > 3 * 8192
    hb, want, brute = ch.expected(name)
    assert brute["dr"].tolist() == [29 if name == "walk_nonprimary" else 30] * 6        # 29 local reads (+ the whole-contig one)


def test_walk_middle_closes_in_a_middle_step():
    st, facts = ch.table("walk_middle")
    w = st.chroms.index("w")
    r0, r1 = int(st.reads_off[w]), int(st.reads_off[w + 1])
    long_row = r0 + int(np.argmax(st.r_end[r0:r1] - st.r_start[r0:r1]))
    assert (long_row - r0, int(np.searchsorted(st.r_start[r0:r1], st.r_end[long_row])) ) == (10001, 30001) and st.r_primary[long_row] == 1
    by = {wk["ktop"]: (wk["steps2"], wk["closed"]) for _, _, _, _, wk in _calls("walk_middle")}
    # row 35 000 (block 8): blocks 7-8, 5-6, then 3-4 holds the first chunk that begins before F; rows 30 500 and 39 000 alike;
    # row 5 000 (block 1) reaches the first chunk at once; row 20 000 (block 4) walks 3-4, 1-2, 0
    assert by == {1: (1, "c0"), 4: (3, "c0"), 7: (3, "before"), 8: (3, "before"), 9: (3, "before")}
    assert ch.expected("walk_middle")[2]["dr"].tolist() == [29, 30, 29, 29, 29]       # (only the window at row 20 000 lies under the long read)


def test_walk_shift_keeps_int64_columns():
    st, _ = ch.table("walk_shift")
    base, _ = ch.table("walk_span")
    assert np.array_equal(st.r_start - ch.WALK_SHIFT, base.r_start) and st.r_start.min() > 1 << 33
    assert "r_start" not in (st.with_narrow().narrow or {}) and "a" not in (st.with_narrow().narrow or {})
    assert ch.expected("walk_shift")[2]["dr"].tolist() == ch.expected("walk_span")[2]["dr"].tolist()


def test_block_table_takes_the_second_bfirst_load():
    st, facts = ch.table("block")
    b = st.chroms.index("b")
    r0, r1 = int(st.reads_off[b]), int(st.reads_off[b + 1])
    assert r1 - r0 == 128 * 4096 + 65 and r0 == 100 and (r1 - 1) >> 12 == 128
    assert int(st.r_start[128 << 12]) == facts["first128"] and st.r_start[(128 << 12) - 1] < facts["first128"] - 1
    by_L = {wins[0][0] >> 1: wk for _, _, wins, _, wk in _calls("block")}
    assert sorted(wk["ktop"] for wk in by_L.values()) == [0, 126, 127, 127, 128, 128]
    assert by_L[facts["first128"]]["ktop"] == 128 and by_L[facts["first128"] - 1]["ktop"] == 127
    assert all(wk["iters1"] == (2 if wk["ktop"] >= 127 else 1) for wk in by_L.values())


def test_seam_table_neighbours_span_every_window():
    st, _ = ch.table("seam")
    assert np.diff(st.reads_off).tolist() == list(ch.SEAM_SIZES)
    hb, want, brute = ch.expected("seam")
    calls = ch.genotyped_calls(ch.PARAMS, hb.segments, want)
    assert sorted(set(c[1] for c in calls)) == list(range(1, 8))          # the chromosome without reads yields no call (INDEL:443-444)
    leaks = 0
    for i, (c, chrom, wins, ) in enumerate(calls):
        pos = int(want["search_pos"][c])
        if pos in (150, ch.SEAM_END + 500):
            assert brute["dr"][i] == 0
            continue
        # the same window over the chromosome's rows AND the 40 rows on either side of it: what a leaking row test would count
        lo, hi = max(int(st.reads_off[chrom]) - 40, 0), min(int(st.reads_off[chrom + 1]) + 40, st.n_reads)
        L2, R2 = wins[0]
        m = (st.r_primary[lo:hi] == 1) & (2 * st.r_start[lo:hi] <= L2) & (2 * st.r_end[lo:hi] >= R2)
        wide = len(np.unique(st.r_id[lo:hi][m]))
        assert wide >= len(brute["cover"][i][0]) > 0, (chrom, pos)
        if pos == ch.SEAM_HI or chrom < 7:                 # (the last chromosome has no successor whose first rows span its low windows)
            assert wide > len(brute["cover"][i][0]), (chrom, pos)
            leaks += 1
    assert leaks == 7 + 6 * 2


def test_tie_table_runs_cross_chunk_and_block_boundaries():
    st, facts = ch.table("tie")
    u = st.chroms.index("u")
    row, L = facts["run_row"], facts["run_L"]
    assert (st.r_start[row:row + 5000] == L).all() and st.r_start[row - 1] < L < st.r_start[row + 5000] and row >= st.reads_off[u]
    k = (row >> 12) + 1
    assert row % 4096 == 4000 and st.r_start[k << 12] == st.r_start[(k + 1) << 12] == L      # equal first starts in consecutive blocks
    t = st.chroms.index("t")
    run = np.flatnonzero(st.r_start == 500_000 - ch.BIAS)
    assert len(run) == 300 and (run >= st.reads_off[t]).all() and (run < st.reads_off[t + 1]).all() and (run[-1] >> 6) - (run[0] >> 6) >= 4
    assert _dr_at("tie", "t", 100_000) == 4 and _dr_at("tie", "t", 200_000) == 4 and _dr_at("tie", "t", 600_000) == facts["dr_600k"]
    assert _dr_at("tie", "t", 500_000) == 200 + 33 and _dr_at("tie", "u", 700_000) == 3333
    # x.5 bounds: four of the nine reads at each breakpoint
    hb, want, brute = ch.expected("tie")
    pair = [i for i, c in enumerate(brute["call"]) if len(brute["cover"][i]) == 2]
    assert len(pair) == 2 and all([len(x) for x in brute["cover"][i]] == [4, 4] for i in pair)
    wins = [w for c in ch.genotyped_calls(ch.PARAMS, hb.segments, want) if len(c[2]) == 2 for w in c[2]]
    assert len(wins) == 4 and all(l % 2 == 1 and r % 2 == 1 for l, r in wins)


def test_edge_table_sits_on_the_int32_limits():
    st, _ = ch.table("edge")
    nw = st.with_narrow().narrow
    assert nw["r_start"].dtype == np.int32 and nw["a"].dtype == np.int32 and int(st.r_end.max()) == ch.INT32_MAX and int(st.r_start.min()) == 0
    e = st.chroms.index("e")
    assert ch.device_maxlen(st, e) == ch.INT32_MAX
    calls = {pos: (wins, wk) for _, _, wins, pos, wk in _calls("edge")}
    assert calls[60][0][0] == (0, 320) and _dr_at("edge", "e", 60) == 41                      # L clamped to 0: the 40 reads from 0 that reach 160 (+ the long one)
    assert calls[ch.INT32_MAX - 49][0][0][1] > 2 * ch.INT32_MAX and _dr_at("edge", "e", ch.INT32_MAX - 49) == 0
    assert calls[ch.INT32_MAX - ch.INS_HALF][0][0][1] == 2 * ch.INT32_MAX and _dr_at("edge", "e", ch.INT32_MAX - ch.INS_HALF) == 101
    # R - maxlen is far below zero for every window that lies inside the int32 range
    assert all(wk["closed"] == "c0" and wins[0][1] - 2 * ch.INT32_MAX < -100_000 for pos, (wins, wk) in calls.items() if pos not in (ch.INT32_MAX - 49, ch.INT32_MAX - ch.INS_HALF))


def _tier_classes(name):
    """the deterministic part of the route: totals (distinct supports + cover) per pile call, the calls that must / may leave the
    first pass and the 8 192-slot table, and the calls whose table does not fit a wavefront's slice of the pool"""
    st, _ = ch.table(name)
    hb, want, brute = ch.expected(name)
    calls = ch.genotyped_calls(ch.PARAMS, hb.segments, want)
    total = brute["dr"] + brute["dv"]
    fits = np.array([ch.fits_slice(st, hb, chrom, wins, int(brute["dv"][i])) for i, (c, chrom, wins) in enumerate(calls)])
    return st, hb, total, fits


def test_tier_table_sizes_and_routes():
    st, hb, total, fits = _tier_classes("tier")
    big = st.chroms.index("big")
    r0, r1 = int(st.reads_off[big]), int(st.reads_off[big + 1])
    assert r1 - r0 == ch.TIER_N and r0 == 100 and ((r1 - 1) >> 12) - (r0 >> 12) + 1 == 513
    assert ch.pool_ints(st, hb) == 1 << 24 and ch.pool_ints(st, hb) // ch.GT2_WAVES == 16384
    assert ch.device_maxlen(st, big) == 3000
    assert sorted(total.tolist()) == [20] * 4 + sorted(ch.TIER_TOTALS)
    # a pile of 20 000 needs the whole pool; the calls of 6 145 and 7 000 leave the 8 192-slot table and fit a slice
    assert (~fits).sum() == 1 and total[~fits].tolist() == [20000] and ((total > 6144) & fits).sum() == 2
    far = [wk for _, _, _, pos, wk in _calls("tier") if pos > 1_000_000]
    assert [wk["ktop"] for wk in far] == [255, 256, 257, 512] and [wk["iters1"] for wk in far] == [3, 3, 3, 5]
    # the cut table: the same piles, a pool of 2^20 ints, and no deep call fits a slice of 1 024
    cst, chb, ctotal, cfits = _tier_classes("tier_cut")
    assert cst.n_reads == 100 + ch.TIER_CUT and ch.pool_ints(cst, chb) == 1 << 20
    assert ctotal.tolist() == total[:10].tolist() and not cfits[ctotal > 704].any()
    assert ch.expected("tier_cut")[2]["dr"].tolist() == ch.expected("tier")[2]["dr"][:10].tolist()


@pytest.mark.parametrize("name", ch.ALL)
def test_extraction_order_is_a_permutation_of_disjoint_runs(name):
    """the third way of every GPU test: with CSV_READS_GAP at half a task region the reads-order stage cuts the table into runs
    that do not interleave and moves them (mode 1), so that the gather builds cfirst / cmax / bfirst from moved runs; with the
    production gap of 1 Mbp these small regions would be glued and the batch repeated through the general sort.  Starts at or
    above 2^32 do not fit the plan's 32-bit run records: the shifted walk table takes the general sort whatever the gap."""
    st, _ = ch.table(name)
    runs, gap = ch.in_extraction_order(st)
    assert not np.array_equal(runs.r_start, st.r_start) and np.array_equal(np.sort(runs.r_start), np.sort(st.r_start))
    plan = ch.run_plan(runs, gap)
    if name == "walk_shift":
        assert not plan["ok"] and plan["why"] == "a run boundary outside [0, 2^32)"
    else:
        assert plan["ok"] and plan["moved"] and plan["runs"] >= 5, plan
    if name != "walk_shift":
        sorted_plan = ch.run_plan(st, gap)                  # (the start-sorted table: runs cut by the gap alone, none moves)
        assert sorted_plan["ok"] and not sorted_plan["moved"]


# ------------------------------------------------------------------------------------------------ GPU
def _three_ways(ctx, monkeypatch, name, narrow=np.int32, capfd=None):
    """the table as int64 columns, as page-locked columns (int32 where they fit) and in extraction order: every result equals
    the oracle's, every genotyped call's dr / dv / gl_idx the brute force's -> {way: (gt_over, gt_huge)} when capfd is given"""
    st, facts = ch.table(name)
    hb0, want, brute = ch.expected(name)
    runs, gap = ch.in_extraction_order(st)
    plan = ch.run_plan(runs, gap)
    routes = {}
    for way, s, dtype in (("int64", st, np.int64), ("pinned", st.pinned(), narrow), ("extraction", runs, np.int64)):
        hb = s.host_batch(s.tasks(), ch.PARAMS)
        assert hb.r_start.dtype == dtype and hb.a.dtype == dtype, way
        if capfd is not None:
            capfd.readouterr()
        if way == "extraction":
            monkeypatch.setenv("CSV_READS_GAP", str(gap))           # (read at every upload: the gap that goes with these task regions)
        got = ctx.cluster_batch(hb, per_sig=True).trimmed()
        if way == "extraction":
            monkeypatch.delenv("CSV_READS_GAP")
            # ordered by moving whole runs, not by the general sort (which is all a table above 2^32 can take)
            assert ctx.last_reads_mode() == (1 if plan["ok"] else 2) and plan["ok"] == (name != "walk_shift"), (name, plan)
        if capfd is not None:
            m = re.findall(r"\[csv\] counters: .* gt_over (\d+) gt_huge (\d+)", capfd.readouterr().err)
            assert m, "no counters line on stderr"
            routes[way] = (int(m[-1][0]), int(m[-1][1]))
        assert len(got["bp1"]) >= facts["placed"]
        assert_soa_equal(got, want, store=st)
        ch.assert_brute_equal(brute, got)
    return routes


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["walk_span", "walk_middle", "walk_nonprimary", "block", "seam", "tie", "edge"])
def test_crafted_tables_three_ways(ctx, monkeypatch, name):
    """(a) the walk of step (2), (b) step (1) beyond 128 blocks, (c) seams, (d) ties, (f) the int32 limits"""
    _three_ways(ctx, monkeypatch, name)


@pytest.mark.gpu
def test_walk_table_above_2_to_33(ctx, monkeypatch):
    """(f) the table of (a) shifted by 2^33 + 12 345: the page-locked store keeps int64 columns, DR is that of the unshifted table"""
    _three_ways(ctx, monkeypatch, "walk_shift", narrow=np.int64)
    assert ch.expected("walk_shift")[2]["dr"].tolist() == ch.expected("walk_span")[2]["dr"].tolist()


@pytest.mark.gpu
def test_tiers_and_their_routes(ctx, monkeypatch, capfd):
    """(e) calls of 640 ... 20 000 distinct supports + cover on a chromosome of 2.1 M reads: LDS 1 024, LDS 8 192, a wavefront's
    slice of the pool (16 384 ints) and the whole pool, the route read from the counters line; then the same calls on the table
    cut to 60 000 reads, where a slice holds 1 024 ints and every deep call takes the whole pool"""
    monkeypatch.setenv("CSV_DEBUG_COUNTERS", "1")
    _, _, total, fits = _tier_classes("tier")
    routes = _three_ways(ctx, monkeypatch, "tier", capfd=capfd)
    for way, (over, huge) in routes.items():
        assert (total > 768).sum() <= over <= (total > 704).sum(), (way, over)
        assert huge == (~fits & (total > 6144)).sum() == 1, (way, huge)
        assert ((total > 6144) & fits).sum() == 2                   # 6 145 and 7 000 left the 8 192 table and are not in gt_huge: the slice path
    _, _, ctotal, cfits = _tier_classes("tier_cut")
    cut_routes = _three_ways(ctx, monkeypatch, "tier_cut", capfd=capfd)
    print("(gt_over, gt_huge) per way - 2.1 M reads: %s; cut to 60 000 reads: %s" % (routes, cut_routes))
    for way, (over, huge) in cut_routes.items():
        assert (ctotal > 768).sum() <= over <= (ctotal > 704).sum(), (way, over)
        assert not cfits[ctotal > 6080].any() and (ctotal > 6144).sum() <= huge <= (ctotal > 6080).sum(), (way, huge)
