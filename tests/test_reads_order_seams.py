"""The reads-order stage (k_reads_runs, k_reads_plan, k_reads_gather, k_reads_maxlen and the general sort behind them) at its
seams: reads tables laid out in file order so that every capacity, every cut position and every rule of the plan is reached.

CPU tests (no marker): every table claims its geometry from plain numpy on its columns; reads_order_helpers.plan_model - the
stage's verdict restated - says what the case is built for and agrees with cover_helpers.run_plan; and the probes of a layout
can see a misplaced run: every wrongly packed variant changes the covering set of a probe.
GPU tests (-m gpu): every table as int64 and as page-locked columns, one-shot and resident; the stage's own verdict (mode, state,
run count from the CSV_DEBUG_COUNTERS line) against the model, the result bit for bit against the oracle on the start-sorted
table and against the brute force, every probe called.  Integer equality throughout."""
import re
import time

import numpy as np
import pytest

from cutesv_amd import engine
from helpers import assert_soa_equal

import cover_helpers as ch
import reads_order_helpers as ro


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def long_layout():
    """the 8 193-tile table, built once for its CPU and its GPU test; the module's tables (1.5 GB with this one) go when it is done"""
    yield ro.case("long")
    ro.case.cache_clear()
    ro.expected.cache_clear()


# ------------------------------------------------------------------------------------------------ CPU: geometry, from the columns
def _listed(st, gap):
    """rows that start a run and are no block start (plain numpy, not plan_model)"""
    d = np.diff(st.r_start)
    rows = np.flatnonzero((d < 0) | (d > gap)) + 1
    return rows[~np.isin(rows, st.reads_off)]


def _per_tile(st, rows):
    return np.bincount(rows // ro.TILE, minlength=-(-st.n_reads // ro.TILE))


def _dest_runs(lay):
    """run index of every row of the start-ordered table"""
    st = lay.store
    run_of = np.repeat(np.arange(lay.n_runs), [b - a for _, a, b, _ in lay.runs])
    chrom = np.repeat(np.arange(len(st.reads_off) - 1), np.diff(st.reads_off))
    return run_of[np.lexsort((np.arange(st.n_reads), st.r_start, chrom))]


def _geometry(name, lay, facts):
    st, gap = lay.store, lay.gap
    s, off = st.r_start, st.reads_off
    nc = len(off) - 1
    rows = _listed(st, gap)
    tiles = _per_tile(st, rows)
    nonempty = int((np.diff(off) > 0).sum())
    if name.startswith("tile_"):
        k = facts["tile1"]
        assert nc == 1 and st.n_reads == 3 * ro.TILE and tiles[1] == k and tiles.max() == k and k in (ro.TCAP, ro.TCAP + 1)
        in1 = rows[rows // ro.TILE == 1] - ro.TILE
        if "ones" in name:
            # k consecutive rows, each a run of its own, descending; 32 of them fill the last four lanes, eight each
            assert in1.tolist() == list(range(ro.TILE - k, ro.TILE)) and (np.diff(s[ro.TILE + in1]) < 0).all()
            assert rows[-1] == 2 * ro.TILE                                     # the main run resumes on row 0 of tile 2
            assert np.bincount(in1 // 8)[-4:].tolist() == [8] * 4
        else:
            assert np.bincount(in1 // ro.SPAN).tolist() == ([8, 8, 8, 8] if k == 32 else [8, 8, 9, 8])
            assert {0, 7, 8, 511} <= set((in1 % ro.SPAN).tolist()) and 1 in np.diff(in1)      # lane 0 of a wavefront; a run of one row
    elif name.startswith("cut_rows_"):
        n = st.n_reads
        assert rows.tolist() == facts["cuts"] == [512, 1024, 1536, ro.TILE, ro.TILE + 16, ro.TILE + 23, n - 1]
        assert n in (2 * ro.TILE + 1, 2 * ro.TILE + 5, 2 * ro.TILE) and (n % 8 == 0) == (n == 2 * ro.TILE)
        assert (ro.TILE + 16) % 8 == 0 and (ro.TILE + 23) % 8 == 7 and (s[rows] < s[rows - 1]).all()
    elif name.startswith("gap_"):
        assert int(s[3000] - s[2999]) == facts["seam"] == (gap if name == "gap_exact" else gap + 1)
        assert rows.tolist() == ([5000] if name == "gap_exact" else [3000, 5000])
        assert s[2999] < s[5000] and s[-1] < s[3000]                           # the third region belongs between the first two
    elif name.startswith("capacity_"):
        assert len(rows) + nc == facts["total"] and nc == 4000 and nc - nonempty == facts["empties"] and tiles.max() <= ro.TCAP
        assert nc + 1 <= ro.CAP and (not facts["empties"] or len(rows) + nonempty <= ro.CAP)      # only the count WITH the empty blocks decides
    elif name.startswith("sorted_chroms_"):
        assert nc == facts["n_chrom"] and len(rows) == 0 and nonempty == nc and nc + 1 in (ro.CAP, ro.CAP + 1)
        assert all((np.diff(s[off[c]:off[c + 1]]) >= 0).all() for c in (0, nc // 2, nc - 1))
    elif name.startswith("gather_"):
        assert nc == 1 and len(rows) + 1 == facts["runs"] and facts["runs"] in (ro.GA_TAB, ro.GA_TAB + 1) and tiles.max() == ro.TCAP
        assert (s[rows] < s[rows - 1]).all()                                   # every run moves
    elif name.startswith("span_"):
        dest = _dest_runs(lay)
        sizes = np.bincount(dest)[np.unique(dest[ro.SPAN:2 * ro.SPAN])]
        if name == "span_five_runs":
            assert len(sizes) == 5 and (sizes == 1).sum() == 2 and dest[ro.SPAN - 1] != dest[ro.SPAN]
        else:
            assert len(sizes) == 5 and dest[ro.SPAN - 1] == dest[ro.SPAN] and dest[2 * ro.SPAN - 1] == dest[2 * ro.SPAN]        # a run across either end
    elif name.startswith("blocks_"):
        a, b = facts["special"]
        assert nc == facts["n_chrom"] and all(off[c + 1] == off[c] for c in range(0, nc, 10) if c not in (a, b))
        assert len(rows) == 2 and off[a] < rows[0] < off[a + 1] and off[b] < rows[1] < off[b + 1]
        assert np.bincount(off[:-1] // ro.TILE).min() >= 24                    # dozens of block starts in every tile
        assert (b >= ro.RP_THREADS) == (nc > ro.RP_THREADS) and int(np.diff(off).max()) == 70
    elif name.startswith("tie_"):
        r = lay.runs
        f = lambda k: int(s[r[k][1]])
        l = lambda k: int(s[r[k][2] - 1])
        if name == "tie_equal_first_ok":
            assert f(0) == f(2) == l(0) < l(2) < f(1)
        elif name == "tie_equal_first_bad":
            assert (r[0][1], r[0][2], r[1][2]) == (0, 2, 3) and f(0) == f(1) == 50_000 < l(0)
        elif name == "tie_last_is_first_ok":
            assert l(0) == f(2) and f(0) < f(2) < l(2) < f(1)
        else:
            assert l(1) == f(0) and f(1) < f(0)
    elif name == "interleave":
        (_, a0, a1, _), (_, b0, b1, _) = lay.runs[:2]
        assert s[b0] < s[a0] < s[b1 - 1] < s[a1 - 1] and rows.tolist() == [b0, 840]
    elif name.startswith("limit_"):
        assert st.r_start.dtype == np.int64 and "r_start" not in (st.with_narrow().narrow or {})
        if name == "limit_last":
            assert s[-1] >= ro.LIMIT and (s[rows] < ro.LIMIT).all() and (s[rows - 1] < ro.LIMIT).all() and (s[off[:-1]] < ro.LIMIT).all() and (s[off[1:-1] - 1] < ro.LIMIT).all()
        else:
            assert int(s[rows].max()) == facts["top"] == (ro.LIMIT - 1 if name == "limit_cut_below" else ro.LIMIT) and s[-1] < ro.LIMIT
    elif name == "identity":
        assert all((np.diff(s[off[c]:off[c + 1]]) >= 0).all() for c in range(nc)) and len(rows) == 40 and tiles.max() <= ro.TCAP
    elif name.startswith("shuffled_"):
        cbytes = 0
        v = nc - 1
        while v:
            cbytes, v = cbytes + 1, v >> 8
        assert nc == facts["n_chrom"] and cbytes == {256: 1, 257: 2, 65536: 2, 65537: 3}[nc]
        assert sum(bool((np.diff(s[off[c]:off[c + 1]]) < 0).any()) for c in range(nc)) == (nc if nc < 1000 else 3)
    else:
        assert name == "long"
        n_tiles = -(-st.n_reads // ro.TILE)
        per = -(-n_tiles // ro.RP_THREADS)
        assert st.n_reads == ro.LONG_N and n_tiles - 1 == ro.LONG_TILES == 8 * ro.RP_THREADS + 1 and per == 9 and st.n_reads % 8 == 5
        assert rows.tolist() == facts["cuts"] and sorted(set((rows // ro.TILE % per).tolist())) == [3, 6, 8]
        assert [int(t) // per for t in rows // ro.TILE if t % per == 8] == [0, 499, 909] and rows[-1] // ro.TILE == n_tiles - 1
        assert int(st.r_end.max()) < 1 << 31 and int((np.diff(s) == 10).sum()) == st.n_reads - 1 - 6                # evenly spaced but for the six cuts


@pytest.mark.parametrize("name", ro.SMALL)
def test_table_claims_its_geometry_and_the_model_its_verdict(name):
    lay, facts = ro.case(name)
    _geometry(name, lay, facts)
    model = ro.plan_model(lay.store, lay.gap)
    assert (model["state"], model["mode"]) == ro.EXPECT[name], model
    assert model["n_found"] == len(_listed(lay.store, lay.gap))
    if model["state"] != ro.GENERAL:
        assert model["n_runs"] == model["n_found"] + int((np.diff(lay.store.reads_off) > 0).sum())
    assert len(lay.probes) >= 2 and ro.runs_are_disjoint(lay) == (name not in ("tie_equal_first_bad", "tie_last_is_first_bad", "interleave"))
    # the start-sorted table of every case needs no move (and where it fits the plan, the model says so)
    again = ro.plan_model(lay.sorted, lay.gap)
    assert again["state"] != ro.REORDER and (again["state"] == ro.IDENTITY or name.startswith(("limit_", "shuffled_", "capacity_%d" % (ro.CAP + 1), "sorted_chroms_%d" % ro.CAP)))


def test_every_case_has_an_expected_verdict():
    states = [s for s, _ in ro.EXPECT.values()]
    assert set(ro.EXPECT) == set(ro.CASES) and len(ro.CASES) == 37 and states.count(ro.GENERAL) == 15 and states.count(ro.IDENTITY) == 2


@pytest.mark.parametrize("name", ch.ALL)
def test_plan_model_agrees_with_run_plan(name):
    """the tables of the cover suite in extraction order (and start-sorted): both models say the same about each"""
    st, _ = ch.table(name)
    runs, gap = ch.in_extraction_order(st)
    # (run_plan looks at the listed run starts only: it has nothing to say about a start-sorted table that lies above 2^32)
    for table in (runs, st) if name != "walk_shift" else (runs,):
        old, new = ch.run_plan(table, gap), ro.plan_model(table, gap)
        assert old["ok"] == (new["state"] != ro.GENERAL), (old, new)
        if old["ok"]:
            assert old["moved"] == (new["state"] == ro.REORDER) and old["runs"] == new["n_runs"], (old, new)


# ------------------------------------------------------------------------------------------------ CPU: the probes see a misplaced run
def _assert_mutants_seen(name):
    lay, _ = ro.case(name)
    wins = ro.probe_windows(lay)
    if not ro.runs_are_disjoint(lay):
        # (no packing of whole runs is right here; the table as it lies in the file is still wrong)
        as_is = ro.Packing(lay, [(0, lay.store.n_reads)])
        assert ro.seen(lay, as_is)
        return 1
    right = ro.Packing(lay, [lay.runs[r][1:3] for r in ro.sorted_runs(lay)])
    for k, (c, L2, R2) in enumerate(wins):                   # on the rightly packed table the query finds the true cover
        assert np.array_equal(right.cover(c, L2, R2), lay.covers[k])
    muts = ro.mutants(lay)
    unseen = [what for what, first, p in muts if not ro.seen(lay, p, first)]
    assert not unseen, "%d of %d wrongly packed tables change no probe: %s" % (len(unseen), len(muts), unseen[:8])
    return len(muts)


@pytest.mark.parametrize("name", ro.SMALL)
def test_probes_see_every_misplaced_run(name):
    n = _assert_mutants_seen(name)
    lay, _ = ro.case(name)
    moved = ro.plan_model(lay.store, lay.gap)["state"] == ro.REORDER
    probed = sum(1 for r in lay.runs if r[3] >= 0)
    assert n >= (min(probed, 64) if moved else 0)


def test_long_table_geometry_model_and_mutants(long_layout):
    """the 8 193-tile table: its geometry, its verdict and its wrongly packed variants"""
    lay, facts = long_layout
    _geometry("long", lay, facts)
    model = ro.plan_model(lay.store, lay.gap)
    assert (model["state"], model["mode"], model["n_found"], model["n_runs"]) == (ro.REORDER, 1, 6, 7)
    assert _assert_mutants_seen("long") >= 12


# ------------------------------------------------------------------------------------------------ GPU
COUNTERS = re.compile(r"\[csv\] counters: .*\| reads: mode (\d+) runs (\d+) state (\d+) \|")


def _verdict(ctx, capfd, model):
    """the stage's own verdict against the model's: csv_batch_reads_mode and the counters lines of the call"""
    lines = [tuple(int(x) for x in m) for m in COUNTERS.findall(capfd.readouterr().err)]
    assert lines, "no counters line on stderr"
    assert ctx.last_reads_mode() == model["mode"], (lines, model)
    assert lines[0][0] == 1 and lines[0][2] == model["state"], (lines, model)
    if model["state"] != ro.GENERAL:
        assert lines[0][1] == model["n_runs"] and len(lines) == 1, (lines, model)
    else:
        assert len(lines) == 2 and lines[1][0] == 2, (lines, model)


def _called(lay, hb, got):
    calls = set((int(hb.segments[int(sg)]["chrom"]), int(p)) for sg, p in zip(got["call_seg"], got["search_pos"]))
    missing = [(c, pos) for c, pos, _ in lay.probes if (c, pos) not in calls]
    assert not missing and len(got["bp1"]) == len(lay.probes), (missing[:5], len(got["bp1"]), len(lay.probes))


def _check(ctx, monkeypatch, capfd, name):
    lay, _ = ro.case(name)
    model = ro.plan_model(lay.store, lay.gap)
    want, brute = ro.expected(name)
    monkeypatch.setenv("CSV_READS_GAP", str(lay.gap))
    monkeypatch.setenv("CSV_DEBUG_COUNTERS", "1")
    narrow = np.int32 if int(lay.store.r_end.max()) < 1 << 31 else np.int64
    batches = []
    for way, s, dtype in (("int64", lay.store, np.int64), ("pinned", lay.store.pinned(), narrow)):
        hb = s.host_batch(s.tasks(), ch.PARAMS)
        assert hb.r_start.dtype == dtype, way
        batches.append(hb)
        capfd.readouterr()
        got = ctx.cluster_batch(hb, per_sig=True, cap_calls=len(lay.probes) + 8).trimmed()           # (room for every call: one pass, one counters line)
        _verdict(ctx, capfd, model)
        assert_soa_equal(got, want, store=lay.sorted)
        ch.assert_brute_equal(brute, got)
        _called(lay, hb, got)
    # resident: the packed table of the upload is kept across runs, or built again by each
    try:
        for reuse in (1, 0):
            ctx.option(1, reuse)
            ctx.upload(batches[0], per_sig=True)
            ctx.run(); ctx.run()
            got = ctx.download(per_sig=True).trimmed()
            assert ctx.last_reads_mode() == model["mode"], reuse
            assert_soa_equal(got, want, store=lay.sorted)
            ch.assert_brute_equal(brute, got)
    finally:
        ctx.option(1, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ro.SMALL)
def test_crafted_layouts_on_the_device(ctx, monkeypatch, capfd, name):
    _check(ctx, monkeypatch, capfd, name)


@pytest.mark.gpu
def test_a_movable_table_after_a_fallback_is_moved_again(ctx, monkeypatch):
    """resident uploads: a table that took the general sort leaves nothing behind - the next upload, of a table whose runs can be
    moved, reports mode 1, and then the other way round"""
    monkeypatch.setenv("CSV_READS_GAP", str(ro.GAP))
    for name in ("interleave", "gap_plus_1", "tile_slices_33", "tile_slices_32", "limit_last"):
        lay, _ = ro.case(name)
        want, brute = ro.expected(name)
        ctx.upload(lay.store.host_batch(lay.store.tasks(), ch.PARAMS), per_sig=True)
        ctx.run(); ctx.run()
        got = ctx.download(per_sig=True).trimmed()
        assert ctx.last_reads_mode() == ro.EXPECT[name][1], name
        assert_soa_equal(got, want, store=lay.sorted)
        ch.assert_brute_equal(brute, got)


@pytest.mark.gpu
def test_long_table_a_plan_thread_owns_nine_tiles(ctx, monkeypatch, capfd, long_layout):
    """8 193 full tiles and five rows (16 779 269 reads, page-locked int32 columns): the plan's loops beyond a thread's first
    eight tiles.  Judged against the brute force alone: the oracle's sort of 16 M rows takes longer than the test."""
    t0 = time.time()
    lay, _ = long_layout
    model = ro.plan_model(lay.store, lay.gap)
    monkeypatch.setenv("CSV_READS_GAP", str(lay.gap))
    monkeypatch.setenv("CSV_DEBUG_COUNTERS", "1")
    s = lay.store.pinned()
    hb = s.host_batch(s.tasks(), ch.PARAMS)
    assert hb.r_start.dtype == np.int32 and hb.r_end.dtype == np.int32
    t1 = time.time()
    capfd.readouterr()
    got = ctx.cluster_batch(hb, per_sig=True, cap_calls=len(lay.probes) + 8).trimmed()           # (room for every call: one pass, one counters line)
    t2 = time.time()
    _verdict(ctx, capfd, model)
    _called(lay, hb, got)
    brute = ch.brute_dr(lay.store, ch.PARAMS, hb.segments, got)
    assert len(brute["call"]) == len(lay.probes) == 7 and sorted(brute["dr"].tolist()) == sorted(min(3 + k % 5, b - a) for k, (_, a, b, _) in enumerate(lay.runs))
    ch.assert_brute_equal(brute, got)
    print("long table: columns page-locked in %.1f s, the call %.1f ms, checked in %.1f s" % (t1 - t0, 1e3 * (t2 - t1), time.time() - t2))
