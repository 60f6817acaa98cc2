"""Crafted reads tables for TRA genotyping over the reads table (k_genotype_tra: Params.genotype_tra, CUTESV_AMD_TRA_GT=reads_table),
every set tier.

CPU tests (no marker): the sequential brute force against the C oracle, against aln.tra_genotype_host and against the reference's
own call_gt (golden/tra_edges.json.gz); the geometry every table claims (the lane that ends a step, the exit, the search rounds,
the set fill, the tier), asserted from a CPU model of the kernel's route; the mutations each table catches.
GPU tests (-m gpu): every table as int64 columns, as page-locked int32 columns and in extraction order, integer equality on dr /
dv / gl_idx against the oracle and the brute force; the tier from the CSV_DEBUG_COUNTERS line; a resident batch run twice; the
refusal of a mate chromosome outside the table."""
import re

import numpy as np
import pytest

from cutesv_amd import _abi, engine
from cutesv_amd.genotype import gl_fields, gl_index
from helpers import assert_soa_equal, load_json

import cover_helpers as ch
import tra_table_helpers as th


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


def _genotyped(name):
    st, T, G = th.table(name)
    hb, want, brute = th.expected(name)
    return [k for k in th.tra_calls(st, hb.segments, want) if k["genotyped"]]


@pytest.fixture(scope="module")
def routes():
    """{table: [(tier, model)] of its genotyped TRA calls}, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            st, T, G = th.table(name)
            hb, _, _ = th.expected(name)
            cache[name] = [th.route(st, hb, k, G) for k in _genotyped(name)]
        return cache[name]
    return get


# ------------------------------------------------------------------------------------------------ CPU: the yardsticks agree
@pytest.mark.parametrize("name", th.ALL)
def test_brute_force_equals_oracle_twin_and_model(name, routes):
    """the sequential walk == the C oracle's dr / dv / gl_idx (and its -1 rows) on every genotyped TRA call; == aln.tra_genotype_host;
    == the step-by-step model of the kernel in the tier the call takes"""
    st, T, G = th.table(name)
    hb, want, brute = th.expected(name)
    calls = _genotyped(name)
    assert len(brute["call"]) == len(calls) == len(T.claims) > 0
    ch.assert_brute_equal(brute, want)
    assert ((brute["status"] == -1) == (brute["dr"] == -1)).all() and ((brute["dr"] == -1) == (brute["gl_idx"] == -1)).all()
    dr, status = th.twin(st, hb.segments, want, G)
    assert dr.tolist() == brute["dr"].tolist() and status.tolist() == brute["status"].tolist()
    model = routes(name)
    assert [m["dr"] for _, m in model] == brute["dr"].tolist() and [m["status"] for _, m in model] == brute["status"].tolist()
    # calls of a segment that is not genotyped keep what a batch without genotyping gives them
    off = [k["c"] for k in th.tra_calls(st, hb.segments, want) if not k["genotyped"]]
    assert len(off) == (2 if T.ungenotyped else 0)
    assert all((int(want["dr"][c]), int(want["dv"][c]), int(want["gl_idx"][c])) == (-1, -1, -1) for c in off)


def test_brute_force_equals_the_reference_call_gt():
    """golden/tra_edges.json.gz: the reference's own call_gt on the step, name and edge tables (make_golden_tra_edges.py).  The
    recorded rows and calls are the builders', the recorded answers the brute force's."""
    cases = load_json("tra_edges.json.gz")
    assert [c["table"] for c in cases] == list(th.RECORDED)
    n, seen, raised = 0, set(), 0
    for case in cases:
        st, T, G = th.table(case["table"])
        hb, want, brute = th.expected(case["table"])
        assert (case["gt_round"], case["bias"], case["chroms"], case["contig_len"], case["reads_off"]) == (G, th.BIAS, st.chroms, st.contig_len.tolist(), st.reads_off.tolist())
        for col, key in ((st.r_start, "start"), (st.r_end, "end"), (st.r_primary, "primary"), (st.r_id, "id")):
            assert col.tolist() == case[key], (case["table"], key)
        calls = _genotyped(case["table"])
        assert [[k["chr1"], k["bp1"], k["chr2"], k["bp2"], k["sup"]] for k in calls] == case["calls"]
        for i, (k, r) in enumerate(zip(calls, case["answers"])):
            if r == "raises":                                  # fetch(start > stop): the build walks window 2 (as for start == stop)
                s, e = th.window(st, k["chr1"], k["bp1"])
                assert s > e and brute["status"][i] == 0
                raised += 1
                continue
            dv, d = int(brute["dv"][i]), int(brute["dr"][i])
            assert int(r[0]) == dv
            if r[1] == ".":
                assert d == -1 and brute["status"][i] == -1 and r[2:] == ["./.", ".,.,.", ".", "."]
            else:
                assert int(r[1]) == d and brute["status"][i] != -1 and list(gl_fields(gl_index(d, dv))) == r[2:], (case["table"], i)
            seen.add(int(brute["status"][i]))
            n += 1
    assert n > 80 and seen == {0, 1, -1} and raised == 3


# ------------------------------------------------------------------------------------------------ CPU: the geometry each table claims
def _check_claim(name, claim, call, tier, m):
    st, T, G = th.table(name)
    w1, w2 = m["w1"], m["w2"]
    assert len(set(call["sup"])) == claim["dv"]
    for key in ("status", "dr"):
        if key in claim:
            assert m[key] == claim[key], (name, key, claim, m[key])
    if "stop1" in claim:
        kind, row = claim["stop1"]
        r0 = w1["r0"]
        assert w1["lo"] == r0, "the long row does not pin the walk to the chromosome's first row"
        assert w1["stop"] == (kind, r0 + row), (name, claim, w1["stop"])
        if "lane" in claim:
            assert (w1["stop"][1] - w1["lo"]) % 64 == claim["lane"]
        assert len(w1["fills"]) - 1 == row // 64               # the step that ends the walk
        if claim.get("last"):
            assert w1["stop"][1] == w1["hi"] - 1
        elif "lane" in claim:
            # rows behind the stop that span and carry names of their own
            rows = th.rows_of(st, call["chr1"])
            behind = [rows[i] for i in range(row + 1, min(row + 21, w1["hi"] - r0))]
            assert sum(1 for a, b, p, _ in behind if p == 1 and a < w1["s"] and b > w1["e"]) >= 5
        if "other" in claim:
            okind, orow = claim["other"]
            assert w1["firsts"][okind] == r0 + orow and (orow // 64 == row // 64) and orow > row
    if "ratio" in claim:
        p, it = claim["ratio"]
        rows = th.rows_of(st, call["chr1"])
        got = [r for r in rows[:w1["stop"][1] - w1["r0"] + 1] if r[0] < w1["e"] and r[1] > w1["s"]]
        assert (sum(r[2] for r in got), len(got)) == (p, it) and it >= G and it % 5 == 0
    if "steps1" in claim:                                     # the steps of window 1 that hold spanning rows
        rows = th.rows_of(st, call["chr1"])
        span = [i for i in range(w1["lo"] - w1["r0"], w1["hi"] - w1["r0"]) if rows[i][2] == 1 and rows[i][0] < w1["s"] and rows[i][1] > w1["e"]]
        assert w1["lo"] == w1["r0"] and len(set(i // 64 for i in span)) == claim["steps1"] and len(w1["fills"]) == (w1["hi"] - w1["lo"] + 63) // 64
    for key, w in (("walked1", w1), ("walked2", w2)):
        if key in claim:
            assert w is not None and w["walked"] == claim[key], (name, key, claim)
    if "win1" in claim:
        assert (w1["s"], w1["e"]) == claim["win1"]
    if "w2" in claim:
        assert w2 is None
    if "fetched1" in claim:
        rows = th.rows_of(st, call["chr1"])
        assert sum(1 for r in rows if r[0] < w1["e"] and r[1] > w1["s"]) == claim["fetched1"]
    if "tier" in claim:
        assert tier == claim["tier"], (name, claim, tier)
    if "bits" in claim:
        assert th.tra_bits_for(m["ns"]) == claim["bits"]
    if claim.get("last_fill"):
        assert w1["fills"][-1] == claim["last_fill"] and claim["last_fill"] + 64 == th.TG_LIMIT and len(w1["fills"]) == (w1["hi"] - w1["lo"] + 63) // 64


@pytest.mark.parametrize("name", [n for n in th.ALL if not n.startswith("edges_r")])
def test_every_table_holds_the_geometry_it_claims(name, routes):
    """the lane and the exit that end a walk, the steps, the windows after the clamp, the tier: from the model of the route"""
    claims = th.claimed(name)
    by_c = {k["c"]: r for k, r in zip(_genotyped(name), routes(name))}
    assert len(claims) == len(by_c)
    for claim, call in claims:
        tier, m = by_c[call["c"]]
        _check_claim(name, claim, call, tier, m)
        if "tier" not in claim:
            assert tier == "lds"


def test_step_tables_stop_where_they_say(routes):
    """over the gt_round values: exit B on lane 63, on lane 0 of the next step, on the window's last row and on lane 10; exit A
    likewise where gt_round lets it (64 and above); the ratio rule on either side of a fifth"""
    for G in th.STEP_ROUNDS:
        claims = th.claimed("steps_r%d" % G)
        stops = [(c["stop1"][0], c.get("lane"), bool(c.get("last"))) for c, _ in claims if "ratio" not in c]
        want = [("B", 63, False), ("B", 0, False), ("B", None, True), ("B", 10, False)]
        if G >= 64:
            want = [("A", 63, False), ("A", 0, False), ("A", None, True), ("A", 10, False)] + want
        assert [(k, None if last else lane, last) for k, lane, last in stops] == want, G
        ratios = sorted((5 * c["ratio"][0] - c["ratio"][1], c["status"]) for c, _ in claims if "ratio" in c)
        assert ratios == ([(-5, 1)] if G > 5 else []) + [(0, 1), (5, -1)], G
    # both exits in one step
    (a, _), (b, _) = th.claimed("ab")
    assert (a["stop1"][0], a["other"][0], a["status"]) == ("A", "B", 1) and (b["stop1"][0], b["other"][0], b["status"]) == ("B", "A", -1)


def test_edge_tables_by_gt_round():
    """the edge table at gt_round 500, 10 and 4: the same rows, another status"""
    by = {}
    for name in ("edges", "edges_r10", "edges_r4"):
        hb, want, brute = th.expected(name)
        by[name] = {(k["chr1"], k["bp1"], k["code"]): (int(brute["dr"][i]), int(brute["status"][i])) for i, k in enumerate(_genotyped(name))}
    st, T, _ = th.table("edges")
    g, e = st.chroms.index("g"), st.chroms.index("e")
    # nine secondaries and one primary: ten fetched rows, a tenth of them primary
    assert by["edges"][(g, 80_000, 0)] == (7, 0) and by["edges_r10"][(g, 80_000, 0)] == (1, 1) and by["edges_r4"][(g, 80_000, 0)] == (1, 1)
    # the window edges: the fourth fetched row is a secondary, the fifth the third primary
    assert by["edges"][(e, 20_000, 0)] == (2, 0) and by["edges_r10"][(e, 20_000, 0)] == (2, 0) and by["edges_r4"][(e, 20_000, 0)] == (-1, -1)
    # 30 primary rows from 0 on: none spans; gt_round 10 ends the call at the tenth with status -1
    assert by["edges"][(e, 300, 0)] == (0, 0) and by["edges_r10"][(e, 300, 0)] == (-1, -1)


def test_search_table_takes_every_round_count(routes):
    """both 64-ary searches return the partition points of a plain scan; the first search runs 0, 1, 2 and 3 rounds over the
    block sizes, the second follows the window's row"""
    st, T, G = th.table("search")
    claims = th.claimed("search")
    by_c = {k["c"]: r for k, r in zip(_genotyped("search"), routes("search"))}
    first, second = {}, set()
    for claim, call in claims:
        n, row = claim["search"]
        w = by_c[call["c"]][1]["w1"]
        r0, r1 = int(st.reads_off[call["chr1"]]), int(st.reads_off[call["chr1"] + 1])
        start = st.r_start[r0:r1]
        assert r1 - r0 == n and ch.device_maxlen(st, call["chr1"]) == 3000
        assert w["hi"] == r0 + int((start < w["e"]).sum()) and w["lo"] == r0 + int((start + 3000 <= w["s"]).sum())
        assert w["lo"] <= r0 + row < w["hi"]
        first.setdefault(n, set()).add(w["rounds"][0])
        second.add(w["rounds"][1])
    assert {n: sorted(v) for n, v in first.items()} == {1: [0], 64: [0], 65: [1], 4096: [1], 4097: [1], 4160: [1], 4161: [1, 2], 262_145: [2], 266_304: [2], 266_305: [2, 3]}      # (the last probe block is the short one)
    assert second == {0, 1, 2}


def test_scan_tables_put_the_calls_where_they_say():
    hb, want, brute = th.expected("scan128")
    assert len(want["bp1"]) == 128 and brute["call"].tolist() == list(range(63, 126))
    st, T, _ = th.table("scan128")
    kinds = [int(hb.segments[int(s)]["svtype"]) for s in want["call_seg"][:63]]
    assert kinds == [_abi.DEL] * 60 + [_abi.INS] * 3 and (want["dr"][:60] > 0).any()
    assert [k["c"] for k in th.tra_calls(st, hb.segments, want) if not k["genotyped"]] == [126, 127]
    # (the windows of the two calls that are not genotyped hold spanning reads: genotyped they would get dr 1 and 2)
    hb, want, brute = th.expected("scan_far")
    assert len(want["bp1"]) % 64 != 0 and brute["call"].tolist() == [16_400, 16_401, 16_402] and brute["call"].min() >= 64 * th.TRA_GRID
    assert brute["dr"].tolist() == [1, 2, 3]


def test_tier_tables_take_the_tier_they_say(routes):
    tiers = {name: sorted(t for t, _ in routes(name) if t != "lds") for name in th.TIERS}
    assert tiers == {"lds_full": [], "lds_over": ["huge"], "huge1": ["huge"], "huge2": ["huge", "huge"], "slice": ["huge", "slice"]}
    for name in th.TIERS:
        st, T, G = th.table(name)
        hb, _, _ = th.expected(name)
        assert th.pool_ints(st, hb) == (1 << 22 if name == "slice" else 1 << 20)
    # the deep calls: 502 and more supports can fill the 4096-slot set before exit A (6 ns - 1 >= 3009); 13 bits up to 529 supports
    assert th.tra_bits_for(529) == 13 and th.tra_bits_for(530) == 14 and 6 * 502 - 1 >= th.TG_LIMIT - 63 > 6 * 501 - 1
    st, T, G = th.table("slice")
    seg = {t: st.seg_index[t] for t in st.seg_index if t[0] == "TRA"}
    assert max(b - a for a, b in seg.values()) == 32_700 > 32_640


@pytest.mark.parametrize("name", th.ALL)
def test_extraction_order_is_a_permutation_the_stage_can_undo(name):
    """the third way of every GPU test (cover_helpers.in_extraction_order): the rows dealt to three workers by task region.  The
    starts of a chromosome are distinct, so the start order of the table - and with it the walk - is the same whatever the order
    the rows arrive in"""
    st, _, _ = th.table(name)
    runs, gap = ch.in_extraction_order(st)
    assert not np.array_equal(runs.r_start, st.r_start) and np.array_equal(np.sort(runs.r_start), np.sort(st.r_start))
    for c in range(len(st.chroms)):
        r0, r1 = int(st.reads_off[c]), int(st.reads_off[c + 1])
        assert (np.diff(st.r_start[r0:r1]) > 0).all()
        o = np.argsort(runs.r_start[r0:r1], kind="stable")
        for col in ("r_start", "r_end", "r_primary", "r_id"):
            assert np.array_equal(getattr(runs, col)[r0:r1][o], getattr(st, col)[r0:r1]), (name, c, col)


# ------------------------------------------------------------------------------------------------ CPU: a test must be able to fail
MUTATIONS = ("behind", "nodup", "ratio", "edge_le", "floorstep", "fill_ge")
SCAN_MUTATIONS = ("lane63", "one_round", "full_rounds", "any_tra")


def _caught(name, mutate):
    """the mutated model gives another dr somewhere, or leaves the LDS set where the model does not"""
    st, T, G = th.table(name)
    hb, want, brute = th.expected(name)
    calls = _genotyped(name)
    if mutate in SCAN_MUTATIONS:
        assert th.scan_visits(hb.segments, want) == [k["c"] for k in calls]
        return th.scan_visits(hb.segments, want, mutate) != [k["c"] for k in calls]
    got = [th.model_call(st, k, G, limit=1 << 30, mutate=mutate) for k in calls]
    over = [th.model_call(st, k, G, mutate=m)["overflow"] for k in calls for m in (None, mutate)]
    return [m["dr"] for m in got] != brute["dr"].tolist() or over[0::2] != over[1::2]


CATCHES = {
    "ab": ("behind", "floorstep"), "names": ("behind", "nodup", "floorstep"),
    "edges": ("behind", "edge_le"), "edges_r10": ("edge_le",), "edges_r4": ("behind",),
    "search": ("floorstep",),
    "scan128": ("floorstep", "lane63", "any_tra"), "scan_far": ("floorstep", "one_round", "full_rounds"),
    "lds_full": ("fill_ge",), "lds_over": ("floorstep",), "huge1": ("behind",), "huge2": ("behind", "floorstep"), "slice": ("behind", "floorstep"),
}
CATCHES.update({"steps_r%d" % G: ("behind", "ratio", "edge_le") + (("floorstep",) if G < 12 else ()) for G in th.STEP_ROUNDS})


def test_mutated_rules_are_caught():
    """a GPU test must be able to fail: the kernel's rules, each broken in the CPU model - lanes behind the stop committed, no
    in-step duplicate rule, `<` for `<=` in the ratio, `<=` for `<` at a window edge, a probe stride rounded down, a step given up
    at filled + 64 == limit, and four ways to lose a call in the scan.  Every table catches at least one; every mutation is caught;
    the sequential walk with the mutated ratio differs from the oracle too"""
    # (the scan mutations are asked of the scan tables only: a table of fewer than 64 calls meets them by being small)
    catches = {name: tuple(m for m in MUTATIONS + (SCAN_MUTATIONS if name.startswith("scan") else ()) if _caught(name, m)) for name in th.ALL}
    assert catches == CATCHES, catches
    assert all(catches.values()) and set(m for v in catches.values() for m in v) == set(MUTATIONS + SCAN_MUTATIONS)
    for G in th.STEP_ROUNDS:
        name = "steps_r%d" % G
        st, T, _ = th.table(name)
        hb, want, brute = th.expected(name)
        assert th.brute(st, hb.segments, want, G, ratio_lt=True)["dr"].tolist() != brute["dr"].tolist()


# ------------------------------------------------------------------------------------------------ GPU
def _counters(err):
    m = re.findall(r"(\[csv\] counters: .* error (\d+) \|.* gt_huge (\d+) tra_huge (\d+))", err)
    assert m, "no counters line on stderr"
    print(m[-1][0])
    return int(m[-1][1]), int(m[-1][3])


def _three_ways(ctx, monkeypatch, name, capfd=None):
    """the table as int64 columns, as page-locked int32 columns and in extraction order: every result equals the oracle's, every
    genotyped TRA call's dr / dv / gl_idx the brute force's -> {way: (error, tra_huge)} when capfd is given"""
    st, T, G = th.table(name)
    hb0, want, brute = th.expected(name)
    runs, gap = ch.in_extraction_order(st)
    plan = ch.run_plan(runs, gap)
    out = {}
    for way, s, dtype in (("int64", st, np.int64), ("pinned", st.pinned(), np.int32), ("extraction", runs, np.int64)):
        hb = th.host_batch(s, T, G)
        assert hb.r_start.dtype == dtype and hb.a.dtype == dtype, way
        if capfd is not None:
            capfd.readouterr()
        if way == "extraction":
            monkeypatch.setenv("CSV_READS_GAP", str(gap))
        got = ctx.cluster_batch(hb, per_sig=True).trimmed()
        if way == "extraction":
            monkeypatch.delenv("CSV_READS_GAP")
            assert ctx.last_reads_mode() == (1 if plan["ok"] else 2), (name, plan)
        if capfd is not None:
            out[way] = _counters(capfd.readouterr().err)
        assert_soa_equal(got, want, store=st)
        ch.assert_brute_equal(brute, got)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in th.ALL if n not in th.TIERS])
def test_crafted_tables_three_ways(ctx, monkeypatch, name):
    """steps, names, edges, search and scan: both table forms and the reads-order stage"""
    _three_ways(ctx, monkeypatch, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", th.TIERS)
def test_tiers_and_their_routes(ctx, monkeypatch, capfd, routes, name):
    """the set in LDS up to its last step, in a workgroup's slice of the pool and in the whole pool: tra_huge of the counters line
    is the number of calls the model sends to the whole pool; no error bit"""
    monkeypatch.setenv("CSV_DEBUG_COUNTERS", "1")
    huge = sum(t == "huge" for t, _ in routes(name))
    got = _three_ways(ctx, monkeypatch, name, capfd=capfd)
    print("%s: (error, tra_huge) per way %s" % (name, got))
    assert got == {way: (0, huge) for way in ("int64", "pinned", "extraction")}


@pytest.mark.gpu
def test_resident_huge_table_runs_twice(ctx, monkeypatch, capfd):
    """upload once, run twice: the same rows and the same tra_huge (the ticket and the counter are per run)"""
    monkeypatch.setenv("CSV_DEBUG_COUNTERS", "1")
    st, T, G = th.table("huge2")
    hb0, want, brute = th.expected("huge2")
    hb = th.host_batch(st.pinned(), T, G)
    ctx.upload(hb, per_sig=True)
    for k in range(2):
        capfd.readouterr()
        ctx.run()
        got = ctx.download(per_sig=True).trimmed()
        assert _counters(capfd.readouterr().err) == (0, 2), k
        assert_soa_equal(got, want, store=st)
        ch.assert_brute_equal(brute, got)


@pytest.mark.gpu
def test_mate_chromosome_outside_the_table_is_refused(ctx):
    """the public entry lets the signature through (csv_batch_upload does not read aux); k_genotype_tra raises ERR_TRA_CHROM and the
    download refuses the result.  The context then runs the untouched batch"""
    st, T, G = th.table("names")
    hb0, want, brute = th.expected("names")
    n_chrom = len(st.chroms)
    for bad in (n_chrom, -1):
        s = st.pinned() if bad < 0 else st
        hb = th.host_batch(s, T, G)
        aux = hb.aux.copy()
        beg, end = st.seg_index[("TRA", "a")]
        aux[beg:end] = np.where(aux[beg:end] >> 3 == st.chroms.index("z"), bad * 8 + (aux[beg:end] & 7), aux[beg:end])
        assert (aux != hb.aux).sum() > 20
        broken = _abi.HostBatch(hb.segments, hb.a, hb.b, hb.read_id, aux, n_chrom=n_chrom, reads_off=hb.reads_off, r_start=hb.r_start, r_end=hb.r_end,
                                r_primary=hb.r_primary, r_id=hb.r_id, contig_len=st.contig_len)
        with pytest.raises(engine.CsvError) as e:
            ctx.cluster_batch(broken, per_sig=True)
        assert e.value.code == _abi.E_INVALID and "mate chromosome" in str(e.value)
        got = ctx.cluster_batch(th.host_batch(st, T, G), per_sig=True).trimmed()
        assert_soa_equal(got, want, store=st)
        ch.assert_brute_equal(brute, got)
