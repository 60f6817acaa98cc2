"""The last stage every call passes through - order, emit, publish (k_items_scan, k_emit with emit_item_serial, k_publish) - AT its seams:
1 .. 130 calls from one cluster (the serial path above 8 slots, the fast path's lanes for the slots 1 .. 7), slots that hold no call and
items without one on tile edges, support lists of 1 .. 257 rows, and item counts on both sides of the 8-item tile, the 512-item piece, the
4096-item chunk and chunk 65 (tests/emit_helpers.py; DESIGN.md, "Emit seams").

CPU: the C oracle, the plain restatement of the order (chain_helpers.restate for the clusters, oracle/py_restatement.py's rules per cluster:
emit_helpers.expected_calls) and, for the small tables, the rows the reference's own resolvers returned (tests/golden/emit_edges.json.gz,
made by tests/golden/make_golden_emit.py) agree; every table lands where it claims by the ORACLE's result, and the tables hold every cell
of the issue's list.  GPU: every table through the routes of the engine and once more through page-locked result arrays that are too
small at first (`published`), every field against the oracle, the call order and the support rows against the restatement directly, the
rows of the small tables against the recorded ones.  Every comparison is an exact integer or string comparison."""
import numpy as np
import pytest

from cutesv_amd import _abi, rows as rows_mod
from helpers import load_json, rows_by_task, assert_soa_equal, digest
import emit_helpers as eh
from test_chain_seams import run_route, ROUTES as CHAIN_ROUTES

ROUTES = CHAIN_ROUTES + ("published",)
E_NAMES = tuple("E%d" % n for n in eh.E_SIZES)
E_RUNS = [("E%d" % n, r) for n in eh.E_SIZES for r in (("oneshot", "int32", "resident") if n in eh.E_ROUTED else ("int32", "resident"))]


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
    return {c["name"]: c for c in load_json("emit_edges.json.gz")}


_REFS = {}


def reference(name):
    """(case, the restatement, the oracle's trimmed result, the expected calls, the expected support rows) of a table - computed once and left
    unchanged; of the tables above 8193 items one at a time is kept"""
    if name not in _REFS:
        case = eh.case(name)
        if case.only32:
            for k in [k for k in _REFS if _REFS[k][0].only32]:
                del _REFS[k]
        r = eh.ch.restate(case)
        r["cluster_id"] = np.array(r["cluster_id"], np.int32)
        want = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _oracle().cluster_batch(case.host_batch(), per_sig=True).trimmed().items()}
        calls, sup = eh.expected_calls(case, r)
        _REFS[name] = (case, r, want, calls, sup)
    return _REFS[name]


def by_task(case, rows):
    """[(segment, row)] -> {(type, chromosome): rows}"""
    tasks = case.store.tasks()
    out = {t: [] for t in tasks}
    for k, row in rows:
        out[tasks[k]].append(row)
    return out


def assert_golden_rows(rec, rows_by):
    want = {(t, c): (dg, rows) for t, c, dg, rows in rec["rows"]}
    assert set(rows_by) == set(want), (rec["name"], sorted(set(rows_by) ^ set(want)))
    for (t, c), (dg, rows) in want.items():
        got = [eh.slim_row(t, r) for r in rows_by[(t, c)]]
        assert len(got) == len(rows), "%s %s:%s: %d rows, the reference has %d" % (rec["name"], t, c, len(got), len(rows))
        for i, (g, w) in enumerate(zip(got, rows)):
            assert g == w, "%s %s:%s row %d:\n got %s\nwant %s" % (rec["name"], t, c, i, g, w)
        assert digest(t, rows_by[(t, c)]) == dg, "%s %s:%s: digest" % (rec["name"], t, c)


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", eh.SMALL_TABLES + E_NAMES)
def test_oracle_equals_the_restatement_and_tables_land(name):
    case, r, want, calls, sup = reference(name)
    assert np.array_equal(r["cluster_id"], want["cluster_id"]) and r["n_clusters"] == want["n_clusters"], name
    eh.assert_order_is_expected(want, calls, sup, name)
    assert eh.check_landing(case, want) == len(case.checks) > 0 and case.cells
    it = eh.items_of(case, want)
    assert [int(f) for f in it["first"]] == [f for f, _, _ in r["items"]], "the oracle's work items are not the restatement's"
    if case.store is not None:                               # the case's segments are the store's own
        hb = case.store.host_batch(case.store.tasks(), case.params)
        assert hb.segments.tobytes() == case.segment_table().tobytes() and np.array_equal(hb.read_id, case.host_batch().read_id)
    assert (case.n_sig > 500000) == (name in ("E266239", "E266240", "E266241", "E270337")) and case.only32 == (case.n_sig > 500000)


@pytest.mark.parametrize("name", eh.SMALL_TABLES)
def test_oracle_rows_are_the_reference_rows(golden, name):
    case, r, want, calls, sup = reference(name)
    rec = golden[name]
    assert (case.n_sig, eh.input_digest(case), rec["params"]) == (rec["n_sig"], rec["input_sha256"], dict(case.params.__dict__)), name
    rows, res, hb = rows_by_task(case.store, case.params, lambda hb: _oracle().cluster_batch(hb, per_sig=True))
    assert_soa_equal(res.trimmed(), want)
    assert_golden_rows(rec, rows)
    assert sum(len(x[3]) for x in rec["rows"]) == len(calls)


def test_every_listed_cell_is_claimed(golden):
    assert tuple(sorted(golden)) == tuple(sorted(eh.SMALL_TABLES))
    cells = set()
    for name in eh.SMALL_TABLES + E_NAMES:
        cells |= eh.case(name).cells
    cells |= {cell for cell, _, _ in eh.publish_plans(reference("A")[2])}
    need = eh.required_cells()
    assert need <= cells, sorted(need - cells, key=str)[:10]
    assert {c[0] for c in need} == set("ABCDEFG")
    # the two facts no earlier input of the suite reaches: 130 calls from one cluster, and a tile behind chunk 64
    assert ("max_calls_ge", 130) in eh.case("A").checks and ("fold",) in eh.case("E266241").checks
    assert eh.FOLD == 266240 and eh.E_SEAMS == (8, 512, 4096, 8192, 266240)


def test_publish_plans_sit_on_the_produced_counts():
    want = reference("A")[2]
    nc, ns = len(want["bp1"]), len(want["support_sig"])
    plans = {cell: (kw, retry) for cell, kw, retry in eh.publish_plans(want)}
    assert plans[("G", "cap_calls", "equal")][0]["cap_calls"] == nc and plans[("G", "cap_calls", "below")][0]["cap_calls"] == nc - 1
    assert plans[("G", "cap_support", "equal")][0]["cap_support"] == ns and plans[("G", "cap_support", "below")][0]["cap_support"] == ns - 1
    assert [retry for _, retry in plans.values()] == [False, True, False, True, False, False, False, False]


def test_restatement_of_the_order_on_a_hand_made_table():
    """two DEL clusters small enough to read: alleles of 3, 2 and 4 reads (the one of 2 has no call; by count, 3 comes before 4), then a
    cluster whose three reads are three alleles (a work item without a call), then one call"""
    L = eh.Layout("hand", eh.base_params())
    L.add("DEL", eh.dels((3, 2, 4)))
    L.add("DEL", eh.NOCALL)
    L.add("DEL", eh.dels((3,)))
    case = L.case()
    r = eh.ch.restate(case)
    calls, sup = eh.expected_calls(case, r)
    assert [(f, s) for f, s, _ in r["items"]] == [(0, 9), (9, 3), (12, 3)]
    assert calls.tolist() == [[0, 0, 10000, 20000, 3], [0, 0, 10000, 22000, 4], [0, 2, 20006, 20000, 3]]
    assert sup.tolist() == [0, 1, 2, 5, 6, 7, 8, 12, 13, 14]


# ------------------------------------------------------------------------------------------------ GPU
def run_published(ctx, case):
    """page-locked result arrays that are too small at first (the capacity retry), then once more into the recycled arrays"""
    ctx._res_cache = None
    hb = case.host_batch(narrow=True)
    res = ctx.cluster_batch(hb, per_sig=True, cap_calls=8, cap_support=8, reuse=True)
    first = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in res.trimmed().items()}
    assert res.narrow_support and res.cap_calls == res.n_calls + 1 and res.cap_support == res.n_support + 1      # (what the retry asked for)
    again = ctx.cluster_batch(hb, per_sig=True, cap_calls=res.cap_calls, cap_support=res.cap_support, reuse=True)
    assert again is res
    return first, again.trimmed()


def assert_result(name, got, rows=None, golden=None):
    case, r, want, calls, sup = reference(name)
    assert_soa_equal(got, want)                              # every SoA field, the support lists, cluster_id, allele_id, seg_status
    eh.assert_order_is_expected(got, calls, sup, name)
    if golden is not None:
        assert_golden_rows(golden[name], by_task(case, rows_mod.materialise_py(case.store, case.segment_table(), got)))


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", eh.SMALL_TABLES)
def test_gpu_emit_at_the_seams(ctx, golden, monkeypatch, name, route):
    case = reference(name)[0]
    results = run_published(ctx, case) if route == "published" else (run_route(ctx, route, case, monkeypatch),)
    for got in results:
        assert got is not None, (name, route)
        try:
            assert_result(name, got, golden=golden)
        except AssertionError as e:
            raise AssertionError("%s via %s: %s" % (name, route, e)) from None


@pytest.mark.gpu
@pytest.mark.parametrize("name,route", E_RUNS)
def test_gpu_item_counts_at_the_seams(ctx, monkeypatch, name, route):
    case = reference(name)[0]
    got = run_route(ctx, route, case, monkeypatch)
    assert got is not None, (name, route)
    try:
        assert_result(name, got)
    except AssertionError as e:
        raise AssertionError("%s via %s: %s" % (name, route, e)) from None


@pytest.mark.gpu
@pytest.mark.parametrize("plan", range(8))
def test_gpu_publish_edges(ctx, plan):
    """k_publish on table A: capacities on and one below the produced counts (below: nothing is written, the retry delivers the same
    bytes), and the slim forms of the result"""
    case, r, want, calls, sup = reference("A")
    cell, kw, retry = eh.publish_plans(want)[plan]
    ctx._res_cache = None
    res = ctx.cluster_batch(case.host_batch(narrow=True), per_sig=True, reuse=True, **kw)
    t = res.trimmed()
    assert (res.n_calls, res.n_support) == (len(want["bp1"]), len(want["support_sig"])), cell
    if "cap_calls" in kw:
        assert ((res.cap_calls, res.cap_support) != (kw["cap_calls"], kw["cap_support"])) == retry, (cell, res.cap_calls, res.cap_support)
        assert_soa_equal(t, want)
        eh.assert_order_is_expected(t, calls, sup, str(cell))
        return
    fields = kw.get("fields", _abi.OPTIONAL_CALL_FIELDS)
    for f in ("call_seg", "bp1", "bp2", "support") + tuple(fields):
        assert t[f] is not None and np.array_equal(t[f].astype(np.int64), want[f].astype(np.int64)), (cell, f)
        assert not (kw.get("coord32") and f in _abi.COORD_FIELDS) or t[f].dtype == np.int32, (cell, f)
    for f in _abi.OPTIONAL_CALL_FIELDS:
        assert f in fields or t[f] is None, (cell, f)
    if kw.get("no_support"):
        assert t["support_off"] is None and t["support_sig"] is None
    else:
        assert t["support_sig"].dtype == np.int32                                              # (the page-locked support list is the int32 one)
        assert np.array_equal(t["support_off"], want["support_off"]) and np.array_equal(t["support_sig"], want["support_sig"]), cell
    for f in ("cluster_id", "allele_id"):
        assert np.array_equal(t[f], want[f]), (cell, f)
