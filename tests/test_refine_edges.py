"""The refine rules (generate_del_cluster / generate_ins_cluster, generate_dup_cluster, generate_semi_inv_cluster,
generate_semi_tra_cluster and the chaining in front of them) ON their thresholds, at every cluster size beside a tier cut of the
refine kernels: crafted clusters (tests/refine_helpers.py) against the rows the reference's resolvers returned for them
(tests/golden/refine_edges.json.gz, made by tests/golden/make_golden_refine.py).

A table is one parameter set; its sites are one case of one rule at one size each (3 .. 2049 signatures), side by side on one
chromosome.  Variants: (a) as built, (b) every position moved by 2^33 + 12 345 (int64 columns only), (c) the DEL / INS rules with
two position groups 270 000 apart under a bias of 300 000, (d) genotyped, with a reads table that makes search_threshold show in DR.

CPU: the builders give the recorded inputs, the oracle's rows are the reference's, every site shows what its builder says it must
(the landing checks), and every (rule, type, tier) cell a variant claims holds a chained cluster of that tier according to the
oracle's cluster_id and refine_helpers.tier_of.  GPU: every table and variant through every route of the engine, bit for bit
against the oracle and row for row against the reference.  Every comparison is an exact integer or string comparison; the one
canonicalisation is the sorted read list of DUP / TRA rows (helpers.SET_ORDER_TYPES)."""
import numpy as np
import pytest

from cutesv_amd import _abi
from helpers import load_json, rows_by_task, assert_soa_equal, digest
import refine_helpers as rh

ROUTES = ("oneshot", "pinned_i32", "gate_first", "no_tiny", "no_pair_in_mid", "resident")
INT64_ROUTES = tuple(r for r in ROUTES if r != "pinned_i32")        # variant (b) has no int32 form
GPU_RUNS = [(n, r) for n in rh.CASE_NAMES for r in (INT64_ROUTES if n.startswith("b_") else ROUTES)]


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
    return {c["name"]: c for c in load_json("refine_edges.json.gz")}


_WANT = {}


def oracle_result(name):
    """(store, the oracle's trimmed result with cluster_id / allele_id) of a case, computed once and left unchanged"""
    if name not in _WANT:
        case = rh.case(name)
        st = rh.store_of(case)
        hb = st.host_batch(st.tasks(), case["params"])
        _WANT[name] = (st, _oracle().cluster_batch(hb, per_sig=True).trimmed())
    return _WANT[name]


def assert_golden_rows(rec, rows_by):
    want = {(t, c): (dg, rows) for t, c, dg, rows in rec["rows"]}
    assert set(rows_by) == set(want), (rec["name"], sorted(set(rows_by) ^ set(want)))
    for (t, c), (dg, rows) in want.items():
        got = [rh.slim_row(t, r) for r in rows_by[(t, c)]]
        assert len(got) == len(rows), "%s %s:%s: %d rows, the reference has %d" % (rec["name"], t, c, len(got), len(rows))
        for i, (g, w) in enumerate(zip(got, rows)):
            assert g == w, "%s %s:%s row %d:\n got %s\nwant %s" % (rec["name"], t, c, i, g, w)
        assert digest(t, rows_by[(t, c)]) == dg, "%s %s:%s: digest" % (rec["name"], t, c)


# ------------------------------------------------------------------------------------------------ CPU
def test_builders_give_the_recorded_inputs(golden):
    assert tuple(sorted(golden)) == tuple(sorted(rh.CASE_NAMES))
    for name in rh.CASE_NAMES:
        case = rh.case(name)
        st = rh.store_of(case)
        assert (st.n_sig, st.n_reads, rh.input_digest(st)) == (golden[name]["n_sig"], golden[name]["n_reads"], golden[name]["input_sha256"]), name
        assert golden[name]["params"] == dict(case["params"].__dict__), name
        if case["variant"] == "b":
            assert int(st.a.min()) > (1 << 33) and "a" not in (st.with_narrow().narrow or {})      # no int32 twins: int64 routes only
        if case["variant"] == "c":
            beg, end = st.seg_index[("DEL", "1")]
            assert int(np.diff(st.a[beg:end]).max()) > (1 << 18)


@pytest.mark.parametrize("name", rh.CASE_NAMES)
def test_oracle_rows_are_the_reference_rows(golden, name):
    case = rh.case(name)
    st, want = oracle_result(name)
    rows, res, hb = rows_by_task(st, case["params"], lambda hb: _oracle().cluster_batch(hb, per_sig=True))
    assert_soa_equal(res.trimmed(), want)
    assert_golden_rows(golden[name], rows)


@pytest.mark.parametrize("name", rh.CASE_NAMES)
def test_every_site_lands_on_its_threshold(golden, name):
    """the builders' own statements of what the reference must return, checked on the recorded rows"""
    case = rh.case(name)
    by_type = {}
    for t, c, _, rows in golden[name]["rows"]:
        assert c == "1"
        by_type[t] = rows
    n = rh.check_landing(case, by_type)
    assert n == sum(len(s["expect"]) for s in case["sites"]) and all(s["expect"]["rows"] == 0 or "support" in s["expect"] for s in case["sites"])
    inside = sum(len(rh.rows_of_site(rows, s)) for s in case["sites"] for t, rows in by_type.items() if t == s["type"])
    assert inside == sum(len(r) for r in by_type.values()), "a row lies outside every site"


@pytest.mark.parametrize("variant", rh.VARIANTS)
def test_every_claimed_rule_and_tier_holds_a_cluster(variant):
    """each (rule, type, tier) cell: a site of the rule whose chained cluster - per the oracle's cluster_id - has exactly the claimed
    size, and tier_of puts that size in the tier"""
    cells = set()
    for name in rh.CASE_NAMES:
        if not name.startswith(variant + "_"):
            continue
        st, want = oracle_result(name)
        got, missing = rh.cluster_cells(rh.case(name), st, want["cluster_id"])
        assert not missing, (name, missing[:5])
        cells |= got
    claimed = rh.claimed_cells(variant)
    assert claimed <= cells, sorted(claimed - cells)
    tiers = {t: set(tier for r, tt, tier in cells if tt == t) for t in rh.TIERS}
    for t in (("DEL", "INS") if variant == "c" else rh.TIERS):
        assert tiers[t] >= set(rh.TIERS[t]) - ({"scratch"} if variant in ("c", "d") else set()), (t, tiers[t])


def test_tier_model_and_the_batch_geometry():
    cuts = {"DEL": (16, 32, 64, 256, 2048), "DUP": (64, 256, 2048)}
    for t, cs in cuts.items():
        for k, c in enumerate(cs):
            assert rh.tier_of(t, c) == rh.TIERS[t][k] and rh.tier_of(t, c + 1) == rh.TIERS[t][k + 1]
    assert rh.tier_of("INS", 16, no_tiny=True) == "wave32" and rh.tier_of("TRA", 3) == "wave"
    # the base table: a cluster straddles a 2048-signature tile edge in every type, and the batch ends inside a cluster that is a call
    st, want = oracle_result("a_base")
    cid = want["cluster_id"]
    edges = np.arange(2048, st.n_sig, 2048)
    straddle = edges[cid[edges] == cid[edges - 1]]
    for t in rh.TIERS:
        beg, end = st.seg_index[(t, "1")]
        assert ((straddle > beg) & (straddle < end)).any(), t
    assert np.bincount(cid[cid >= 0])[cid[-1]] >= 3


# ------------------------------------------------------------------------------------------------ GPU
def _engine(ctx, route, monkeypatch):
    from cutesv_amd import engine
    if route == "gate_first":
        from test_hip_parity import _pinned_batch
        monkeypatch.setenv("CSV_LAZY_MIN", "0")

        def run(hb):
            res = ctx.cluster_batch(_pinned_batch(hb), per_sig=True)
            assert ctx.lazy_info()[0], "the call did not take the gate-first form"
            return res
        return run
    if route == "resident":
        def run(hb):
            ctx.upload(hb, per_sig=True)
            ctx.run()
            ctx.run()
            return ctx.download(per_sig=True)
        return run
    if route == "no_tiny":
        monkeypatch.setenv("CSV_NO_TINY", "1")
    if route == "no_pair_in_mid":
        monkeypatch.setenv("CSV_NO_PAIR_IN_MID", "1")
    assert isinstance(ctx, engine.Context)
    return lambda hb: ctx.cluster_batch(hb, per_sig=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name,route", GPU_RUNS)
def test_gpu_equals_the_oracle_and_the_reference(ctx, golden, monkeypatch, name, route):
    case = rh.case(name)
    st, want = oracle_result(name)
    run = _engine(ctx, route, monkeypatch)
    src = st
    if route == "pinned_i32":
        src = st.pinned()
        hb = src.host_batch(src.tasks(), case["params"])
        assert hb.a.dtype == np.int32 and hb.c.flags & _abi.IN_SIG_I32
    rows, res, hb = rows_by_task(src, case["params"], run)
    if route != "pinned_i32":
        assert hb.a.dtype == np.int64
    assert_soa_equal(res.trimmed(), want, store=st)                   # every SoA field, support lists, cluster_id, allele_id, seg_status
    assert_golden_rows(golden[name], rows)
