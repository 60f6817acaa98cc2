"""The chain kernels (k_chain_count, k_chain_apply, k_chain_ids) AT the seams of their layout: a break, a segment start, a position 0 or the
end of the batch placed on purpose on the byte of 8 signatures a lane owns, the 64-flag word, the 512-signature wavefront span, the
2048-signature tile, the halo row behind the tile and the rows behind that (tests/chain_helpers.py; DESIGN.md, "Chain seams").

CPU: the plain restatement (chain_helpers.restate: Python ints, from the rules alone) and the C oracle agree on cluster_id, n_clusters and
on which clusters are work items for every case; every case keeps the input order contract and lands where it claims (check_landing); the
union of the cases holds every cell of the issue's list.  GPU: every case through every route of the engine - one-shot int64, int32
columns, gate-first, resident (upload, validate, run, run), and for int32 cases the position column as 16-bit gaps - every field against the
oracle (assert_soa_equal) and cluster_id against the restatement's array directly.  Every comparison is an exact integer comparison."""
import numpy as np
import pytest

from helpers import assert_soa_equal
import chain_helpers as ch

ROUTES = ("oneshot", "int32", "gate_first", "resident", "gaps16")
GROUPS = sorted(ch.groups())
BIG = (2049, 2052)
INT64_GROUPS = ("f4_bias",) + tuple(g for g in GROUPS if g.startswith("f6_shifted_"))       # groups that hold values beyond 32 bits: those cases have no int32 form


def _oracle():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


_REFS = {"group": None, "by_name": {}}


def references(group):
    """{name: (case, the restatement, the oracle's trimmed result with cluster_id)} of a group's cases - computed once for the tests of the
    group (which run one after the other) and left unchanged; one group at a time is kept"""
    if _REFS["group"] != group:
        cases = [ch.big_case(int(group.rsplit("_", 1)[1]))] if group.startswith("f7_big_") else ch.cases_of(group)
        by_name = {}
        for case in cases:
            ch.assert_order(case)
            r = ch.restate(case)
            r["cluster_id"] = np.array(r["cluster_id"], np.int32)
            res = _oracle().cluster_batch(case.host_batch(), per_sig=True)
            by_name[case.name] = (case, r, {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in res.trimmed().items()})
        _REFS["group"], _REFS["by_name"] = group, by_name
    return _REFS["by_name"]


def assert_restatement_is_the_oracle(group, name):
    case, r, want = references(group)[name]
    assert np.array_equal(r["cluster_id"], want["cluster_id"]), (name, np.flatnonzero(r["cluster_id"] != want["cluster_id"])[:5])
    assert r["n_clusters"] == want["n_clusters"], name
    # the builders make every work item a call (chain_helpers.cols): the clusters the oracle's calls name ARE the work items
    item_ids = [int(r["cluster_id"][f]) for f, _, _ in r["items"]]
    assert sorted(set(want["call_cluster"].tolist())) == item_ids, (name, item_ids[:5], want["call_cluster"][:5])
    seg_of = dict(zip(want["call_cluster"].tolist(), want["call_seg"].tolist()))
    assert [seg_of[i] for i in item_ids] == [s for _, _, s in r["items"]], name
    return case, r


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("group", GROUPS)
def test_restatement_equals_the_oracle_and_cases_land(group):
    n = 0
    assert list(references(group)) == ch.groups()[group]
    for name in ch.groups()[group]:
        case, r = assert_restatement_is_the_oracle(group, name)
        assert case.checks, name
        n += ch.check_landing(case, r)
    assert n > 0


@pytest.mark.parametrize("tiles", BIG)
def test_large_shapes_restated(tiles):
    case, r = assert_restatement_is_the_oracle("f7_big_%d" % tiles, "f7_tiles_%d" % tiles)
    assert ch.check_landing(case, r) == 2 and case.fits32
    # 2052 tiles + 5 signatures: the last workgroup of k_chain_apply begins at tile 2052, behind the 2048 tile counts of its first form
    assert (case.n_sig + ch.TILE - 1) // ch.TILE == tiles + 1
    first_tile_of_last_group = ((tiles + 1 - 1) // 4) * 4
    assert (first_tile_of_last_group > 2048) == (tiles == 2052)


def test_every_listed_cell_is_claimed():
    cells = set(ch.index()[1])                               # (index() also asserts that every case claims cells and carries checks)
    for tiles in BIG:
        cells |= {(7, "tiles", tiles)}                       # (built and landed by test_large_shapes_restated)
    need = ch.required_cells()
    assert need <= cells, sorted(need - cells, key=str)[:10]
    assert {c[0] for c in need} == set(range(1, 8))
    for o in ch.SEAMS:
        assert ch.seam_class(o)
    assert len(ch.SEAMS) == 60 and set(ch.SEAMS) >= {1, 17, 63, 65, 504, 520, 2040, 2056, 2111, 2113, 4095, 4097}


def test_restatement_on_a_hand_made_batch():
    """the restatement itself on rows small enough to read: a (0,0) row, both biases, an INV b gap, a TRA aux change, a dropped segment"""
    segs = [ch.seg("DEL", 5, 10, 2), ch.seg("INV", 4, 10, 2), ch.seg("TRA", 3, 10, 1), ch.seg("DEL", 2, 10, 1, genotype=True)]
    a = [0, 5, 15, 26, 27, 100, 101, 102, 103, 7, 8, 9, 50, 51]
    b = [0, 1, 1, 1, 1, 600, 611, 600, 611, 900, 901, 902, 1, 1]
    x = [0, 0, 0, 0, 0, 1, 1, 1, 2, 8, 8, 16, 0, 0]
    r = ch.restate(ch.Case("hand", 0, "hand", segs, a, b, x, {("hand",)}, [("W", 14)]))
    assert r["flags"] == [0, 1, 3, 5, 6, 8, 9, 11, 12]
    assert r["cluster_id"] == [0, 1, 1, 2, 2, 3, 4, 4, 5, 6, 6, 7, 8, 8] and r["n_clusters"] == 9
    assert r["items"] == [(1, 2, 0), (3, 2, 0), (6, 2, 1), (9, 2, 2), (11, 1, 2)]       # (0,0) singleton: none; the genotyped DEL without reads: dropped
    assert [sorted(t) for t in r["tiers"]] == [["tiny"], ["tiny"], [], [], []]
    assert [sorted(ch.tier_bits("INS", m)) for m in (16, 17, 32, 33, 64, 65)] == [["tiny"], [], [], ["wide"], ["wide"], ["big"]]
    assert sorted(ch.tier_bits("DUP", 16)) == [] and sorted(ch.tier_bits("TRA", 65)) == ["big"]


# ------------------------------------------------------------------------------------------------ GPU
def run_route(ctx, route, case, monkeypatch):
    """the case through one route of the engine -> trimmed result, or None where the route does not apply (int32 forms of values beyond 32 bits)"""
    from cutesv_amd import engine, _abi
    if route in ("int32", "gaps16") and not case.fits32:
        return None
    if route == "oneshot":
        if case.only32:
            return None
        return ctx.cluster_batch(case.host_batch(), per_sig=True).trimmed()
    if route == "int32":
        hb = case.host_batch(narrow=True)
        assert hb.a.dtype == np.int32 and hb.c.flags & _abi.IN_SIG_I32
        return ctx.cluster_batch(hb, per_sig=True).trimmed()
    if route == "gate_first":
        from test_hip_parity import _pinned_batch
        monkeypatch.setenv("CSV_LAZY_MIN", "0")
        res = ctx.cluster_batch(_pinned_batch(case.host_batch(narrow=case.only32)), per_sig=True)
        assert ctx.lazy_info()[0], "the call did not take the gate-first form"
        return res.trimmed()
    if route == "resident":
        ctx.upload(case.host_batch(narrow=case.only32), per_sig=True)
        ctx.validate()                                       # the input order contract, on the device (k_validate_order)
        ctx.run()
        ctx.run()
        return ctx.download(per_sig=True).trimmed()
    assert route == "gaps16"
    monkeypatch.setenv("CSV_DELTA16_MIN", "0")
    monkeypatch.setenv("CSV_DELTA16_ESC", "0")
    monkeypatch.setenv("CSV_LAZY_MIN", "1000000000")         # the bulk form: k_unpack_a16 writes the column AND the padding behind it
    hb = case.host_batch(narrow=True, copy=engine.pinned_copy, empty=engine.pinned_empty, gaps16=True)
    assert hb.c.flags & _abi.IN_SIG_DELTA16 and hb.a_delta is not None
    got = ctx.cluster_batch(hb, per_sig=True).trimmed()
    assert ctx.delta16_info() and not ctx.lazy_info()[0]
    return got


def applies(route, case):
    if route in ("int32", "gaps16"):
        return case.fits32
    return route != "oneshot" or not case.only32


def assert_route(ctx, route, group, name, monkeypatch):
    case, r, want = references(group)[name]
    got = run_route(ctx, route, case, monkeypatch)
    assert (got is not None) == applies(route, case), (name, route)
    if got is None:
        return 0
    try:
        assert_soa_equal(got, want)                          # every SoA field, the support lists, cluster_id, allele_id, seg_status
        assert np.array_equal(got["cluster_id"], r["cluster_id"]), "cluster_id differs from the restatement"
    except AssertionError as e:
        raise AssertionError("%s via %s: %s" % (name, route, e)) from None
    return 1


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("group", GROUPS)
def test_gpu_chain_at_the_seams(ctx, monkeypatch, group, route):
    names = ch.groups()[group]
    ran = sum(assert_route(ctx, route, group, name, monkeypatch) for name in names)
    assert ran == len(names) or (route in ("int32", "gaps16") and group in INT64_GROUPS), (group, route, ran)


@pytest.mark.gpu
@pytest.mark.parametrize("route", [r for r in ROUTES if r != "oneshot"])
@pytest.mark.parametrize("tiles", BIG)
def test_gpu_chain_apply_prefix_over_many_tiles(ctx, monkeypatch, tiles, route):
    """2049 tiles + 5 signatures, and 2052 tiles + 5: the smallest batch whose last workgroup of k_chain_apply sums tile counts in the loop
    behind the first 2048 (int32 columns; all singletons but a few clusters of 3 around the last tiles)"""
    assert assert_route(ctx, route, "f7_big_%d" % tiles, "f7_tiles_%d" % tiles, monkeypatch) == 1
