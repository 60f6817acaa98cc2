"""The rebuild sort (csv_rebuild_signatures: stage_rebuild.hip.h, sort.hip.h) on every route and key layout, against a stable
lexsort.

CPU tests (no marker): the yardstick `rebuild_helpers.rebuild_host` against the reference's recorded lists
(golden/rebuild_order.json.gz), and the geometry every crafted case claims - route, passes, digit shapes, seam and tie positions -
asserted from the case's own columns through `rebuild_helpers.key_layout`.
GPU tests (-m gpu): every case through rebuild.rebuild_columns (one through the pool), integer equality of every returned column
with the yardstick, src_row included; after every call the pass count and the route the library reports equal the model's."""
import os
import re

import numpy as np
import pytest

from cutesv_amd import _abi, _lib, engine, rebuild
from helpers import load_json, rebuild_expected

import rebuild_helpers as rh
from rebuild_helpers import COMPACT, WIDE, PERM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = (COMPACT, WIDE, PERM)
ROUTE_IDS = [rh.ROUTE_NAME[r] for r in ROUTES]
ENV = "CSV_RB_PERM_SORT"


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


def on_route(cols, major, route, natural_perm=False):
    """the case's rows on `route` -> (columns, permutation sort forced by the environment): the wide route by padding a and b to
    T == 128; the permutation route forced on the columns as they are, or (natural_perm) by padding to T == 129"""
    if route == PERM and not natural_perm:
        return cols, True
    return rh.to_route(cols, major, route), False


# ================================================================================================ CPU: the interface
def test_route_accessor_is_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "cutesv_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+csv_rebuild_route\s*\(\s*const\s+csv_ctx\s*\*", header)
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    assert "csv_rebuild_route" in bound and len(bound["csv_rebuild_route"][1]) == 1
    assert hasattr(_lib.lib(), "csv_rebuild_route")
    assert _lib.lib().csv_rebuild_route(None) == 0                   # (no context: no rebuild; needs no GPU)
    assert (_abi.RB_ROUTE_NONE, _abi.RB_ROUTE_COMPACT, _abi.RB_ROUTE_WIDE, _abi.RB_ROUTE_PERM) == (0, COMPACT, WIDE, PERM)


# ================================================================================================ CPU: the yardstick
def test_yardstick_reproduces_the_reference_order():
    """rebuild_host on the concatenated per-worker candidates of every recorded case, read back through src_row, == the lists the
    reference's process_process_sigs_type + remove_duplicates_sorted wrote (main script :750-857, :958-969): duplicates across
    workers, adversarial name orders, INS rows that differ in their sequence or their x.5 only"""
    cases = load_json("rebuild_order.json.gz")
    assert len(cases) > 0
    n_tie = n_drop = 0
    for case in cases:
        cols, major, nodedup, seqs, half, rows = rh.golden_case_columns(case)
        got = rh.rebuild_host(cols, major, nodedup, seqs.__getitem__, half.__getitem__)
        mine = {}
        for sr in got["src_row"].tolist():
            t, x = rows[sr]
            row = tuple([int(x[0])] + list(x[1:])) if t in ("DEL", "INS", "DUP") else tuple(x)
            mine.setdefault((t, x[-1]), []).append(row)
        want = rebuild_expected(case)
        assert set(mine) == set(want), case["name"]
        for k, lst in want.items():
            assert mine[k] == lst, (case["name"], k)
        assert got["n_out"] == sum(len(v) for v in want.values()) and got["n_ins_ties"] == 0
        assert got["seg_count"].sum() == got["n_out"]
        n_tie += got["n_tie_rows"]
        n_drop += got["n_tie_dropped"]
        # ... and without the sequences the tie rows are counted, not settled
        plain = rh.rebuild_host(cols, major, nodedup)
        assert plain["n_out"] == got["n_out"] + got["n_tie_dropped"] and (plain["n_ins_ties"] > 0) == (got["n_tie_rows"] > 0)
    assert n_tie > 0 and n_drop > 0                                 # (the recorded cases do hold sequence ties and whole-tuple duplicates)


def test_yardstick_on_a_hand_made_case():
    """the three rules, small enough to check by eye: segment 0 de-duplicated, 1 de-duplicated aux-major, 2 keep-every-row"""
    major, nodedup = rh.flags(3, major=(1,), nodedup=(2,))
    #                  0  1  2  3  4  5  6  7  8  9
    cols = rh.columns([0, 0, 0, 1, 1, 1, 2, 2, 2, 0],
                      [5, 5, 5, 9, 3, 3, 4, 4, 4, 5],
                      [1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
                      [7, 7, 7, 7, 7, 7, 7, 7, 7, 7],
                      [1, 2, 1, 0, 1, 1, 8, 9, 8, 1])
    got = rh.rebuild_host(cols, major, nodedup)
    # segment 0: equal keys, aux 1, 2, 1, 1 in input order: the fourth repeats the third; segment 1: aux first (0 before 1), one duplicate
    assert got["src_row"].tolist() == [0, 1, 2, 3, 4, 6, 7, 8] and got["n_ins_ties"] == 2 and got["seg_count"].tolist() == [3, 2, 3]
    seqs, half = {6: "C", 7: "A", 8: "C"}, {6: 0, 7: 0, 8: 0}
    tied = rh.rebuild_host(cols, major, nodedup, seqs.__getitem__, half.__getitem__)
    assert tied["src_row"].tolist() == [0, 1, 2, 3, 4, 7, 6] and (tied["n_tie_rows"], tied["n_tie_dropped"], tied["n_ins_ties"]) == (3, 1, 0)
    half[8] = 1
    assert rh.rebuild_host(cols, major, nodedup, seqs.__getitem__, half.__getitem__)["src_row"].tolist() == [0, 1, 2, 3, 4, 7, 6, 8]


# ================================================================================================ CPU: the geometry of every case
@pytest.mark.parametrize("name", sorted(rh.LAYOUTS))
def test_layout_case_reaches_the_geometry_it_claims(name):
    n, widths, forced, route, npass, last = rh.LAYOUTS[name]
    cols, major, nodedup, forced = rh.layout_case(name)
    L = rh.key_layout(cols, major, forced)
    sb, xb, ab, bb, rb, pb = widths
    assert (L["n"], L["sb"], L["xb"], L["ab"], L["bb"], L["rb"], L["pb"]) == (n, sb, xb, ab, bb, rb, pb)
    assert (L["route"], L["npass"]) == (route, npass), (name, L)
    if route != PERM:
        assert L["digits"][-1] == last and len(L["digits"]) == -(-L["T"] // 10)
        assert L["digits"][0] == ((L["ib"], 10) if route == COMPACT else (0, 10))
    want = rh.rebuild_host(cols, major, nodedup)
    assert 0 < n - want["n_out"] < n // 8 and want["n_ins_ties"] > 0                    # duplicates to drop, ties to count
    if route != PERM:
        # every pass that lies below the segment field alone orders some pair of neighbours, in both input orders: a wrong digit
        # there shows (the passes that reach into the segment bits order the random rows at large)
        for p, (up, down) in enumerate(rh.probed_passes(cols, major, L, want)):
            assert (up > 0 and down > 0) or (p + 1) * 10 > L["T"] - L["sb"], (name, p, up, down)


def test_layout_table_of_the_issue():
    """the seven layouts: sums of widths as stated"""
    def L(name):
        cols, major, _, forced = rh.layout_case(name)
        return rh.key_layout(cols, major, forced)
    a = L("c_sum128"); assert a["ib"] + a["T"] + a["pb"] == 128 and a["route"] == COMPACT
    b = L("w_sum129"); assert b["ib"] + b["T"] + b["pb"] == 129 and b["ab"] == a["ab"] + 1 and b["route"] == WIDE
    c = L("w_ibT128"); assert c["ib"] + c["T"] == 128 and c["pb"] == 0 and c["route"] == WIDE
    d = L("c_ibT127"); assert d["ib"] + d["T"] == 127 and d["pb"] == 1 and d["route"] == COMPACT
    e = L("w_T128"); assert e["T"] == 128 and e["digits"][-1][1] == 8
    f = L("p_T129"); assert f["T"] == 129 and f["route"] == PERM
    g = L("p_forced_c53"); assert g["T"] == 53 and g["route"] == PERM and L("c53")["route"] == COMPACT


@pytest.mark.parametrize("at", rh.WIDEST_AT)
def test_widest_case_has_every_maximum_in_one_row(at):
    cols, major, nodedup, _ = rh.widest_case(at)
    L = rh.key_layout(cols, major)
    assert (L["sb"], L["xb"], L["ab"], L["bb"], L["rb"], L["pb"]) == rh.WIDEST and L["n"] == 4097
    assert (L["route"], L["npass"]) == (PERM, 2 + 4 + 8 + 8 + 4)
    for k in rh.COLS:
        assert np.flatnonzero(cols[k] == cols[k].max()).tolist() == [at], k
    assert int(cols["a"][at]) == (1 << 63) - 1 and int(cols["aux"][at]) == (1 << 31) - 1 and major[cols["seg"][at]]
    for route, T in ((COMPACT, 94), (WIDE, 128)):
        small, major, nodedup = rh.one_wide_row_case(at, route)
        L = rh.key_layout(small, major)
        assert (L["route"], L["T"], L["xb"], L["pb"]) == (route, T, 4, 4)
        for k in rh.COLS:
            assert int(np.delete(small[k], at).max()) <= 7 < int(small[k][at]), k


def test_digit_shapes_cover_every_position_in_the_element():
    """conditions on the case list: where a digit can lie relative to the 64-bit words of an element, and how narrow the last is"""
    shapes = {COMPACT: set(), WIDE: set()}
    lasts = {COMPACT: set(), WIDE: set()}
    for name in rh.LAYOUTS:
        cols, major, _, forced = rh.layout_case(name)
        L = rh.key_layout(cols, major, forced)
        if L["route"] != PERM:
            shapes[L["route"]].update(L["digits"])
            lasts[L["route"]].add(L["digits"][-1][1])
    c, w = shapes[COMPACT], shapes[WIDE]
    assert any(s < 64 < s + d for s, d in c) and any(s + d == 64 for s, d in c) and any(s == 64 for s, d in c) and any(s > 64 for s, d in c)
    assert {1, 3, 9, 10} <= lasts[COMPACT]
    assert (54, 10) in c and (64, 3) in c and (63, 3) in c and (123, 4) in c
    assert any(s == 0 for s, d in w) and any(s < 64 < s + d for s, d in w) and 8 in lasts[WIDE] and (120, 8) in w


def _routes_of(cols, major, natural_perm=False):
    out = {}
    for route in ROUTES:
        c, forced = on_route(cols, major, route, natural_perm)
        out[route] = rh.key_layout(c, major, forced)
    return out


@pytest.mark.parametrize("n", rh.SEAM_N)
def test_seam_cases_reach_their_route_and_their_seams(n):
    for kind in rh.SEAM_KINDS:
        cols, major, nodedup = rh.seam_case(kind, n)
        for route, L in _routes_of(cols, major).items():
            assert L["route"] == route and L["n"] == n, (kind, n, route, L)
            if route == WIDE:
                assert L["T"] == 128
        want = rh.rebuild_host(cols, major, nodedup)
        if kind == "same_dedup":
            assert want["n_out"] == 1 and want["src_row"].tolist() == [0]
        elif kind == "same_nodedup":
            assert want["src_row"].tolist() == list(range(n)) and want["n_ins_ties"] == n - 1
        elif kind == "pairs_121":
            order = np.lexsort((cols["rid"], cols["b"], cols["a"], cols["seg"]))
            full = np.stack([cols[k][order] for k in rh.COLS])
            for p in rh.SEAM_PAIRS:
                if p < n:
                    assert (full[:, p] == full[:, p - 1]).all()
                    assert order[p] not in want["src_row"] and order[p - 1] in want["src_row"]
            if n >= 3:                                          # the first group: equal keys, aux 1, 2, 1, all three stay
                assert full[1, :3].tolist() == [0, 0, 0] and full[4, :3].tolist() == [1, 2, 1] and (want["a"][:3] == 0).all()
                assert sorted(order[:3].tolist()) == order[:3].tolist()
        else:
            keys = set(zip(*(cols[k].tolist() for k in ("seg", "a", "b", "rid"))))
            assert len(keys) <= 48 and (n < 512 or (0 < want["n_out"] < n and want["n_ins_ties"] > 0))


@pytest.mark.parametrize("route", (COMPACT, WIDE), ids=ROUTE_IDS[:2])
def test_skew_cases_have_the_digit_distribution_they_claim(route):
    for kind in rh.SKEW_KINDS:
        cols, major, nodedup = rh.skew_case(kind, route)
        L = rh.key_layout(cols, major)
        assert L["route"] == route and L["T"] == (60 if route == COMPACT else 120) and L["pb"] == 2, (kind, L)
        assert any(s < 64 < s + d for s, d in L["digits"])
        for p, dig in enumerate(rh.pass_digits(cols, major, L)):
            chunks = [dig[c:c + 64] for c in range(0, len(dig) - 63, 64)]
            if kind == "one_bucket":
                assert set(dig) == {1023}
            elif kind == "distinct64":
                assert all(len(set(ch)) == 64 for ch in chunks), (kind, p)
            else:
                assert set(dig) == {0, 1023} and all(ch == ch[:2] * 32 and ch[0] != ch[1] for ch in chunks), (kind, p)
        n_out = rh.rebuild_host(cols, major, nodedup)["n_out"]
        assert n_out == (L["n"] if kind != "alternate" else min(L["n"], 1 << L["npass"]))      # (alternate: a key per value of the low bits of i)


@pytest.mark.parametrize("n", rh.CARRY_N)
def test_carry_cases_have_the_tile_counts_they_claim(n):
    cols, major, nodedup = rh.carry_case(n)
    assert -(-n // rh.WTILE) == {rh.CARRY_N[0]: 65, rh.CARRY_N[1]: 257}[n]
    for route, L in _routes_of(cols, major, natural_perm=True).items():
        assert L["route"] == route, (n, route, L)
        assert L["T"] == {COMPACT: 24, WIDE: 128, PERM: 129}[route]
    want = rh.carry_host(n)
    assert 0 < want["n_out"] < n and want["n_ins_ties"] > 0


@pytest.mark.parametrize("name", sorted(rh.TIE_GROUPS))
def test_tie_cases_have_their_groups_where_they_claim(name):
    cols, major, nodedup, seqs, half = rh.tie_case(name)
    for route, L in _routes_of(cols, major).items():
        assert L["route"] == route and L["n"] == rh.TIE_N
    auxk = np.where(major[cols["seg"]] != 0, cols["aux"], 0)
    order = np.lexsort((cols["rid"], cols["b"], cols["a"], auxk, cols["seg"]))
    s, a, r = cols["seg"][order], cols["a"][order], cols["rid"][order]
    cont = np.r_[False, (s[1:] == s[:-1]) & (a[1:] == a[:-1]) & (r[1:] == r[:-1])] & (nodedup[s] != 0)
    heads = np.flatnonzero(~cont & np.r_[cont[1:], False])
    sizes = [int(np.argmin(np.r_[cont[h + 1:], False])) + 1 for h in heads]
    assert list(zip(heads.tolist(), sizes)) == sorted(rh.TIE_GROUPS[name])
    assert sorted(k for _, k in rh.TIE_GROUPS[name]) == [2, 3, 3, 70] or sorted(k for _, k in rh.TIE_GROUPS[name]) == [2, 2, 3, 70]
    assert heads[0] == 0 and heads[-1] + sizes[-1] == rh.TIE_N and any(h <= 2047 < 2048 < h + k for h, k in zip(heads, sizes))
    plain = rh.rebuild_host(cols, major, nodedup)
    tied = rh.rebuild_host(cols, major, nodedup, seqs.__getitem__, half.__getitem__)
    assert plain["n_ins_ties"] == sum(sizes) - len(sizes) and plain["n_out"] == rh.TIE_N - 250
    assert tied["n_tie_rows"] == sum(sizes) and 0 < tied["n_tie_dropped"] == plain["n_out"] - tied["n_out"]
    # the tie answer moves rows: in some group the settled order is not the stable one, and the aux word follows its row
    assert (tied["aux"] == cols["aux"][tied["src_row"]]).all()
    kept = np.isin(plain["src_row"], tied["src_row"])
    assert (plain["src_row"][kept] != tied["src_row"]).any()


# ================================================================================================ GPU
def run_case(ctx, monkeypatch, cols, major, nodedup, forced=False, tie=None, where=""):
    """one rebuild_columns call == the yardstick; the pass count and the route are the model's -> (layout, result)"""
    if forced:
        monkeypatch.setenv(ENV, "1")
    else:
        monkeypatch.delenv(ENV, raising=False)
    L = rh.key_layout(cols, major, forced)
    cb, kw = None, {}
    if tie is not None:
        seqs, half = tie
        cb = rebuild.tie_callback(seqs.__getitem__, half.__getitem__)
        kw = dict(seq_of_src=seqs.__getitem__, half_of_src=half.__getitem__)
    got = rebuild.rebuild_columns(ctx, cols["seg"], cols["a"], cols["b"], cols["rid"], cols["aux"], major, nodedup, tie_order=cb)
    assert got["n_passes"] == L["npass"], (where, got["n_passes"], L)
    assert rebuild.last_route(ctx) == L["route"], (where, rebuild.last_route(ctx), L)
    rh.assert_equal_to_host(got, rh.rebuild_host(cols, major, nodedup, **kw), where, ties=tie is not None)
    return L, got


@pytest.mark.gpu
def test_route_is_none_before_any_rebuild():
    with engine.Context(0) as c:
        assert rebuild.last_route(c) == _abi.RB_ROUTE_NONE


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(rh.LAYOUTS))
def test_gpu_layout_edges(ctx, monkeypatch, name):
    cols, major, nodedup, forced = rh.layout_case(name)
    L, _ = run_case(ctx, monkeypatch, cols, major, nodedup, forced, where=name)
    assert (L["route"], L["npass"]) == rh.LAYOUTS[name][3:5]


@pytest.mark.gpu
@pytest.mark.parametrize("at", rh.WIDEST_AT)
def test_gpu_widest_columns_maximum_at(ctx, monkeypatch, at):
    """k_pool_to_rows reduces the maxima per 2048-row block: a missed maximum truncates the key"""
    cols, major, nodedup, _ = rh.widest_case(at)
    L, _ = run_case(ctx, monkeypatch, cols, major, nodedup, where="widest at %d" % at)
    assert (L["route"], L["npass"]) == (PERM, 26)
    # the same row as the only wide one of the composite routes: every other row small
    for route in (COMPACT, WIDE):
        small, major, nodedup = rh.one_wide_row_case(at, route)
        L, _ = run_case(ctx, monkeypatch, small, major, nodedup, where="one wide row at %d" % at)
        assert L["route"] == route, L


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_gpu_tile_and_tail_seams(ctx, monkeypatch, route):
    for n in rh.SEAM_N:
        for kind in rh.SEAM_KINDS:
            cols, major, nodedup = rh.seam_case(kind, n)
            c, forced = on_route(cols, major, route)
            L, got = run_case(ctx, monkeypatch, c, major, nodedup, forced, where="%s n=%d" % (kind, n))
            assert L["route"] == route
            if kind == "same_dedup":
                assert got["n_out"] == 1
            if kind == "same_nodedup":
                assert np.array_equal(got["src_row"], np.arange(n))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", rh.SKEW_KINDS)
@pytest.mark.parametrize("route", (COMPACT, WIDE), ids=ROUTE_IDS[:2])
def test_gpu_digit_skew(ctx, monkeypatch, route, kind):
    cols, major, nodedup = rh.skew_case(kind, route)
    L, got = run_case(ctx, monkeypatch, cols, major, nodedup, where=kind)
    assert L["route"] == route and (got["n_out"] == L["n"] or kind == "alternate")


@pytest.mark.gpu
@pytest.mark.parametrize("n", rh.CARRY_N)
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_gpu_scan_carries(ctx, monkeypatch, route, n):
    """65 tiles: the row scan's offset crosses a wavefront; 257 tiles: it takes a second 256-unit step"""
    cols, major, nodedup = rh.carry_case(n)
    c, forced = on_route(cols, major, route, natural_perm=True)
    monkeypatch.delenv(ENV, raising=False)
    L = rh.key_layout(c, major)
    assert L["route"] == route and not forced
    got = rebuild.rebuild_columns(ctx, c["seg"], c["a"], c["b"], c["rid"], c["aux"], major, nodedup)
    assert got["n_passes"] == L["npass"] and rebuild.last_route(ctx) == route
    # (the padding of a route sets one bit of a and of b in every row: the order is the unpadded rows', sorted once for all routes)
    want = dict(rh.carry_host(n))
    for k in ("a", "b"):
        pad = int(c[k][0]) ^ int(cols[k][0])
        assert (c[k] == cols[k] | np.int64(pad)).all() and (pad == 0 or pad > int(cols[k].max()))
        want[k] = want[k] | np.int64(pad)
    rh.assert_equal_to_host(got, want, "n=%d" % n)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_gpu_ties_counted_without_a_callback(ctx, monkeypatch, route):
    for name in sorted(rh.TIE_GROUPS):
        cols, major, nodedup, seqs, half = rh.tie_case(name)
        c, forced = on_route(cols, major, route)
        L, got = run_case(ctx, monkeypatch, c, major, nodedup, forced, where=name)
        assert L["route"] == route and got["n_ins_ties"] == sum(k - 1 for _, k in rh.TIE_GROUPS[name])


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_gpu_ties_settled_by_the_callback(ctx, monkeypatch, route):
    for name in sorted(rh.TIE_GROUPS):
        cols, major, nodedup, seqs, half = rh.tie_case(name)
        c, forced = on_route(cols, major, route)
        L, got = run_case(ctx, monkeypatch, c, major, nodedup, forced, tie=(seqs, half), where=name)
        assert L["route"] == route and got["n_tie_rows"] == sum(k for _, k in rh.TIE_GROUPS[name]) and got["n_tie_dropped"] > 0


@pytest.mark.gpu
def test_gpu_ties_through_the_pool_on_the_wide_route(ctx, monkeypatch):
    """pool_append + rebuild_pool with read_rank: the pool's read indices become ranks on the device, the tie answer names pool rows"""
    monkeypatch.delenv(ENV, raising=False)
    cols, major, nodedup, seqs, half = rh.tie_case("g70_across")
    c = rh.to_route(cols, major, WIDE)
    rank = np.random.default_rng(3).permutation(8).astype(np.int32)
    read = np.argsort(rank).astype(np.int32)[c["rid"]]                # rank[read] == rid
    assert (rank[read] == c["rid"]).all() and (read != c["rid"]).any()
    rebuild.pool_reset(ctx)
    try:
        rebuild.pool_append(ctx, c["seg"][:1000], c["a"][:1000], c["b"][:1000], read[:1000], c["aux"][:1000])
        rebuild.pool_append(ctx, c["seg"][1000:], c["a"][1000:], c["b"][1000:], read[1000:], c["aux"][1000:])
        cb = rebuild.tie_callback(seqs.__getitem__, half.__getitem__)
        got = rebuild.rebuild_pool(ctx, rank, major, nodedup, keep_on_device=False, tie_order=cb)
    finally:
        rebuild.pool_reset(ctx)
    L = rh.key_layout(c, major)
    assert L["route"] == WIDE and got["n_passes"] == L["npass"] and rebuild.last_route(ctx) == WIDE
    rh.assert_equal_to_host(got, rh.rebuild_host(c, major, nodedup, seqs.__getitem__, half.__getitem__), "pool", ties=True)


@pytest.mark.gpu
def test_gpu_alternating_calls_on_one_context(monkeypatch):
    """what a larger call left behind - drop map, histograms, element buffers - does not leak into a smaller one"""
    with engine.Context(0) as c:
        big, major, nodedup = rh.carry_case(rh.CARRY_N[1])
        L, _ = run_case(c, monkeypatch, rh.to_route(big, major, WIDE), major, nodedup, where="257 tiles, wide")
        assert L["route"] == WIDE
        cols, major, nodedup = rh.seam_case("mixed", 65)
        assert run_case(c, monkeypatch, cols, major, nodedup, where="n=65")[0]["route"] == COMPACT
        cols, major, nodedup, seqs, half = rh.tie_case("g70_across")
        assert run_case(c, monkeypatch, cols, major, nodedup, True, tie=(seqs, half), where="forced permutation, ties")[0]["route"] == PERM
        cols, major, nodedup, seqs, half = rh.tie_case("g2_across")
        assert run_case(c, monkeypatch, cols, major, nodedup, tie=(seqs, half), where="compact, ties")[0]["route"] == COMPACT
        # (the drop map of the call before holds flags at these positions: a call without a callback must not read it)
        assert run_case(c, monkeypatch, cols, major, nodedup, where="compact, ties counted")[0]["route"] == COMPACT
        cols, major, nodedup = rh.seam_case("mixed", 1)
        assert run_case(c, monkeypatch, cols, major, nodedup, where="n=1")[0]["route"] == COMPACT


@pytest.mark.gpu
@pytest.mark.parametrize("what", ("negative a", "negative aux", "segment out of range", "pool read without a rank"))
def test_gpu_refusals_leave_the_context_usable(ctx, monkeypatch, what):
    monkeypatch.delenv(ENV, raising=False)
    cols, major, nodedup = rh.seam_case("mixed", 2049)
    bad = {k: v.copy() for k, v in cols.items()}
    with pytest.raises(engine.CsvError) as err:
        if what == "pool read without a rank":
            rebuild.pool_reset(ctx)
            try:
                bad["rid"][2048] = 3                                # (ranks are given for the reads 0, 1, 2 only)
                rebuild.pool_append(ctx, bad["seg"], bad["a"], bad["b"], bad["rid"], bad["aux"])
                rebuild.rebuild_pool(ctx, np.arange(3, dtype=np.int32), major, nodedup, keep_on_device=False)
            finally:
                rebuild.pool_reset(ctx)
        else:
            if what == "negative a":
                bad["a"][2048] = -1
            elif what == "negative aux":
                bad["aux"][2047] = -5
            else:
                bad["seg"][0] = len(major)
            rebuild.rebuild_columns(ctx, bad["seg"], bad["a"], bad["b"], bad["rid"], bad["aux"], major, nodedup)
    assert err.value.code == _abi.E_INVALID
    run_case(ctx, monkeypatch, cols, major, nodedup, where="after the refusal")
