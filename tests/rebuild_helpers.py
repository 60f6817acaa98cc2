"""The yardstick, the route model and the crafted columns of tests/test_rebuild_sort.py.

`rebuild_host` states what csv_rebuild_signatures computes in plain numpy and Python: a stable lexsort, the adjacent
de-duplication, the tie groups of the keep-every-row segments as a tuple sort.  `key_layout` does the host's arithmetic of
stage_rebuild.hip.h from the columns - field widths, route, passes, the bit offset and width of every digit inside the element -
so that every case can prove, without a GPU, which geometry it reaches.  The builders below make the cases from seeds."""
import functools

import numpy as np

COMPACT, WIDE, PERM = 1, 2, 3                     # csv_rebuild_route
ROUTE_NAME = {COMPACT: "compact", WIDE: "wide", PERM: "permutation"}
RS_BITS = 10                                      # sort.hip.h: bits of a composite-key digit
WTILE = 4096                                      # rows per wavefront tile of the radix passes (64 chunks of 64 rows)
COLS = ("seg", "a", "b", "rid", "aux")
DTYPE = dict(seg=np.int32, a=np.int64, b=np.int64, rid=np.int32, aux=np.int32)


def columns(seg, a, b, rid, aux):
    return dict(seg=np.asarray(seg, np.int32), a=np.asarray(a, np.int64), b=np.asarray(b, np.int64), rid=np.asarray(rid, np.int32), aux=np.asarray(aux, np.int32))


def flags(n_seg, major=(), nodedup=()):
    m, d = np.zeros(n_seg, np.uint8), np.zeros(n_seg, np.uint8)
    m[list(major)] = 1
    d[list(nodedup)] = 1
    return m, d


# ------------------------------------------------------------------------------------------------ the yardstick
def rebuild_host(cols, major, nodedup=None, seq_of_src=None, half_of_src=None):
    """-> dict(seg_id, a, b, read_id, aux, src_row, n_out, seg_count, n_ins_ties, n_tie_rows, n_tie_dropped).
    key(row) = (seg, aux if major[seg] else 0, a, b, rid); stable sort; in segments without `nodedup` a sorted row goes when
    (seg, a, b, rid, aux) equals that of the sorted row before it; `nodedup` segments keep every row and, with seq_of_src, every
    group of equal (seg, a, b, rid) is ordered by sequence (stably) and adjacent rows of equal (sequence, half) go."""
    seg, a, b, rid, aux = (np.asarray(cols[k]) for k in COLS)
    major = np.asarray(major, bool)
    nodedup = np.zeros(len(major), bool) if nodedup is None else np.asarray(nodedup, bool)
    n = len(a)
    auxk = np.where(major[seg], aux, 0)
    order = np.lexsort((rid, b, a, auxk, seg))                 # (the last key is the primary one; lexsort is stable)
    s, x, y, r, u = seg[order], a[order], b[order], rid[order], aux[order]
    same4 = np.zeros(n, bool)
    same4[1:] = (s[1:] == s[:-1]) & (x[1:] == x[:-1]) & (y[1:] == y[:-1]) & (r[1:] == r[:-1])
    same5 = same4.copy()
    same5[1:] &= u[1:] == u[:-1]
    nd = nodedup[s]
    keep = ~(same5 & ~nd)
    tie = same4 & nd                                           # position i continues the tie group of i - 1
    n_tie_rows = n_tie_dropped = 0
    if seq_of_src is not None:
        order = order.copy()
        starts = np.flatnonzero(tie & ~np.r_[False, tie[:-1]]) - 1
        for g0 in starts.tolist():
            g1 = g0 + 1
            while g1 < n and tie[g1]:
                g1 += 1
            rows = sorted((seq_of_src(src), k, src) for k, src in enumerate(order[g0:g1].tolist()))     # (k: equal sequences keep their order)
            prev = None
            for k, (sq, _, src) in enumerate(rows):
                cur = (sq, int(half_of_src(src)) if half_of_src is not None else 0)
                order[g0 + k] = src
                keep[g0 + k] = cur != prev
                n_tie_dropped += cur == prev
                prev = cur
            n_tie_rows += g1 - g0
        n_ins_ties = 0
    else:
        n_ins_ties = int(tie.sum())
    sel = order[keep]
    return dict(seg_id=seg[sel], a=a[sel], b=b[sel], read_id=rid[sel], aux=aux[sel], src_row=sel.astype(np.int32), n_out=len(sel),
                seg_count=np.bincount(seg[sel], minlength=len(major)).astype(np.int64), n_ins_ties=n_ins_ties, n_tie_rows=n_tie_rows,
                n_tie_dropped=int(n_tie_dropped))


RESULT_COLUMNS = ("seg_id", "a", "b", "read_id", "aux", "src_row", "seg_count")
RESULT_SCALARS = ("n_out", "n_ins_ties")


def assert_equal_to_host(got, want, where="", ties=False):
    """integer equality of everything the rebuild returns (src_row shows a stability error or the wrong survivor of a pair)"""
    for k in RESULT_SCALARS + (("n_tie_rows", "n_tie_dropped") if ties else ()):
        assert int(got[k]) == int(want[k]), "%s: %s is %d, the yardstick has %d" % (where, k, got[k], want[k])
    for k in RESULT_COLUMNS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, "%s: %s has %s entries, the yardstick %s" % (where, k, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, "%s: %s differs at %d places, first %s: got %s, want %s" % (where, k, len(bad), bad[:4], g[bad[:4]], w[bad[:4]])


# ------------------------------------------------------------------------------------------------ the route model
def _bits(v):
    return int(v).bit_length()


def _bytes(v):
    return (int(v).bit_length() + 7) // 8


def key_layout(cols, major, forced_perm=False):
    """the arithmetic of csv_rebuild_signatures from the columns: dict(n, ib, rb, bb, ab, xb, sb, pb, T, route, npass, digits);
    digits = [(s, dbits)] per pass of the composite routes, s = the digit's bit offset inside the element ([] for the
    permutation route: one pass per non-zero byte of read id, b, a, aux-as-key, and at least one of the segment)."""
    seg, a, b, rid, aux = (np.asarray(cols[k]) for k in COLS)
    n = len(a)
    is_major = np.asarray(major, bool)[seg]
    mx = dict(a=int(a.max()), b=int(b.max()), rid=int(rid.max()), seg=int(seg.max()), aux_all=int(aux.max()),
              aux=int(aux[is_major].max()) if is_major.any() else 0)
    L = dict(n=n, ib=max(1, _bits(n - 1)), rb=max(1, _bits(mx["rid"])), bb=max(1, _bits(mx["b"])), ab=max(1, _bits(mx["a"])), xb=_bits(mx["aux"]),
             sb=max(1, _bits(mx["seg"])), pb=_bits(mx["aux_all"]))
    T = L["T"] = L["rb"] + L["bb"] + L["ab"] + L["xb"] + L["sb"]
    if T > 128 or forced_perm:
        L["route"], L["digits"] = PERM, []
        L["npass"] = _bytes(mx["rid"]) + _bytes(mx["b"]) + _bytes(mx["a"]) + _bytes(mx["aux"]) + max(1, _bytes(mx["seg"]))
        return L
    compact = L["ib"] + T + L["pb"] <= 128 and L["ib"] + T < 128
    L["route"] = COMPACT if compact else WIDE
    L["digits"] = [(shift + (L["ib"] if compact else 0), min(RS_BITS, T - shift)) for shift in range(0, T, RS_BITS)]
    L["npass"] = len(L["digits"])
    assert L["npass"] == -(-T // RS_BITS)
    return L


def composite_keys(cols, major, L):
    """the T-bit key of every row as the composite routes pack it (Python integers): seg | aux of aux-major segments | a | b | rid"""
    seg, a, b, rid, aux = (np.asarray(cols[k]).tolist() for k in COLS)
    out = []
    for i in range(len(a)):
        k = seg[i]
        k = (k << L["xb"]) | (aux[i] if major[seg[i]] else 0)
        k = (k << L["ab"]) | a[i]
        k = (k << L["bb"]) | b[i]
        out.append((k << L["rb"]) | rid[i])
    return out


def pass_digits(cols, major, L):
    """the LSD passes of a composite route replayed on the host: per pass, the digit of every row in the order that pass meets them"""
    keys = composite_keys(cols, major, L)
    order = list(range(len(keys)))
    out = []
    for shift in range(0, L["T"], RS_BITS):
        mask = (1 << min(RS_BITS, L["T"] - shift)) - 1
        dig = [(keys[i] >> shift) & mask for i in order]
        out.append(dig)
        order = [i for _, i in sorted(zip(dig, order), key=lambda t: t[0])]
    return out


def probed_passes(cols, major, L, want):
    """per pass of a composite route: (pairs of neighbours in the sorted order `want` whose keys differ inside that pass's digit alone
    and whose input rows ascend, ... descend)"""
    keys = composite_keys(cols, major, L)
    src = want["src_row"].tolist()
    out = []
    for p in range(L["npass"]):
        lo, hi = p * RS_BITS, min(L["T"], (p + 1) * RS_BITS)
        inside = ((1 << hi) - 1) ^ ((1 << lo) - 1)
        up = down = 0
        for x, y in zip(src[:-1], src[1:]):
            d = keys[x] ^ keys[y]
            if d and not d & ~inside:
                up += x < y
                down += x > y
        out.append((up, down))
    return out


# ------------------------------------------------------------------------------------------------ crafted columns: layouts
def layout_columns(n, sb, xb, ab, bb, rb, pb, at=None, seed=0, dup=True):
    """n rows of random full-width values whose column maxima (2^bits - 1) all sit in row `at`; the aux payload's maximum, when it
    is wider than the aux-as-key field, sits in the row after it.  Odd segments sort on aux first when xb > 0; segments 2 mod 4
    keep every row.  An eighth of the other rows are copies of one another (half of them with another aux word), and every bit
    of the key below the segment has its probe pairs (below).
    -> (cols, major, nodedup)"""
    rng = np.random.default_rng(seed)
    at = n // 2 if at is None else at
    at_p = (at + 1) % n
    n_seg = 1 << sb

    def draw(bits, dtype):
        return rng.integers(0, max(1, (1 << bits) - 1), n, dtype=np.int64).astype(dtype)
    seg, a, b, rid = draw(sb, np.int32), draw(ab, np.int64), draw(bb, np.int64), draw(rb, np.int32)
    major = np.zeros(n_seg, np.uint8)
    if xb > 0:
        major[1::2] = 1
    nodedup = np.zeros(n_seg, np.uint8)
    nodedup[2::4] = 1
    aux = np.where(major[seg] != 0, draw(xb, np.int32), draw(pb, np.int32)).astype(np.int32)
    if dup and n > 16:
        free = np.setdiff1d(np.arange(n), [at, at_p])
        pick = rng.permutation(free)
        dst, src = pick[:n // 8], pick[n // 8:2 * (n // 8)]
        for col in (seg, a, b, rid, aux):
            col[dst] = col[src]
        other = dst[::2]                                       # (same key, another aux word: both rows stay in a de-duplicated segment)
        room = np.where(major[seg[other]] != 0, xb, pb) > 1
        aux[other] = np.where(room, np.where(aux[other] > 0, aux[other] - 1, aux[other] + 1), aux[other])
        # Probes: random full-width rows are told apart by their top dozen bits, so a wrong low digit would go unseen.  For every bit of
        # read id, b, a and the aux-as-key field, two pairs of rows that differ in that bit alone, the row with the bit flipped once
        # later and once earlier in the input: only the pass over that bit orders such a pair.
        spare = pick[2 * (n // 8):].tolist()
        for col, bits in ((rid, rb), (b, bb), (a, ab), (aux, xb)):
            for bit in range(bits):
                for flipped_later in (True, False):
                    lo, hi = sorted((spare.pop(), spare.pop()))
                    src, dst = (lo, hi) if flipped_later else (hi, lo)
                    if col is aux:                              # (aux is a key in odd segments only)
                        seg[src] |= 1
                        aux[src] = (aux[src] & ((1 << xb) - 1)) >> 1
                    for c in (seg, a, b, rid, aux):
                        c[dst] = c[src]
                    col[dst] ^= col.dtype.type(1 << bit)
    seg[at], a[at], b[at], rid[at] = n_seg - 1, (1 << ab) - 1, (1 << bb) - 1, (1 << rb) - 1
    aux[at] = (1 << xb) - 1 if xb > 0 else 0
    if pb > xb:
        seg[at_p], aux[at_p] = 0, (1 << pb) - 1
    elif xb == 0:
        aux[at] = (1 << pb) - 1
    return columns(seg, a, b, rid, aux), major, nodedup


# name: (n, (sb, xb, ab, bb, rb, pb), forced permutation sort) -> what the case claims: route, passes, last digit (s, dbits)
LAYOUTS = {
    "c53":          (4097, (10, 0, 12, 28, 3, 9), False, COMPACT, 6, (63, 3)),
    "c53_ib14":     (8200, (10, 0, 12, 28, 3, 9), False, COMPACT, 6, (64, 3)),
    "c51":          (4097, (10, 0, 12, 26, 3, 9), False, COMPACT, 6, (63, 1)),
    "c59_auxkey":   (4097, (10, 2, 14, 28, 5, 9), False, COMPACT, 6, (63, 9)),
    "c60_auxkey":   (4097, (10, 2, 15, 28, 5, 9), False, COMPACT, 6, (63, 10)),
    "c_sum128":     (4097, (20, 0, 40, 40, 6, 9), False, COMPACT, 11, (113, 6)),
    "w_sum129":     (4097, (20, 0, 41, 40, 6, 9), False, WIDE, 11, (100, 7)),
    "w_ibT128":     (4097, (20, 0, 45, 44, 6, 0), False, WIDE, 12, (110, 5)),
    "c_ibT127":     (4097, (20, 0, 44, 44, 6, 1), False, COMPACT, 12, (123, 4)),
    "w_T128":       (4097, (18, 2, 51, 51, 6, 9), False, WIDE, 13, (120, 8)),
    "p_T129":       (4097, (9, 1, 48, 47, 24, 9), False, PERM, 18, None),
    "p_forced_c53": (4097, (10, 0, 12, 28, 3, 9), True, PERM, 9, None),
}
WIDEST = (11, 31, 63, 63, 31, 31)                               # 2000-odd segments, every column at the width the ABI allows: 26 byte passes
WIDEST_AT = (0, 2047, 2048, 4096)


@functools.lru_cache(maxsize=None)
def layout_case(name):
    n, widths, forced, route, npass, last = LAYOUTS[name]
    cols, major, nodedup = layout_columns(n, *widths, at=(sorted(LAYOUTS).index(name) * 337) % n, seed=sorted(LAYOUTS).index(name) + 1)
    return cols, major, nodedup, forced


@functools.lru_cache(maxsize=None)
def widest_case(at):
    return layout_columns(4097, *WIDEST, at=at, seed=100 + at) + (False,)


@functools.lru_cache(maxsize=None)
def one_wide_row_case(at, route):
    """the widest case with every value cut to 3 bits but row `at`, which alone carries the widths of a compact (T = 4 + 4 + 40 + 40 + 6)
    or a wide (T = 128) call; its segment 15 sorts on aux first"""
    cols, major, nodedup, _ = widest_case(at)
    small = {k: (v & 7) for k, v in cols.items()}
    for k, bits in (("a", 40 if route == COMPACT else 60), ("b", 40 if route == COMPACT else 54), ("rid", 6), ("aux", 4), ("seg", 4)):
        small[k][at] = (1 << bits) - 1
    return small, major, nodedup


# ------------------------------------------------------------------------------------------------ crafted columns: routes by padding
def to_route(cols, major, route):
    """the same rows on another route: WIDE sets one high bit in every a and b so that T == 128 exactly (whatever the other
    columns hold), PERM one more bit (T == 129).  The order of the rows does not change; COMPACT returns the columns as they are."""
    if route == COMPACT:
        return cols
    L = key_layout(cols, major)
    rest = L["rb"] + L["xb"] + L["sb"]
    ab = 63
    bb = (128 if route == WIDE else 129) - rest - ab
    assert bb > L["bb"] and ab > L["ab"] and bb <= 63
    out = dict(cols)
    out["a"] = cols["a"] | np.int64(1 << (ab - 1))
    out["b"] = cols["b"] | np.int64(1 << (bb - 1))
    return out


# ------------------------------------------------------------------------------------------------ crafted columns: seams
SEAM_N = (1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 16383, 16384, 16385)
SEAM_KINDS = ("same_dedup", "same_nodedup", "pairs_121", "mixed")
SEAM_PAIRS = (64, 512, 2048)                                    # a full duplicate sits at sorted positions p - 1 | p
# segments of the seam and carry cases: 0 de-duplicated, 1 de-duplicated aux-major, 2 keep-every-row, 3 keep-every-row aux-major
SEAM_FLAGS = flags(4, major=(1, 3), nodedup=(2, 3))


def _shuffled(sorted_rows, seed):
    """rows given in their sorted order -> columns in a random input order that keeps rows of equal keys in the order given"""
    n = len(sorted_rows[0])
    rng = np.random.default_rng(seed)
    seg, a, b, rid, aux = (np.asarray(c) for c in sorted_rows)
    key_change = np.r_[True, (seg[1:] != seg[:-1]) | (a[1:] != a[:-1]) | (b[1:] != b[:-1]) | (rid[1:] != rid[:-1])]
    group = np.cumsum(key_change) - 1
    slot = rng.permutation(n)
    # inside every group of equal keys the input slots ascend with the sorted position: the stable sort gives this order back
    o = np.lexsort((slot, group))
    slot_sorted = slot[o]
    cols = {}
    for name, c in zip(COLS, (seg, a, b, rid, aux)):
        v = np.empty(n, DTYPE[name])
        v[slot_sorted] = c
        cols[name] = v
    return cols


@functools.lru_cache(maxsize=None)
def seam_case(kind, n):
    """-> (cols, major, nodedup) of few distinct values, so that equal keys lie on both sides of every seam"""
    major, nodedup = SEAM_FLAGS
    i = np.arange(n)
    if kind == "same_dedup":                                    # every row the same: one row survives
        return columns(np.zeros(n), np.full(n, 5), np.full(n, 7), np.full(n, 1), np.full(n, 3)), major, nodedup
    if kind == "same_nodedup":                                  # every row the same and kept: src_row == arange(n)
        return columns(np.full(n, 2), np.full(n, 5), np.full(n, 7), np.full(n, 1), np.full(n, 3)), major, nodedup
    if kind == "pairs_121":
        # sorted: groups of three equal keys with aux 1, 2, 1 in the de-duplicated segment 0 (not aux-major: all three stay) and,
        # at every p of SEAM_PAIRS, the row p a full copy of the row p - 1
        a, aux = i // 3, np.array([1, 2, 1])[i % 3]
        for p in SEAM_PAIRS:
            if p < n:
                a[p], aux[p] = a[p - 1], aux[p - 1]
        return _shuffled((np.zeros(n, np.int64), a, np.full(n, 7), np.full(n, 1), aux), 7 * n + 1), major, nodedup
    rng = np.random.default_rng(n)
    return columns(rng.integers(0, 4, n), rng.integers(5, 7, n), rng.integers(7, 9, n), rng.integers(0, 3, n), rng.integers(1, 4, n)), major, nodedup


# ------------------------------------------------------------------------------------------------ crafted columns: digit skew
SKEW_KINDS = ("one_bucket", "distinct64", "alternate")
SKEW_N = {"one_bucket": 4097, "distinct64": 1024, "alternate": 8192}
SKEW_WIDTHS = {COMPACT: (4, 16, 28, 12), WIDE: (6, 50, 48, 16)}    # sb, ab, bb, rb: T = 60 and 120 (no aux-major segment)


@functools.lru_cache(maxsize=None)
def skew_case(kind, route):
    """keys made digit by digit (10 bits at a time, least significant first) and cut into the fields:
    one_bucket: one key for every row (all bits set);  distinct64: digit d of row i = (2 d + 1) i mod 1024 with n = 1024, so every
    pass meets 64 different digits in every chunk of 64 rows;  alternate: digit d = all ones when bit d of i is set, with n = 2^13:
    pass d meets the rows ordered by the bits below d, so the two buckets alternate lane by lane in every pass."""
    sb, ab, bb, rb = SKEW_WIDTHS[route]
    T = sb + ab + bb + rb
    n = SKEW_N[kind]
    nd = T // RS_BITS
    assert nd * RS_BITS == T
    keys = []
    for i in range(n):
        if kind == "one_bucket":
            k = (1 << T) - 1
        elif kind == "distinct64":
            k = sum((((2 * d + 1) * i) % 1024) << (RS_BITS * d) for d in range(nd))
        else:
            k = sum(1023 << (RS_BITS * d) for d in range(nd) if (i >> d) & 1)
        keys.append(k)
    rid = [k & ((1 << rb) - 1) for k in keys]
    b = [(k >> rb) & ((1 << bb) - 1) for k in keys]
    a = [(k >> (rb + bb)) & ((1 << ab) - 1) for k in keys]
    seg = [k >> (rb + bb + ab) for k in keys]
    major, nodedup = flags(1 << sb)
    return columns(seg, a, b, rid, np.arange(n) % 2 + 1), major, nodedup          # (aux 1, 2, 1, 2, ...: equal keys all stay)


# ------------------------------------------------------------------------------------------------ crafted columns: scan carries
CARRY_N = (64 * WTILE + 1, 256 * WTILE + 1)                     # 65 tiles: the row scan's offset crosses a wavefront; 257: a second 256-unit step


@functools.lru_cache(maxsize=2)
def carry_case(n):
    """random rows over 4 segments, ~n / 2 distinct (a, b) so that duplicates and ties occur everywhere"""
    rng = np.random.default_rng(n)
    major, nodedup = SEAM_FLAGS
    return columns(rng.integers(0, 4, n), rng.integers(0, 1 << 14, n), rng.integers(0, 1 << 5, n), rng.integers(0, 2, n), rng.integers(1, 3, n)), major, nodedup


@functools.lru_cache(maxsize=2)
def carry_host(n):
    cols, major, nodedup = carry_case(n)
    return rebuild_host(cols, major, nodedup)


# ------------------------------------------------------------------------------------------------ crafted columns: ties
TIE_N = 4097
# (first sorted position, rows) of the tie groups: 2, 3 and 70 rows (70: longer than a chunk), at position 0, at n - 1, across 2047 | 2048
TIE_GROUPS = {"g70_across": ((0, 2), (300, 3), (2010, 70), (TIE_N - 3, 3)),
              "g2_across": ((0, 70), (300, 3), (2047, 2), (TIE_N - 2, 2)),
              "g3_across": ((0, 3), (300, 2), (2046, 3), (TIE_N - 70, 70))}


TIE_FLAGS = flags(3, major=(1, 2), nodedup=(0, 2))


@functools.lru_cache(maxsize=None)
def tie_case(name):
    """sorted: keep-every-row segment 0 over [0, 1000), de-duplicated segment 1 (aux-major) over [1000, 1500) in full duplicate pairs,
    keep-every-row segment 2 (aux-major) from 1500 on; distinct keys but for the tie groups; every row its own aux word (it has to
    follow the row through the tie answer) except where it is a key.  -> (cols, major, nodedup, seqs, half)"""
    n = TIE_N
    major, nodedup = TIE_FLAGS
    i = np.arange(n)
    seg = np.where(i < 1000, 0, np.where(i < 1500, 1, 2))
    a = 2 * i
    aux = 1 + i % 500
    mid = (i >= 1000) & (i < 1500)
    a[mid] = 2 * (i[mid] // 2 * 2)
    aux[mid] = 7
    rid = i % 3
    rid[mid] = (i[mid] // 2) % 3
    aux[i >= 1500] = 5                                          # (aux-major and kept: aux is a key there)
    for g0, k in TIE_GROUPS[name]:
        a[g0:g0 + k], rid[g0:g0 + k] = a[g0], rid[g0]
    cols = _shuffled((seg, a, np.full(n, 9), rid, aux), 11)
    rng = np.random.default_rng(5)
    seqs = [("A", "C", "AC", "")[v] for v in rng.integers(0, 4, n)]      # by input row: few values, so equal (sequence, half) pairs occur
    half = rng.integers(0, 2, n).astype(np.uint8)
    return cols, major, nodedup, seqs, half


# ------------------------------------------------------------------------------------------------ the reference's recorded cases
def golden_case_columns(case):
    """a rebuild_order.json.gz case -> (cols, major, nodedup, seqs by input row, half by input row, rows: [(type, tuple)] by input row)"""
    from cutesv_amd import rebuild
    from cutesv_amd.columns import intern_names, BND_CODE, TYPES
    from helpers import rebuild_case_inputs
    per, reads = rebuild_case_inputs(case)
    chroms = sorted({x[-1] for t in per for x in per[t]} | {x[2] for x in per["TRA"]} | {r[-1] for r in reads})
    cidx = {c: i for i, c in enumerate(chroms)}
    npos = {"DEL": 2, "INS": 2, "DUP": 2, "INV": 3, "TRA": 4}
    uniq, _ = intern_names([x[npos[t]] for t in per for x in per[t]] + [r[3] for r in reads])
    rank = {nm: i for i, nm in enumerate(uniq)}
    strands = sorted({x[0] for x in per["INV"]})
    order, crank, major, nodedup = rebuild._segments(chroms, True)
    seg, a, b, rid, aux, seqs, half, rows = [], [], [], [], [], [], [], []
    for ti, t in enumerate(TYPES):
        for x in per[t]:
            seg.append(ti * len(chroms) + int(crank[cidx[x[-1]]]))
            rid.append(rank[x[npos[t]]])
            if t in ("DEL", "DUP", "INS"):
                a.append(int(x[0])); b.append(int(x[1])); aux.append(len(x[3]) if t == "INS" else 0)
            elif t == "INV":
                a.append(int(x[1])); b.append(int(x[2])); aux.append(strands.index(x[0]))
            else:
                a.append(int(x[1])); b.append(int(x[3])); aux.append(cidx[x[2]] * 8 + BND_CODE[x[0]])
            seqs.append(x[3] if t == "INS" else "")
            half.append(int(t == "INS" and x[0] != int(x[0])))
            rows.append((t, x))
    return columns(seg, a, b, rid, aux), major, nodedup, seqs, half, rows
