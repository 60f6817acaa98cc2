"""Crafted batches for the chain kernels (k_chain_count / k_chain_apply / k_chain_ids) and a plain restatement of what they decide.

A case is a segment table plus the four signature columns, built directly (no SigStore), so that any number of segments of any type,
bias, read_count and chromosome can share a chain tile, and a break, a segment start, a position 0 or the end of the batch can be put
on a chosen offset of the layout: the byte of 8 signatures a lane owns, the 64-flag word, the 512-signature wavefront span, the
2048-signature tile, the halo row behind the tile and the rows behind that ("Chain seams").

restate() says, in Python ints and from the rules alone (INDEL:62-64, 80-86; sig_flag), which signature starts a cluster, which
clusters are work items and which tier bits they carry.  tile_records() says what the upload's per-tile records hold (how many
non-empty segments a tile overlaps and whether they are inline).  Every case carries the cells of the issue's list it claims and the
checks that show it lands where it says (check_landing)."""
import numpy as np

from cutesv_amd import _abi

BYTE, WORD, SPAN, TILE = 8, 64, 512, 2048
N = 4200                                                  # signatures of an ordinary case: two whole tiles and a third begun
SEAM_CLASSES = {"byte": tuple(range(1, 18)), "word": (63, 64, 65), "span": tuple(range(504, 521)), "tile": tuple(range(2040, 2057)),
                "halo_end": (2111, 2112, 2113), "tile2": (4095, 4096, 4097)}
SEAMS = tuple(o for c in SEAM_CLASSES.values() for o in c)
# offsets the many-break contents use: both sides of every seam kind, in every wavefront span of the first tile and in the rows behind it
MULTI = (1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 2047, 2048, 2049, 2111, 2112, 2113, 4095, 4096, 4097)
RCS = (1, 2, 3, 8, 9, 57, 58, 64, 65, 100)
SHIFT = (1 << 33) + 12345
PAIR = ("INV", "TRA")


def seam_class(o):
    for k, v in SEAM_CLASSES.items():
        if o in v:
            return k
    raise KeyError(o)


class Case:
    """name, family (1..7), group (the GPU tests' grain), segs: [dict(type, n, bias, rc, chrom, genotype)] in table order (their rows lie back to
    back), columns a / b / aux (int64 arrays; read_id is the row index), cells claimed, checks (check_landing), reads: None or
    (n_chrom, reads_off, r_start, r_end, r_primary, r_id), fits32 / only32"""

    def __init__(self, name, family, group, segs, a, b, aux, cells, checks, reads=None, only32=False):
        self.name, self.family, self.group, self.segs = name, family, group, segs
        self.a, self.b, self.aux = np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(aux, np.int64)
        self.cells, self.checks, self.reads, self.only32 = set(cells), list(checks), reads, only32
        self.rid = None                                      # read ids other than the row index (emit_helpers.EmitCase)
        n = len(self.a)
        assert sum(s["n"] for s in segs) == n == len(self.b) == len(self.aux), name
        lim = 1 << 31
        self.fits32 = bool(n == 0 or (self.a.min() >= -lim and self.a.max() < lim and self.b.min() >= -lim and self.b.max() < lim))
        assert self.fits32 or not only32

    @property
    def n_sig(self):
        return len(self.a)

    def bounds(self):
        """[(begin, end)] of the segments"""
        out, w = [], 0
        for s in self.segs:
            out.append((w, w + s["n"]))
            w += s["n"]
        return out

    def segment_table(self):
        recs = []
        for s, (beg, end) in zip(self.segs, self.bounds()):
            recs.append(_abi.make_segment(s["type"], s.get("chrom", 0), beg, end, s["bias"], s["rc"], diff_ratio=0.6 if s["type"] == "TRA" else 0.3,
                                          sv_size=30, genotype=s.get("genotype", False)))
        return np.array(recs, dtype=_abi.SEGMENT_DTYPE)

    def host_batch(self, narrow=False, copy=None, empty=None, gaps16=False):
        """the _abi.HostBatch of the case: int64 or (narrow) int32 position / length columns; copy / empty: where the columns live
        (engine.pinned_copy / engine.pinned_empty for page-locked ones); gaps16: the position column also as 16-bit gaps and the
        interleaved {b, read_id} rows beside it (what SigStore.pinned() hands a batch)"""
        assert self.fits32 or not narrow
        copy = copy or (lambda x: x)
        dt = np.int32 if narrow else np.int64
        a, b = copy(self.a.astype(dt)), copy(self.b.astype(dt))
        rid = copy(np.arange(self.n_sig, dtype=np.int32) if self.rid is None else np.ascontiguousarray(self.rid, np.int32))
        aux = copy(self.aux.astype(np.int32))
        kw = {}
        if self.reads is not None:
            n_chrom, off, rs, re, rp, ri = self.reads
            kw = dict(n_chrom=n_chrom, reads_off=off, r_start=copy(rs), r_end=copy(re), r_primary=copy(rp), r_id=copy(ri))
        if gaps16:
            assert narrow
            r8 = (empty or np.empty)((self.n_sig, 2), np.int32)
            r8[:, 0], r8[:, 1] = b, rid
            kw.update(a_delta=_abi.delta16_of(a, alloc=empty), rows8=r8)
        return _abi.HostBatch(self.segment_table(), a, b, rid, aux, per_sig=True, **kw)


# ------------------------------------------------------------------------------------------------ the plain restatement
def dropped(seg, reads):
    """a segment yields nothing when it is genotyped, is not TRA, and its chromosome has no reads block"""
    if not seg.get("genotype", False) or seg["type"] == "TRA":
        return False
    return reads is None or int(reads[1][seg.get("chrom", 0) + 1]) == int(reads[1][seg.get("chrom", 0)])


def tier_bits(svtype, size):
    """the tier bits of close_gate: tiny <= 16 and wide 33 .. 64 (DEL / INS only), big > 64"""
    bits = set()
    if size > 64:
        bits.add("big")
    if svtype in ("DEL", "INS"):
        if size <= 16:
            bits.add("tiny")
        if 33 <= size <= 64:
            bits.add("wide")
    return frozenset(bits)


def restate(case):
    """-> dict(flags: cluster starts, ascending; cluster_id: one int per signature; n_clusters; items: [(first, size, segment)] in order;
    tiers: one frozenset per item).  Python ints only."""
    a, b, x = case.a.tolist(), case.b.tolist(), case.aux.tolist()
    start = [False] * len(a)
    for s, (beg, end) in zip(case.segs, case.bounds()):
        bias, t = int(s["bias"]), s["type"]
        for i in range(beg, end):
            if i == beg:
                start[i] = True
            elif a[i] - a[i - 1] > bias or (a[i - 1] == 0 and b[i - 1] == 0):
                start[i] = True
            elif t == "INV" and (b[i] - b[i - 1] > bias or x[i] != x[i - 1]):
                start[i] = True
            elif t == "TRA" and x[i] != x[i - 1]:
                start[i] = True
    flags = [i for i, f in enumerate(start) if f]
    cid, c = [], -1
    for f in start:
        c += 1 if f else 0
        cid.append(c)
    items, tiers = [], []
    ends = flags[1:] + [len(a)]
    seg_of, bounds = 0, case.bounds()
    for first, nxt in zip(flags, ends):
        while not (bounds[seg_of][0] <= first < bounds[seg_of][1]):
            seg_of += 1
        s, size = case.segs[seg_of], nxt - first
        assert nxt <= bounds[seg_of][1]
        if size >= s["rc"] and not (a[nxt - 1] == 0 and b[nxt - 1] == 0) and not dropped(s, case.reads):
            items.append((first, size, seg_of))
            tiers.append(tier_bits(s["type"], size))
    return dict(flags=flags, cluster_id=cid, n_clusters=c + 1, items=items, tiers=tiers)


def tile_records(case):
    """per chain tile (first segment, last segment, non-empty segments overlapping it, inline count as the upload's tile record holds it:
    0 when there are more than three or one of the first three has a bias beyond 32 bits)"""
    bounds, out = case.bounds(), []
    for w0 in range(0, case.n_sig, TILE):
        w1 = min(w0 + TILE, case.n_sig) - 1
        over = [k for k, (beg, end) in enumerate(bounds) if end > beg and beg <= w1 and end - 1 >= w0]
        wide = any(not (-(1 << 31) <= int(case.segs[k]["bias"]) < (1 << 31)) for k in over[:3])
        out.append((over[0], over[-1], len(over), len(over) if len(over) <= 3 and not wide else 0))
    return out


def general_form(case, tile):
    """does k_chain_count take the general form for every span of the tile?  (no inline record, or an INV / TRA segment in it)"""
    k0, k1, n, nin = tile_records(case)[tile]
    bounds = case.bounds()
    inl = [k for k in range(k0, k1 + 1) if bounds[k][1] > bounds[k][0]][:3]
    return nin == 0 or any(case.segs[k]["type"] in PAIR for k in inl)


def assert_order(case):
    """the input order contract (k_validate_order): strictly increasing (a, b, read_id) inside a DEL / INS / DUP segment, (aux, a, b, read_id)
    inside an INV / TRA segment; read_id is the row index, so a tie of the other keys is in order already"""
    a, b, x = case.a, case.b, case.aux
    for s, (beg, end) in zip(case.segs, case.bounds()):
        if end - beg < 2:
            continue
        keys = [a[beg:end], b[beg:end]]
        if s["type"] in PAIR:
            keys.insert(0, x[beg:end])
        ok = np.zeros(end - beg - 1, bool)
        tie = np.ones(end - beg - 1, bool)
        for k in keys:
            d = np.diff(k)
            ok |= tie & (d > 0)
            tie &= d == 0
        assert bool((ok | tie).all()), (case.name, s["type"], int(np.flatnonzero(~(ok | tie))[0]) + beg + 1)


def check_landing(case, r):
    """every check of the case against the restatement r; returns how many were made"""
    a, b = case.a, case.b
    sizes = {f: s for f, s, _ in r["items"]}
    ends = dict(zip(r["flags"], r["flags"][1:] + [case.n_sig]))
    recs = tile_records(case)
    for chk in case.checks:
        kind, arg = chk[0], chk[1:]
        if kind == "flags":                                  # the cluster starts are exactly these
            assert r["flags"] == sorted(set(arg[0])), (case.name, r["flags"][:8], sorted(set(arg[0]))[:8])
        elif kind == "flag":                                 # w starts a cluster / does not
            assert (arg[0] in ends) == arg[1], (case.name, chk)
        elif kind == "items":                                # the work items are exactly these
            assert r["items"] == list(arg[0]), (case.name, r["items"][:6], list(arg[0])[:6])
        elif kind == "n_items":                              # the tile holds exactly this many work items
            assert sum(1 for f, _, _ in r["items"] if f // TILE == arg[0]) == arg[1], (case.name, chk)
        elif kind == "cluster":                              # a cluster starts at `first` and has `size` signatures; item: is it a work item?
            first, size, item = arg
            assert ends.get(first) == first + size and ((first in sizes) == item), (case.name, chk, ends.get(first))
        elif kind == "tier":
            first, want = arg
            assert r["tiers"][[f for f, _, _ in r["items"]].index(first)] == frozenset(want), (case.name, chk)
        elif kind == "end":                                  # where the cluster's end lies: inside its tile, in the halo row, or beyond it
            first, where = arg
            rel = ends[first] - (first // TILE + 1) * TILE
            assert ("tile" if rel < 0 else "halo" if rel < WORD else "far") == where, (case.name, chk, rel)
        elif kind == "nonempty":                             # non-empty segments overlapping the tile, and whether the record is inline
            tile, count, inline = arg
            assert recs[tile][2] == count and (recs[tile][3] > 0) == inline, (case.name, chk, recs[tile])
        elif kind == "general":
            assert general_form(case, arg[0]) == arg[1], (case.name, chk)
        elif kind == "seg_start":                            # a non-empty segment begins at w
            assert any(beg == arg[0] and end > beg for beg, end in case.bounds()), (case.name, chk)
        elif kind == "seg_type_at":
            k = [i for i, (beg, end) in enumerate(case.bounds()) if beg <= arg[0] < end][0]
            assert case.segs[k]["type"] == arg[1], (case.name, chk)
        elif kind == "zero":                                 # the row's position is 0; sentinel: and its length too
            w, sentinel = arg
            assert a[w] == 0 and (b[w] == 0) == sentinel, (case.name, chk)
        elif kind == "end_z":
            assert a[-1] == 0 and b[-1] == 0, case.name
        elif kind == "W":
            assert case.n_sig == arg[0], (case.name, chk)
        elif kind == "falls":                                # b falls at w and w starts no cluster
            assert b[arg[0]] < b[arg[0] - 1] and arg[0] not in ends, (case.name, chk)
        elif kind == "gap":                                  # a[w] - a[w - 1]
            assert int(a[arg[0]] - a[arg[0] - 1]) == arg[1], (case.name, chk)
        elif kind == "no_item_in":                           # the segments hold clusters of read_count signatures and more, yet no work item
            for k in arg[0]:
                beg, end = case.bounds()[k]
                big = [f for f, e in ends.items() if beg <= f < end and e - f >= case.segs[k]["rc"]]
                assert big and not any(s == k for _, _, s in r["items"]), (case.name, chk)
        else:
            raise KeyError(kind)
    return len(case.checks)


# ------------------------------------------------------------------------------------------------ column builders
def ramp(n, gap, other=None, start=1000):
    """positions start, start + gap, ...; other: {w: the gap in front of w}"""
    g = np.full(n, gap, np.int64)
    for w, v in (other or {}).items():
        if 0 < w < n:
            g[w] = v
    if n:
        g[0] = 0
    return start + np.cumsum(g)


def from_sizes(sizes, bias=50, start=1000):
    """consecutive clusters of the given sizes: the gap in front of a cluster's first row is bias + 1, every other gap is the bias"""
    first = np.cumsum([0] + list(sizes[:-1]))
    g = np.full(int(sum(sizes)), bias, np.int64)
    g[first] = bias + 1
    g[0] = 0
    return start + np.cumsum(g)


def cols(svtype, a):
    """b and aux that make every work item of the type a call: one length for DEL / INS (one allele; the INS sequence as long), an end /
    second position 500 behind the first for DUP / INV / TRA, aux 0 (TRA: type 0)"""
    a = np.asarray(a, np.int64)
    if svtype == "DEL":
        return np.full(len(a), 100, np.int64), np.zeros(len(a), np.int64)
    if svtype == "INS":
        return np.full(len(a), 100, np.int64), np.full(len(a), 100, np.int64)
    return a + 500, np.zeros(len(a), np.int64)


def seg(svtype, n, bias=50, rc=2, **kw):
    return dict(type=svtype, n=int(n), bias=bias, rc=rc, **kw)


def multi_ramp(n, small=40, wide=120, start=1000, at=MULTI):
    """one rising position column for several segments: every gap `small` except `wide` in front of the rows `at`"""
    return ramp(n, small, {w: wide for w in at}, start=start)


# ------------------------------------------------------------------------------------------------ family 1: one break at offset o
F1_KINDS = (("gap", "DEL"), ("gap", "INS"), ("gap", "DUP"), ("b", "INV"), ("aux", "INV"), ("aux", "TRA"))


def f1_case(kind, svtype, o, inverse, shifted=False):
    bias, n = 50, N
    form = "inverse" if inverse else "forward"
    checks = []
    if kind == "gap":
        jump = (1 << 35) if shifted else bias + 1
        a = ramp(n, bias + 1, {o: bias}) if inverse else ramp(n, bias, {o: jump})
        if inverse and shifted:
            a = ramp(n, bias + 1, {o: bias, o + 5: 1 << 35})
        b, aux = cols(svtype, a)
        size = 2
    elif kind == "b":
        a = ramp(n, 1)
        db = np.full(n, bias + 1 if inverse else bias, np.int64)
        fall = o + 1 if inverse else (o - 2 if o >= 3 else o + 2)
        db[o] = bias if inverse else ((1 << 35) if shifted else bias + 1)
        db[fall] = -30
        db[0] = 0
        b, aux = int(a[0]) + 500 + np.cumsum(db), np.zeros(n, np.int64)
        checks.append(("falls", fall))
        size = 3                                             # the row whose b falls joins the pair
    else:
        a = ramp(n, 1)
        b = a + 500
        chg = np.ones(n, np.int64) if inverse else np.zeros(n, np.int64)
        chg[o] = 0 if inverse else 1
        chg[0] = 0
        aux = 8 * np.cumsum(chg)
        size = 2
    if shifted:
        a = a + SHIFT
        if svtype != "DEL":
            b = b + SHIFT
    if inverse:
        checks += [("items", [(o - 1, size, 0)]), ("flag", o, False), ("flag", o - 1, True), ("flag", o + size - 1, True)]
    else:
        checks += [("flags", [0, o]), ("items", [(0, o, 0), (o, n - o, 0)])]
    label = "%s_%s_%s%s" % (kind, svtype, form, "_shifted" if shifted else "")
    return Case("f1_%s_%d" % (label, o), 1, "f1_" + label, [seg(svtype, n, bias, 2 if inverse else 1)], a, b, aux, {(1, label, o)}, checks)


def family1():
    for kind, t in F1_KINDS:
        for inverse in (False, True):
            for o in SEAMS:
                yield f1_case(kind, t, o, inverse)


# ------------------------------------------------------------------------------------------------ family 2: size against read_count
def f2_starts(rc):
    """(seam name, seam position, j) of the issue's list: starts at seam - j for j in {1, rc - 1, rc, rc + 1}; the 64-signature word seam is
    the one at 64 where the start fits in front of it and the one at 2048 + 64 (the halo row's end) where it does not"""
    for name, seam in (("tile", TILE), ("span", SPAN), ("word", WORD)):
        for j in sorted({1, rc - 1, rc, rc + 1}):
            pos = seam if seam - j >= 1 else TILE + seam
            yield name, pos, j


def family2():
    bias = 50
    for rc in RCS:
        for name, pos, j in f2_starts(rc):
            for size in (rc - 1, rc):
                if size == 0:                                # (read_count 1: there is no cluster of 0 signatures)
                    continue
                s = pos - j
                a = ramp(N, bias + 1, {w: bias for w in range(s + 1, s + size)})
                b, aux = cols("DEL", a)
                item = size >= rc
                checks = [("cluster", s, size, item), ("flag", s - 1, True), ("flag", s + size, True)]
                if rc > 1:                                   # (read_count 1: every singleton is a work item)
                    checks.append(("items", [(s, size, 0)] if item else []))
                which = "at" if item else "below"
                yield Case("f2_rc%d_%s_j%d_%s" % (rc, name, j, which), 2, "f2_%s" % name, [seg("DEL", N, bias, rc)], a, b, aux,
                           {(2, rc, name, j, which)}, checks)


# ------------------------------------------------------------------------------------------------ family 3: clusters that leave the tile
LEAVE_SIZES = (9, 64, 65, 129, 200, 2100)
END_W = (2111, 2112, 2113, 2175, 2176, 2177, 4159, 4160, 4161)
TIER_CUTS = (16, 17, 32, 33, 64, 65, 256, 257)


def sized_case(name, group, cells, sizes, checks, svtype="DEL", rc=2):
    a = from_sizes(sizes)
    b, aux = cols(svtype, a)
    return Case(name, 3, group, [seg(svtype, len(a), 50, rc)], a, b, aux, cells, checks)


def family3():
    for s in range(TILE - 8, TILE):
        for size in LEAVE_SIZES:
            where = "halo" if s + size - TILE < WORD else "far"
            yield sized_case("f3_leave_%d_%d" % (s, size), "f3_leave", {(3, "leave", s, size), (3, "end_" + where)}, [1] * s + [size] + [1] * (N - s - size),
                             [("items", [(s, size, 0)]), ("end", s, where)])
    for W in END_W:                                          # a cluster that runs to the end of the batch
        cell = {0: "mult64", 63: "below64", 1: "above64"}[W % 64]
        yield sized_case("f3_to_end_%d" % W, "f3_end", {(3, "to_end", cell), (3, "to_end_W", W)}, [1] * 2044 + [W - 2044],
                         [("items", [(2044, W - 2044, 0)]), ("W", W), ("end", 2044, "halo" if W - TILE < WORD else "far")])
    yield sized_case("f3_W2048", "f3_end", {(3, "W_exact", 2048)}, [1] * 2043 + [5], [("items", [(2043, 5, 0)]), ("W", 2048)])
    yield sized_case("f3_W4096", "f3_end", {(3, "W_exact", 4096)}, [1] * 4091 + [5], [("items", [(4091, 5, 0)]), ("W", 4096)])
    yield sized_case("f3_W4096_across", "f3_end", {(3, "W_exact_across", 4096)}, [1] * 2044 + [2052], [("items", [(2044, 2052, 0)]), ("W", 4096), ("end", 2044, "far")])
    for t in ("DEL", "INS"):
        for size in TIER_CUTS:
            want = tier_bits(t, size)
            yield sized_case("f3_tier_%s_%d" % (t, size), "f3_tier", {(3, "tier", t, size)}, [1] * 2040 + [size] + [1] * (N - 2040 - size),
                             [("items", [(2040, size, 0)]), ("tier", 2040, want), ("end", 2040, "halo" if size - 8 < WORD else "far")], svtype=t)


# ------------------------------------------------------------------------------------------------ family 4: segment starts
def f4_boundary(o, form):
    """two DEL segments that meet at o, positions continuing across; biases 50 | 200 (form A) or 200 | 50 (form B), read_count 2 | 3; a gap
    of 120 in front of o - 1 (inside the left segment) and in front of o + 1 (inside the right one): it breaks under 50 only"""
    b0, b1 = (50, 200) if form == "A" else (200, 50)
    other = {}
    if o >= 2:
        other[o - 1] = 120
    other[o + 1] = 120
    a = ramp(N, 40, other)
    b, aux = cols("DEL", a)
    flags = {0, o} | ({o - 1} if b0 == 50 and o >= 2 else set()) | ({o + 1} if b1 == 50 else set())
    checks = [("flags", flags), ("seg_start", o), ("gap", o, 40), ("gap", o + 1, 120)]
    return Case("f4_boundary_%s_%d" % (form, o), 4, "f4_boundary_" + form, [seg("DEL", o, b0, 2), seg("DEL", N - o, b1, 3)], a, b, aux, {(4, "boundary", form, o)}, checks)


def f4_many(lengths, name, cells, checks, types=("DEL", "INS", "DUP"), drop=(), rcs=(2, 3), at=MULTI, group="f4_segments"):
    """segments of the given lengths (0: an empty one) on one rising position column with a wide gap in front of every row of `at`;
    biases 50 / 200, read counts and types alternate over the non-empty ones; drop: indices of genotyped segments without a reads block"""
    n = sum(lengths)
    a = multi_ramp(n, at=at)
    b, aux, segs, w, q = np.zeros(n, np.int64), np.zeros(n, np.int64), [], 0, 0
    for k, ln in enumerate(lengths):
        t = types[q % len(types)]
        b[w:w + ln], aux[w:w + ln] = cols(t, a[w:w + ln])
        segs.append(seg(t, ln, (50, 200)[q % 2], rcs[q % len(rcs)], chrom=0, genotype=k in drop))
        w += ln
        q += 1 if ln else 0
    reads = None
    if drop:                                                 # chromosome 0 has no reads block, chromosome 1 has one
        reads = (2, np.array([0, 0, 4], np.int64), np.array([100, 200, 300, 400], np.int64), np.array([5000, 5100, 5200, 5300], np.int64),
                 np.ones(4, np.uint8), np.arange(4, dtype=np.int32))
    return Case(name, 4, group, segs, a, b, aux, cells, checks, reads=reads)


def family4():
    for form in ("A", "B"):
        for o in SEAMS:
            yield f4_boundary(o, form)
    # 1, 2, 3, 4 and 6 non-empty segments in the first tile, empty segments around and between them
    for k, lens in ((1, [N]), (2, [1000, N - 1000]), (3, [700, 700, N - 1400]), (4, [500, 500, 500, N - 1500]), (6, [300] * 5 + [N - 1500])):
        lengths = [0]
        for ln in lens:
            lengths += [ln, 0]
        yield f4_many(lengths, "f4_nonempty_%d" % k, {(4, "nonempty", min(k, 4))}, [("nonempty", 0, k, k <= 3), ("nonempty", 1, 1, True), ("general", 0, k > 3)])
    # the halo row's tile holds five segments while the first tile is inline: the row after the tile takes the segment table
    yield f4_many([2060, 500, 500, 500, N - 3560], "f4_halo_table", {(4, "halo_not_inline")}, [("nonempty", 0, 1, True), ("nonempty", 1, 5, False), ("seg_start", 2060)])
    yield f4_many([2047, 1, N - 2048], "f4_last_slot", {(4, "last_slot")}, [("seg_start", 2047), ("seg_start", 2048), ("cluster", 2047, 1, False), ("nonempty", 0, 2, True)])
    # a bias at and beyond the 32-bit limit of the inline record
    for label, bias in (("2p31m1", (1 << 31) - 1), ("2p31", 1 << 31), ("2p40", 1 << 40)):
        inline = bias < (1 << 31)
        for wide_gap in (False, True):                       # (the wide gaps need int64 columns)
            other = {w: 51 for w in MULTI if w > 2100}
            # (a gap equal to the bias stays inside its cluster; not under 2^40: refine's exact variance is stated for spreads below 2^31)
            other.update(({300: bias + 1, 600: bias} if bias < (1 << 32) else {300: bias + 1}) if wide_gap else {300: 120, 600: 1000})
            a = ramp(N, 40, other)
            b, aux = cols("DEL", a)
            flags = {0, 2100} | {w for w in MULTI if w > 2100} | ({300} if wide_gap else set())
            yield Case("f4_bias_%s_%s" % (label, "wide" if wide_gap else "narrow"), 4, "f4_bias", [seg("DEL", 2100, bias, 2), seg("DEL", N - 2100, 50, 2)], a, b, aux,
                       {(4, "bias", label, "int64_gap" if wide_gap else "fits32")}, [("flags", flags), ("nonempty", 0, 1, inline), ("nonempty", 1, 2, inline), ("general", 0, not inline)])
    # DEL + INV in one tile: every span of the tile takes the general form; the INV part breaks by aux and by b alone
    n_inv = N - 1000
    a = np.concatenate([ramp(1000, 40, {w: 120 for w in MULTI}), ramp(n_inv, 1, start=100000)])
    aux_at, b_at = (1024, 1535, 2047, 2048, 2049, 2112, 4096), (1536, 2111, 4095)
    chg, db = np.zeros(N, np.int64), np.full(N, 50, np.int64)
    chg[list(aux_at)] = 1
    db[list(b_at)] = 51
    b = np.concatenate([np.full(1000, 100, np.int64), 100500 + np.cumsum(db[1000:])])
    aux = np.concatenate([np.zeros(1000, np.int64), 8 * np.cumsum(chg[1000:])])
    flags = {0, 1000} | {w for w in MULTI if w < 1000} | set(aux_at) | set(b_at)
    yield Case("f4_del_inv_tile", 4, "f4_segments", [seg("DEL", 1000, 50, 2), seg("INV", n_inv, 50, 2)], a, b, aux, {(4, "del_inv_tile")},
               [("flags", flags), ("general", 0, True), ("nonempty", 0, 2, True)])
    # the halo row lies in an INV segment: the first tile is plain DEL (fast form), its last cluster runs into the row
    for cut in (2048, 2060):
        a = np.concatenate([from_sizes([1] * 2044 + [cut - 2044]), ramp(N - cut, 1, start=200000)])
        chg, db = np.zeros(N, np.int64), np.full(N, 50, np.int64)
        chg[[2070, 2112]] = 1
        db[[2100, 2111]] = 51
        b = np.concatenate([np.full(cut, 100, np.int64), 200500 + np.cumsum(db[cut:])])
        aux = np.concatenate([np.zeros(cut, np.int64), 8 * np.cumsum(chg[cut:])])
        yield Case("f4_halo_inv_%d" % cut, 4, "f4_segments", [seg("DEL", cut, 50, 2), seg("INV", N - cut, 50, 2)], a, b, aux, {(4, "halo_inv", cut)},
                   [("flags", set(range(2045)) | {cut, 2070, 2100, 2111, 2112}), ("seg_type_at", 2100, "INV"), ("general", 0, False), ("general", 1, True),
                    ("cluster", 2044, cut - 2044, True)])
    # a dropped segment beside a live one: inline (two segments in the tile) and with more than three
    fours = tuple(range(3, N, 4))                           # clusters of 4 under the bias of 50; the (dropped) segments of bias 200 are one cluster each
    yield f4_many([1000, N - 1000], "f4_drop_right", {(4, "drop", "inline")}, [("no_item_in", [1]), ("nonempty", 0, 2, True)], types=("DEL",), drop=(1,), rcs=(2,))
    yield f4_many([1000, N - 1000], "f4_drop_left", {(4, "drop", "inline")}, [("no_item_in", [0]), ("nonempty", 0, 2, True)], types=("DEL",), drop=(0,), rcs=(2,))
    yield f4_many([400, 400, 400, 400, N - 1600], "f4_drop_table", {(4, "drop", "table")}, [("no_item_in", [1, 3]), ("nonempty", 0, 5, False)], types=("DEL", "INS"), drop=(1, 3),
                  rcs=(2,), at=fours)


# ------------------------------------------------------------------------------------------------ family 5: position 0
ZERO_ROWS = {"sentinel1": [(0, 0)], "sentinel3": [(0, 0)] * 3, "length": [(0, 5), (0, 9)], "mixed": [(0, 0), (0, 0), (0, 3), (0, 7)], "negative": [(-3, 100), (0, 0)]}
ZERO_SPOTS = (("span0", 5), ("span1", 700), ("span2", 1100), ("span3", 1700), ("halo", 2050), ("left_of_span", None), ("left_of_halo", None))


def f5_case(name, cells, s, rows, rc=2, first_pos=10, n=N, extra=()):
    """a DEL segment of s ordinary rows, then a DEL segment that begins with `rows` [(a, b)] and goes on at first_pos; wide gaps at MULTI"""
    k = len(rows)
    a0 = ramp(s, 40, {w: 120 for w in MULTI})
    other = {w - s - k: 120 for w in MULTI if w - s - k > 0}
    a1 = ramp(n - s - k, 40, other, start=first_pos)
    a = np.concatenate([a0, [r[0] for r in rows], a1])
    b = np.full(n, 100, np.int64)
    b[s:s + k] = [r[1] for r in rows]
    checks = [("seg_start", s)] + [("zero", s + i, r[1] == 0) for i, r in enumerate(rows) if r[0] == 0] + list(extra)
    # the other wavefronts of the tile keep their flags: every MULTI offset outside the zero rows starts a cluster
    checks += [("flag", w, True) for w in MULTI if not (s <= w <= s + k) and w < n]
    return Case(name, 5, "f5_zero", [seg("DEL", s, 50, rc), seg("DEL", n - s, 50, rc)], a, b, np.zeros(n, np.int64), cells, checks)


def family5():
    for spot, s in ZERO_SPOTS:
        for label, rows in ZERO_ROWS.items():
            at = s
            if spot == "left_of_span":                       # the last row at position 0 is the row left of the second span
                last0 = max(i for i, r in enumerate(rows) if r[0] == 0)
                at = SPAN - 1 - last0
            if spot == "left_of_halo":
                last0 = max(i for i, r in enumerate(rows) if r[0] == 0)
                at = TILE - 1 - last0
            extra = []
            if spot.startswith("left_of"):
                extra.append(("zero", (SPAN if spot == "left_of_span" else TILE) - 1, rows[max(i for i, r in enumerate(rows) if r[0] == 0)][1] == 0))
            yield f5_case("f5_%s_%s" % (spot, label), {(5, spot, label)}, at, rows, extra=extra)
    # read_count 1: a (0,0) singleton yields nothing, a (0,1) singleton is a call
    for s in (5, TILE - 2, TILE - 1):
        yield f5_case("f5_rc1_%d" % s, {(5, "rc1", s)}, s, [(0, 0), (0, 1)], rc=1, first_pos=1000,
                      extra=[("cluster", s, 1, False), ("cluster", s + 1, 1, True)])
    # the batch's last segment is only (0,0) rows
    for W in (N, 2058, 2049, 2048, 2112, 2113):
        for k in (1, 3):
            body = W - k
            sizes = [3, 1] * (body // 4) + ([body % 4] if body % 4 else [])
            a = np.concatenate([from_sizes(sizes), np.zeros(k, np.int64)])
            b = np.concatenate([np.full(body, 100, np.int64), np.zeros(k, np.int64)])
            last = body - sizes[-1]
            yield Case("f5_end_z_%d_%d" % (W, k), 5, "f5_end", [seg("DEL", body, 50, 2), seg("DEL", k, 50, 1)], a, b, np.zeros(W, np.int64), {(5, "end_z", W, k)},
                       [("end_z",), ("W", W), ("no_item_in", [1]), ("cluster", W - 1, 1, False), ("cluster", last, sizes[-1], sizes[-1] >= 2)])
    # a cluster of negative positions that leaves the tile and ends, far behind the halo row, in a (0,0) row at the batch's end - or in a (0,5) row
    for label, lastb in (("sentinel", 0), ("length", 5)):
        a = np.concatenate([from_sizes([1] * 2040), -3000 + 10 * np.arange(299), [0]])
        b = np.full(2340, 100, np.int64)
        b[-1] = lastb
        yield Case("f5_far_end_%s" % label, 5, "f5_end", [seg("DEL", 2040, 50, 2), seg("DEL", 300, 50, 2)], a, b, np.zeros(2340, np.int64), {(5, "far_end", label)},
                   [("cluster", 2040, 300, lastb != 0), ("end", 2040, "far"), ("zero", 2339, lastb == 0)])


# ------------------------------------------------------------------------------------------------ family 6: widths
def family6():
    # int64 only: every position moved by 2^33 + 12 345, one gap of 2^35 (the DEL a-gap forms and the INV b-gap forms of family 1)
    for kind, t in (("gap", "DEL"), ("b", "INV")):
        for inverse in (False, True):
            for o in SEAMS:
                c = f1_case(kind, t, o, inverse, shifted=True)
                c.family, c.cells = 6, {(6, "shifted", kind, "inverse" if inverse else "forward", o)}
                c.group = "f6_shifted_%s_%s" % (kind, "inverse" if inverse else "forward")
                yield c
    # int32: positions 1 and 2^31 - 1 side by side, under a bias of 2^31 - 1 (no break) and of 100 (a break)
    top = (1 << 31) - 1
    for o in (1, 8, 64, 512, 2048):
        for bias in (top, 100):
            n = 2100
            a = np.concatenate([np.ones(o, np.int64), np.full(n - o, top, np.int64)])
            b, aux = cols("DEL", a)
            flags = [0] if bias == top else [0, o]
            yield Case("f6_top_%d_%s" % (o, "top" if bias == top else "100"), 6, "f6_top", [seg("DEL", n, bias, 1)], a, b, aux, {(6, "top", o, bias)},
                       [("flags", flags), ("gap", o, top - 1)])


# ------------------------------------------------------------------------------------------------ family 7: k_chain_apply
def f7_sizes_case(name, cells, sizes, checks, svtype="DEL", group="f7_apply"):
    a = from_sizes(sizes)
    b, aux = cols(svtype, a)
    return Case(name, 7, group, [seg(svtype, len(a), 50, 2)], a, b, aux, cells, checks)


def f7_tile_sizes(n_items):
    """cluster sizes that fill the first tile with exactly n_items work items of mixed tiers (read_count 2: singletons are none); the last one starts at
    2040 and, with 70 signatures, leaves the tile"""
    mix = [3, 17, 2, 33, 5, 16, 2, 3]                       # tiny, no bit, tiny, wide, ...
    sizes = [2] * (n_items - 1)
    total = sum(sizes)
    for i in range(len(sizes)):                             # as many of the mixed sizes as the tile has room for
        if total - 2 + mix[i % len(mix)] <= 2040:
            total += mix[i % len(mix)] - 2
            sizes[i] = mix[i % len(mix)]
    sizes += [1] * (2040 - sum(sizes)) + [70]
    return sizes + [1] * (N - sum(sizes))


def big_singletons(tiles, threes):
    """tiles * 2048 + 5 signatures, all singletons but clusters of 3 at the rows `threes`"""
    n = tiles * TILE + 5
    g = np.full(n, 51, np.int64)
    for w in threes:
        g[w + 1:w + 3] = 50
    g[0] = 0
    return 1000 + np.cumsum(g)


def family7():
    for n_items in (64, 65, 676):
        sizes = f7_tile_sizes(n_items)
        kinds = {frozenset(t) for t in (tier_bits("DEL", s) for s in sizes if s >= 2)}
        assert len(kinds) >= 3
        yield f7_sizes_case("f7_tile_%d" % n_items, {(7, "tile_items", n_items)}, sizes, [("n_items", 0, n_items), ("cluster", 2040, 70, True), ("tier", 2040, {"big"})])
    # nine tiles: the prefix of a tile spans more than one workgroup's four tiles
    rng_sizes = []
    k = 0
    while sum(rng_sizes) < 9 * TILE + 5 - 300:
        rng_sizes.append((1, 1, 3, 1, 17, 2, 1, 40, 1, 5, 90, 1, 1, 2)[k % 14] + (k % 3 == 0) * (k % 7))
        k += 1
    rng_sizes += [1] * (9 * TILE + 5 - sum(rng_sizes))
    yield f7_sizes_case("f7_nine_tiles", {(7, "nine_tiles")}, rng_sizes, [("W", 9 * TILE + 5)])


def big_case(tiles):
    """the large k_chain_apply shapes (int32 columns only): 2049 tiles + 5 signatures is the shape the issue names; 2052 tiles + 5 is the smallest whose
    last workgroup (tiles 2052 ..) sums tile counts in the loop past the first 2048"""
    threes = [(tiles - 2) * TILE + 100, (tiles - 2) * TILE + 2046, (tiles - 1) * TILE + 7, (tiles - 1) * TILE + 2040, tiles * TILE + 1]
    if tiles > 2049:
        threes = [2048 * TILE + 5, 2049 * TILE + 64, 2050 * TILE + 511, 2051 * TILE + 2046] + threes
    a = big_singletons(tiles, threes)
    b, aux = cols("DEL", a)
    return Case("f7_tiles_%d" % tiles, 7, "f7_big_%d" % tiles, [seg("DEL", len(a), 50, 2)], a, b, aux, {(7, "tiles", tiles)},
                [("items", [(w, 3, 0) for w in sorted(threes)]), ("W", tiles * TILE + 5)], only32=True)


# ------------------------------------------------------------------------------------------------ the registry
FAMILIES = {1: family1, 2: family2, 3: family3, 4: family4, 5: family5, 6: family6, 7: family7}
_INDEX = None


def index():
    """({group: [case names]}, the union of the cells the cases claim) of every ordinary case (the two large shapes come from big_case).  The
    cases themselves are not kept: cases_of builds a group's when a test asks for them."""
    global _INDEX
    if _INDEX is None:
        groups, cells, seen = {}, set(), set()
        for fam, gen in FAMILIES.items():
            for c in gen():
                assert c.name not in seen and c.cells and c.checks and c.family == fam and c.group.startswith("f%d_" % fam), c.name
                seen.add(c.name)
                groups.setdefault(c.group, []).append(c.name)
                cells |= c.cells
        _INDEX = (groups, cells)
    return _INDEX


def groups():
    return index()[0]


def cases_of(group):
    """the cases of one group, in order"""
    return [c for c in FAMILIES[int(group[1])]() if c.group == group]


def required_cells():
    """every (family, ...) cell the issue lists, written down independently of the builders"""
    need = set()
    for kind, t in F1_KINDS:
        for form in ("forward", "inverse"):
            need |= {(1, "%s_%s_%s" % (kind, t, form), o) for o in SEAMS}
    for rc in RCS:
        for name in ("tile", "span", "word"):
            for j in {1, rc - 1, rc, rc + 1}:
                need.add((2, rc, name, j, "at"))
                if rc > 1:
                    need.add((2, rc, name, j, "below"))
    need |= {(3, "leave", s, size) for s in range(2040, 2048) for size in LEAVE_SIZES} | {(3, "end_halo"), (3, "end_far")}
    need |= {(3, "to_end", c) for c in ("mult64", "below64", "above64")} | {(3, "W_exact", 2048), (3, "W_exact", 4096)}
    need |= {(3, "tier", t, size) for t in ("DEL", "INS") for size in TIER_CUTS}
    need |= {(4, "boundary", form, o) for form in ("A", "B") for o in SEAMS}
    need |= {(4, "nonempty", k) for k in (1, 2, 3, 4)} | {(4, "last_slot"), (4, "del_inv_tile"), (4, "halo_inv", 2048), (4, "drop", "inline"), (4, "drop", "table")}
    need |= {(4, "bias", label, "int64_gap") for label in ("2p31m1", "2p31", "2p40")} | {(4, "bias", label, "fits32") for label in ("2p31m1", "2p31", "2p40")}
    need |= {(5, spot, label) for spot, _ in ZERO_SPOTS for label in ("sentinel1", "sentinel3", "length", "mixed")}
    need |= {(5, "rc1", s) for s in (5, TILE - 2, TILE - 1)} | {(5, "end_z", W, k) for W in (N, 2048) for k in (1, 3)}
    need |= {(6, "shifted", kind, form, o) for kind in ("gap", "b") for form in ("forward", "inverse") for o in SEAMS}
    need |= {(6, "top", o, bias) for o in (1, 8, 64, 512, 2048) for bias in ((1 << 31) - 1, 100)}
    need |= {(7, "tile_items", 64), (7, "tile_items", 65), (7, "tile_items", 676), (7, "nine_tiles"), (7, "tiles", 2049), (7, "tiles", 2052)}
    return need
