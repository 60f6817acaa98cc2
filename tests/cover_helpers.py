"""Helpers of tests/test_genotype_cover.py: a brute-force statement of the genotype cover (no index of any kind), a CPU model
of the ROUTE k_genotype takes through its three-level index and its hash-set tiers (so that a table can assert the geometry it
claims), and the builders of the crafted reads tables.

A call is a cluster of `k` identical DEL / INS signatures (or DUP / INV pairs) with distinct read names at one position, which
puts the call's genotype window exactly where a case wants it: DEL [pos - bias, pos + bias], INS [pos - 1000, pos + 1000],
DUP / INV two windows of half-width nb / 2 around the two breakpoints (x.5 bounds when nb is odd)."""
import dataclasses
import functools

import numpy as np

from cutesv_amd import _abi, genotype, synth
from cutesv_amd.columns import Params, SigStore

PARAMS = Params(min_support=3, genotype=True, max_cluster_bias_DEL=100, max_cluster_bias_INS=100, max_cluster_bias_INV=501,
                max_cluster_bias_DUP=500)
BIAS = 100                    # half-width of a DEL window under PARAMS
INS_HALF = 1000               # ... of an INS window (INDEL:451)
GT2_WAVES = 1024              # wavefronts of the second genotype pass: one slice of the global pool each
INT32_MAX = (1 << 31) - 1


# ------------------------------------------------------------------------------------------------ the yardstick
def windows2(params, svtype, bp1, bp2, search_pos):
    """the one or two genotype windows of a call as (L2, R2) in doubled coordinates (INDEL:450-451, DUP:146-151, INV:218-221)"""
    if svtype in (_abi.DEL, _abi.INS):
        half = params.max_cluster_bias_DEL if svtype == _abi.DEL else INS_HALF
        return [(2 * max(search_pos - half, 0), 2 * (search_pos + half))]
    nb = params.max_cluster_bias_DUP if svtype == _abi.DUP else params.max_cluster_bias_INV
    if svtype == _abi.DUP:
        nb = min(nb, bp2 - bp1)
    return [(max(2 * bp - nb, 0), 2 * bp + nb) for bp in (bp1, bp2)]


def genotyped_calls(params, segments, result):
    """[(call, chromosome, windows)] of every genotyped DEL / INS / DUP / INV call of a trimmed result"""
    out = []
    for c in range(len(result["call_seg"])):
        sg = segments[int(result["call_seg"][c])]
        t = int(sg["svtype"])
        if not sg["genotype"] or t == _abi.TRA:
            continue
        out.append((c, int(sg["chrom"]), windows2(params, t, int(result["bp1"][c]), int(result["bp2"][c]), int(result["search_pos"][c]))))
    return out


def cover_ids(store, chrom, L2, R2):
    """distinct ids of the primary rows of the chromosome with 2 start <= L2 and 2 end >= R2: every row looked at"""
    lo, hi = int(store.reads_off[chrom]), int(store.reads_off[chrom + 1])
    m = (store.r_primary[lo:hi] == 1) & (2 * store.r_start[lo:hi].astype(np.int64) <= L2) & (2 * store.r_end[lo:hi].astype(np.int64) >= R2)
    return np.unique(store.r_id[lo:hi][m])


def brute_dr(store, params, segments, result):
    """(DR, DV, gl_idx) of every genotyped non-TRA call, recomputed from the whole table -> dict(call=, dr=, dv=, gl_idx=, cover=
    [distinct covering ids per window])"""
    calls, dr, dv, gl, cover = [], [], [], [], []
    off, sig = result["support_off"], result["support_sig"]
    for c, chrom, wins in genotyped_calls(params, segments, result):
        per_win = [cover_ids(store, chrom, L2, R2) for L2, R2 in wins]
        ids = per_win[0] if len(per_win) == 1 else np.union1d(per_win[0], per_win[1])
        support = store.read_id[sig[int(off[c]):int(off[c + 1])]]
        d, v = int((~np.isin(ids, support)).sum()), int(off[c + 1] - off[c])
        calls.append(c); dr.append(d); dv.append(v); gl.append(genotype.gl_index(d, v)); cover.append(per_win)
    return dict(call=np.array(calls, np.int64), dr=np.array(dr, np.int64), dv=np.array(dv, np.int64), gl_idx=np.array(gl, np.int64), cover=cover)


def assert_brute_equal(brute, got):
    """every genotyped non-TRA call: the result's dr / dv / gl_idx are the brute-force ones (integer equality)"""
    c = brute["call"]
    for f in ("dr", "dv", "gl_idx"):
        g = np.asarray(got[f])[c].astype(np.int64)
        assert np.array_equal(g, brute[f]), "%s differs from the brute force at calls %s: got %s, want %s" % (
            f, c[g != brute[f]][:8], g[g != brute[f]][:8], brute[f][g != brute[f]][:8])


# ------------------------------------------------------------------------------------------------ the route, modelled on the CPU
def device_maxlen(store, chrom):
    """the chromosome's longest read as k_reads_maxlen bounds it: the maximum over the 512-row spans that hold a row of it
    (a span shared with a neighbour counts for both), non-primary rows included"""
    r0, r1 = int(store.reads_off[chrom]), int(store.reads_off[chrom + 1])
    if r1 <= r0:
        return 0
    lo, hi = (r0 >> 9) << 9, min((((r1 - 1) >> 9) + 1) << 9, store.n_reads)
    return int(np.maximum(store.r_end[lo:hi] - store.r_start[lo:hi], 0).max())


def walk(store, chrom, L2, R2):
    """cover_window's steps (1) and (2) on the start-sorted table -> dict(k0, k1, ktop, iters1 = bfirst loads of step (1), steps2 =
    iterations of step (2), closed = "c0" | "before" | "empty")"""
    st = store.r_start
    r0, r1 = int(store.reads_off[chrom]), int(store.reads_off[chrom + 1])
    Lh, Fh = L2 >> 1, (R2 - 2 * device_maxlen(store, chrom) + 1) >> 1
    c0, c1 = r0 >> 6, (r1 - 1) >> 6
    k0, k1 = c0 >> 6, c1 >> 6
    ktop, iters1 = k0, 0
    for kb in range(k0, k1 + 1, 128):
        iters1 += 1
        ks = np.arange(kb, min(kb + 128, k1 + 1))
        nn = int(((ks == k0) | (st[ks << 12] <= Lh)).sum())
        if nn == 0:
            break
        ktop = kb + nn - 1
        if nn < 128:
            break
    steps2, closed, kk = 0, None, ktop
    while kk >= k0:
        steps2 += 1
        two = 1 if kk > k0 else 0
        cb = (kk - two) << 6
        lo_c, hi_c = max(cb, c0), min(cb + 63 + (two << 6), c1)
        cs = np.arange(lo_c, hi_c + 1)
        first = st[cs << 6]
        if kk == ktop and not ((cs == c0) | (first <= Lh)).any():
            closed = "empty"
            break
        if ((cs > c0) & (first < Fh)).any():
            closed = "before"
            break
        if lo_c == c0:
            closed = "c0"
            break
        kk -= 2
    return dict(k0=k0, k1=k1, ktop=ktop, iters1=iters1, steps2=steps2, closed=closed)


def scan_rows(store, chrom, L2, R2):
    """rows of the chromosome with R - maxlen <= start <= L: window_range's top - bot + 1, and the range step (2) has to close"""
    r0, r1 = int(store.reads_off[chrom]), int(store.reads_off[chrom + 1])
    s2 = 2 * store.r_start[r0:r1]
    top = int(np.searchsorted(s2, L2, side="right"))
    bot = int(np.searchsorted(s2, R2 - 2 * device_maxlen(store, chrom), side="left"))
    return max(top - bot, 0)


def pool_ints(store, hb):
    """the global hash pool's size as the upload plans it: a power of two >= 2 (2 longest reads block + longest genotyped segment) + 4096"""
    rc_max = int(np.diff(store.reads_off).max())
    sg = hb.segments
    gt = (sg["genotype"] != 0) & (sg["svtype"] != _abi.TRA)
    maxseg = int((sg["sig_end"] - sg["sig_begin"])[gt].max()) if gt.any() else 0
    n = 1 << 20
    while n < 2 * (2 * rc_max + maxseg) + 4096:
        n <<= 1
    return n


def fits_slice(store, hb, chrom, wins, n_support):
    """genotype_global's size test for one wavefront's slice of the pool: need = supports + scan rows of the window(s), table =
    the power of two >= 2 need (at least 1024)"""
    need = n_support + sum(scan_rows(store, chrom, L2, R2) for L2, R2 in wins)
    bits = 10
    while (1 << bits) < 2 * need:
        bits += 1
    return (1 << bits) <= pool_ints(store, hb) // GT2_WAVES


# ------------------------------------------------------------------------------------------------ table builder
class Table:
    """reads and calls collected per chromosome -> SigStore.  Read ids: a support read gets the rank of its name among the
    signatures' names (SigStore.from_tuple_lists), which is its creation index here; a row of the reads table either names one of
    those or gets a fresh id above all of them."""

    def __init__(self, chroms, shift=0):
        self.chroms, self.shift = list(chroms), int(shift)
        self.per = {t: [] for t in ("DEL", "INS", "DUP", "INV", "TRA")}
        self.rows = {c: [] for c in self.chroms}
        self.n_support = self.n_fresh = 0
        self.placed = 0                                   # calls placed: the least number of genotyped calls of the table

    def reads(self, chrom, start, end, primary=1, ids=None):
        """rows of one chromosome (arrays or scalars broadcast against `start`); ids None: fresh ids, one per row -> their codes"""
        start = np.atleast_1d(np.asarray(start, np.int64))
        end = np.broadcast_to(np.asarray(end, np.int64), start.shape)
        primary = np.broadcast_to(np.asarray(primary, np.uint8), start.shape)
        if ids is None:
            ids = -1 - (self.n_fresh + np.arange(len(start), dtype=np.int64))          # (resolved in store(): above every support id)
            self.n_fresh += len(start)
        ids = np.broadcast_to(np.asarray(ids, np.int64), start.shape)
        assert (end >= start).all()
        self.rows[chrom].append((start, end, primary, ids))
        return ids

    def _names(self, k):
        ids = list(range(self.n_support, self.n_support + k))
        self.n_support += k
        self.placed += 1
        return ids

    def call(self, chrom, pos, svtype="DEL", k=3):
        """k identical DEL / INS signatures at `pos` -> the support read ids"""
        ids = self._names(k)
        p = int(pos) + self.shift
        for j in ids:
            self.per[svtype].append((p, 50, "s%08d" % j, "DEL", chrom) if svtype == "DEL" else (p, 50, "s%08d" % j, "A" * 50, "INS", chrom))
        return ids

    def pair(self, chrom, p1, p2, svtype="INV", k=3):
        """k identical DUP / INV signatures with the breakpoints p1 < p2 -> the support read ids"""
        ids = self._names(k)
        a, b = int(p1) + self.shift, int(p2) + self.shift
        for j in ids:
            self.per[svtype].append((a, b, "s%08d" % j, "DUP", chrom) if svtype == "DUP" else ("++", a, b, "s%08d" % j, "INV", chrom))
        return ids

    def sorted_starts(self, chrom):
        """the chromosome's start column as the table will hold it (unshifted), to place windows by row"""
        return np.sort(np.concatenate([r[0] for r in self.rows[chrom]]), kind="stable")

    def store(self):
        st = SigStore.from_tuple_lists(self.per, chroms=self.chroms)
        assert st.n_sig == self.n_support and np.array_equal(np.sort(st.read_id), np.arange(self.n_support))
        off, cols = [0], [[], [], [], []]
        for c in self.chroms:
            if self.rows[c]:
                blk = [np.concatenate([r[i] for r in self.rows[c]]) for i in range(4)]
                o = np.argsort(blk[0], kind="stable")
                for i in range(4):
                    cols[i].append(blk[i][o])
            off.append(off[-1] + sum(len(r[0]) for r in self.rows[c]))
        s, e, p, i = [np.concatenate(x) if x else np.zeros(0, np.int64) for x in cols]
        i = np.where(i < 0, self.n_support + (-1 - i), i)
        return dataclasses.replace(st, reads_off=np.array(off, np.int64), r_start=s + self.shift, r_end=e + self.shift,
                                   r_primary=p.astype(np.uint8), r_id=i.astype(np.int32))


def in_extraction_order(st, seed=7):
    """the table as cuteSV's extraction leaves it: eight task regions over the chromosomes' extent, dealt to three workers
    -> (store, the CSV_READS_GAP that goes with regions of this width: half a region; 1 Mbp goes with the 10 Mbp of production)"""
    lo, hi = int(st.r_start.min()), int(st.r_start.max())
    region = max((hi - lo) // 8, 2)
    runs, _ = synth.extraction_order(st, seed=seed, region=region, workers=3)
    return runs, region // 2


RO_TILE, RO_TCAP, RO_CAP = 2048, 32, 4096     # the reads-order stage: rows per tile, run starts a tile may hold, runs it plans


def run_plan(st, gap):
    """k_reads_runs + k_reads_plan on the CPU: cut every chromosome block where a start descends or jumps ahead by more than `gap`,
    order the runs of a chromosome by (first start, position) and check that they do not interleave -> dict(runs, moved = a run
    changes place, ok = the stage moves whole runs (else the host repeats the batch through the general sort), why)"""
    s = st.r_start
    n = len(s)
    cut = np.zeros(n, bool)
    cut[1:] = (s[1:] < s[:-1]) | (s[1:] - s[:-1] > gap)
    off = st.reads_off
    cut[off[:-1][off[:-1] < n]] = False                     # (a block start is a run start of the plan's own)
    per_tile = np.bincount(np.flatnonzero(cut) // RO_TILE, minlength=1)
    if per_tile.max() > RO_TCAP:
        return dict(runs=int(cut.sum()), moved=False, ok=False, why="more than %d run starts in a tile" % RO_TCAP)
    at = np.flatnonzero(cut)
    if ((s[at] >= 1 << 32) | (s[at] < 0) | (s[at - 1] >= 1 << 32) | (s[at - 1] < 0)).any():
        return dict(runs=int(cut.sum()), moved=False, ok=False, why="a run boundary outside [0, 2^32)")
    runs, moved = 0, False
    for c in range(len(off) - 1):
        lo, hi = int(off[c]), int(off[c + 1])
        if hi <= lo:
            continue
        beg = np.r_[lo, lo + 1 + np.flatnonzero(cut[lo + 1:hi])]
        end = np.r_[beg[1:], hi]                              # (exclusive)
        order = np.lexsort((beg, s[beg]))
        runs += len(beg)
        moved = moved or not np.array_equal(order, np.arange(len(beg)))
        last_prev, first = s[end[order[:-1]] - 1], s[beg[order[1:]]]
        if ((last_prev > first) | ((last_prev == first) & (order[:-1] > order[1:]))).any():
            return dict(runs=runs, moved=moved, ok=False, why="the runs of chromosome %d interleave" % c)
    if runs > RO_CAP:
        return dict(runs=runs, moved=moved, ok=False, why="more than %d runs" % RO_CAP)
    return dict(runs=runs, moved=moved, ok=True, why="")


def _front(T, chrom="f0"):
    """100 short reads in front of the table: the next chromosome begins inside a chunk, a block and a 512-row span"""
    T.reads(chrom, 1000 + 50 * np.arange(100), 2000 + 50 * np.arange(100))


# (a) ------------------------------------------------------------------------------------------- the walk of step (2)
WALK_N, WALK_STEP, WALK_LEN, WALK_BASE = 40960, 100, 3000, 10_000
WALK_SHIFT = (1 << 33) + 12345


def walk_table(kind, shift=0):
    """One chromosome of 40 960 reads (10 blocks of its own, 11 touched), evenly spaced, ~28 deep, behind 100 reads of another.
    kind "span": one primary read over the whole contig (F <= 0: every window walks down to the chromosome's first chunk);
    "middle": the long read covers the middle 20 000 reads (windows above it close by a chunk that begins before F, in a middle
    step); "nonprimary": the whole-contig read is non-primary (it widens every scan and covers nothing).
    -> (store, dict(rows = global rows whose start is a window's L, placed = calls placed))"""
    T = Table(["f0", "w"], shift=shift)
    _front(T)
    n = WALK_N - 1
    starts = WALK_BASE + WALK_STEP * np.arange(n)
    T.reads("w", starts, starts + WALK_LEN)
    if kind == "middle":
        T.reads("w", starts[10000] + 1, starts[30000])
        rows = [5000, 20000, 30500, 35000, 39000]
    else:
        T.reads("w", WALK_BASE - 1, starts[-1] + WALK_LEN + 1000, primary=1 if kind == "span" else 0)
        rows = [k * 4096 + 2000 - 100 for k in (0, 1, 2, 3, 8, 9)]          # (chromosome rows: global block k, row 2000 of it)
    ss = T.sorted_starts("w")
    for j in rows:
        T.call("w", int(ss[j]) + BIAS)
    return T.store(), dict(rows=[100 + j for j in rows], placed=T.placed)


# (b) ------------------------------------------------------------------------------------------- step (1) beyond 128 blocks
BLOCK_N = 128 * 4096 + 65


def block_table():
    """a chromosome of 128 * 4096 + 65 reads behind 100 reads of another: 129 blocks, so step (1) loads bfirst a second time.
    Windows in blocks 0, 126, 127 and 128, one whose L IS the first start of block 128 (a DEL call) and one a base below it (an INS
    call: two DEL calls a base apart would chain into one cluster) -> (store, dict(rows = global rows of L, first128 = first start of block 128))"""
    T = Table(["f0", "b"])
    _front(T)
    starts = 10_000 + 10 * np.arange(BLOCK_N)
    T.reads("b", starts, starts + 3000)
    rows = [2000, 126 * 4096 + 7, 127 * 4096 + 7, 128 * 4096 + 40]
    for g in rows:
        T.call("b", int(starts[g - 100]) + BIAS)
    first128 = int(starts[128 * 4096 - 100])
    T.call("b", first128 + BIAS)                          # DEL: L == bfirst[128]
    T.call("b", first128 - 1 + INS_HALF, "INS")           # INS: L == bfirst[128] - 1
    return T.store(), dict(rows=rows, first128=first128, placed=T.placed)


# (c) ------------------------------------------------------------------------------------------- seams
SEAM_SIZES = (0, 1, 63, 64, 65, 4095, 4096, 4097)
SEAM_END, SEAM_HI = 1_000_000, 900_000


def seam_table():
    """chromosomes of 0, 1, 63 ... 4 097 reads in one table.  The first 40 rows of each (start 200 .., end 1 000 000) and the
    last 40 (start just below the high window's L) are primary, carry ids of their own and span the window coordinates of the
    calls of EVERY chromosome: one row test that lets a neighbour's row through changes DR.  Calls per chromosome: L below the
    first start (cover 0), a low and a high window, one beyond the last end (cover 0)."""
    names = ["s%d" % k for k in range(len(SEAM_SIZES))]
    T = Table(names)
    for ch, n in zip(names, SEAM_SIZES):
        head = min(n, 40)
        tail = min(n - head, 40)
        mid = n - head - tail
        if head:
            T.reads(ch, 200 + np.arange(head), SEAM_END)
        if mid:
            s = 10_000 + (870_000 * np.arange(mid)) // mid
            T.reads(ch, s, s + 2000, primary=(np.arange(mid) % 7 != 0).astype(np.uint8))
        if tail:
            T.reads(ch, SEAM_HI - BIAS - tail + np.arange(tail), SEAM_END)
        for pos in (150, 1000, SEAM_HI, SEAM_END + 500):
            T.call(ch, pos)
        T.call(ch, 500_000, "INS")
    # (a chromosome without reads yields no call: INDEL:443-444.  k_genotype's own `r1 > r0` guards are therefore reached by no
    # call of this table either: the calls of such a chromosome are dropped before the genotype step)
    T.placed -= 5
    return T.store(), dict(placed=T.placed)


# (d) ------------------------------------------------------------------------------------------- ties
def _nine(T, ch, L, R, dl=1, dr=1):
    """reads with start = L - dl, L, L + dl and end = R - dr, R, R + dr in all nine combinations (four of them cover)"""
    for s in (L - dl, L, L + dl):
        for e in (R - dr, R, R + dr):
            T.reads(ch, s, e)


def tie_table():
    """exact ties on integer and x.5 bounds, runs of equal starts across chunk and block boundaries, repeated ids
    -> (store, dict of the facts a test asserts)"""
    T = Table(["f0", "t", "u"])
    _front(T)
    bg = 1_000_000 + 100 * np.arange(3000)
    T.reads("t", bg, bg + 2000)
    T.call("t", 1_150_000)                                 # (an ordinary call in the background)
    # integer bounds: DEL [P - 100, P + 100], INS [P - 1000, P + 1000]
    T.call("t", 100_000); _nine(T, "t", 100_000 - BIAS, 100_000 + BIAS)
    T.call("t", 200_000, "INS"); _nine(T, "t", 200_000 - INS_HALF, 200_000 + INS_HALF)
    # x.5 bounds: INV with the odd bias 501 (windows bp -+ 250.5), DUP with bp2 - bp1 = 301 < bias (windows bp -+ 150.5):
    # 2 start <= 2 bp - nb <=> start <= bp - (nb + 1) / 2, 2 end >= 2 bp + nb <=> end >= bp + (nb + 1) / 2
    T.pair("t", 300_000, 305_000, "INV")
    for bp in (300_000, 305_000):
        _nine(T, "t", bp - 251, bp + 251)
    T.pair("t", 400_000, 400_301, "DUP")
    for bp in (400_000, 400_301):
        _nine(T, "t", bp - 151, bp + 151)
    # 300 reads that share the start L (any 300 rows cross four chunk boundaries), a third of them one base short of R
    P = 500_000
    T.call("t", P)
    T.reads("t", np.full(300, P - BIAS), P + BIAS - 1 + np.arange(300) % 3)
    T.reads("t", np.full(50, P - BIAS + 1), P + BIAS + 5)
    T.reads("t", np.full(50, P - BIAS - 1), P + BIAS - 1 + np.arange(50) % 3)
    # repeated ids: one id three times as primary in one cover (counts once); a covering read that is a support read (no DR);
    # a primary and a non-primary row of one id (counts once); an id with a non-primary covering row only (does not count)
    P = 600_000
    sup = T.call("t", P)
    three = T.reads("t", P - BIAS - 30, P + BIAS + 30)
    T.reads("t", [P - BIAS - 20, P - BIAS], [P + BIAS, P + BIAS + 9], ids=three[0])
    T.reads("t", P - BIAS - 10, P + BIAS + 10, ids=sup[1])
    both = T.reads("t", P - BIAS - 5, P + BIAS + 5)
    T.reads("t", P - BIAS - 4, P + BIAS + 4, primary=0, ids=both[0])
    T.reads("t", P - BIAS - 3, P + BIAS + 3, primary=0)
    want_600k = 2                                          # `three` and `both`
    # 5 000 reads that share the start L, laid so that TWO consecutive blocks begin inside the run (equal first starts)
    P = 700_000
    r0_u = 100 + sum(len(r[0]) for r in T.rows["t"])
    fill = (4000 - r0_u) % 4096
    if fill < 400:
        fill += 4096
    f = 1000 + 10 * np.arange(fill)
    T.reads("u", f, f + 500)
    T.call("u", P)
    T.reads("u", np.full(5000, P - BIAS), P + BIAS - 1 + np.arange(5000) % 3)
    T.reads("u", np.full(100, P - BIAS + 1), P + BIAS + 5)
    T.call("u", 3000)                                      # (an ordinary call among the filler rows)
    return T.store(), dict(run_row=r0_u + fill, run_L=P - BIAS, dr_600k=want_600k, placed=T.placed)


# (e) ------------------------------------------------------------------------------------------- tiers
TIER_N = 2_100_000
TIER_CUT = 60_000
TIER_TOTALS = (640, 704, 705, 768, 769, 6080, 6144, 6145, 7000, 20000)
TIER_K = 5


def tier_table(full=True):
    """One chromosome of 2 100 000 reads (513 blocks; the pool becomes 2^24 ints and a wavefront's slice 16 384) behind 100 reads
    of another.  Background: 1 kb reads, one per 50 bp.  Ten piles of 3 kb reads, each under one call, sized so that the call's
    distinct supports + cover is exactly 640 ... 20 000 (the support reads are rows of the pile).  full=False: the same piles in the first 60 000 rows only (pool 2^20).
    The full table adds ordinary calls in blocks 255, 256, 257 and the last (step (1) loads bfirst five times)."""
    T = Table(["f0", "big"])
    _front(T)
    piles = []
    for i, total in enumerate(TIER_TOTALS):
        P = 10_000 + 25_000 + 50_000 * i
        pos = P + 1500
        # background rows covering [pos - 100, pos + 100]: start in (pos + 100 - 1000, pos - 100], starts at 10 000 + 50 j
        lo, hi = pos + BIAS - 1000, pos - BIAS
        bgc = hi // 50 - (lo + 49) // 50 + 1
        piles.append((P, pos, total - bgc))
    n_pile = sum(p[2] for p in piles)
    n_bg = (TIER_N if full else TIER_CUT) - n_pile
    bg = 10_000 + 50 * np.arange(n_bg)
    T.reads("big", bg, bg + 1000)
    for P, pos, n in piles:
        sup = T.call("big", pos, k=TIER_K)
        T.reads("big", np.full(TIER_K, P), P + 3000, ids=sup)          # the support reads lie in the pile: the set must hold them first
        T.reads("big", np.full(n - TIER_K, P), P + 3000)
    rows = []
    if full:
        ss = T.sorted_starts("big")
        rows = [255 * 4096 + 9, 256 * 4096 + 9, 257 * 4096 + 9, 100 + TIER_N - 30]
        for g in rows:
            T.call("big", int(ss[g - 100]) + BIAS)
    return T.store(), dict(rows=rows, placed=T.placed)


# (f) ------------------------------------------------------------------------------------------- coordinate edges
def edge_table():
    """int32 edges: reads that end at 2^31 - 1, a window whose R lies beyond it (the int32 form returns early), L = 0 after the
    clamp with reads that start at 0, a read as long as the int32 range (R - maxlen far below zero)"""
    T = Table(["f0", "e"])
    _front(T)
    T.reads("e", 0, INT32_MAX)                             # the whole range, primary
    i = np.arange(200)
    T.reads("e", INT32_MAX - 2000 - 10 * i, np.where(i % 2 == 0, INT32_MAX, INT32_MAX - 1 - i))
    T.reads("e", np.zeros(50, np.int64), 150 + np.arange(50))                 # start 0: end 160 and above covers [0, 160]
    T.reads("e", 1 + np.arange(50), 3000)                  # start 1 and above: never
    m = 1_000_000_000 + 100 * np.arange(300)
    T.reads("e", m, m + 3000)
    T.call("e", 60)                                        # L = max(-40, 0) = 0, R = 160
    T.call("e", 1_000_015_000)                             # ordinary
    T.call("e", INT32_MAX - INS_HALF, "INS")               # R == 2^31 - 1 (an INS call: two DEL calls this close would chain)
    T.call("e", INT32_MAX - 49)                            # R == 2^31 + 50: nothing covers
    return T.store(), dict(placed=T.placed)


# ------------------------------------------------------------------------------------------------ shared, computed once
SMALL = ("walk_span", "walk_middle", "walk_nonprimary", "seam", "tie", "edge")
ALL = SMALL + ("block", "walk_shift", "tier", "tier_cut")


@functools.lru_cache(maxsize=None)
def table(name):
    """-> (store, facts of the table: the calls placed and what a test asserts about its geometry)"""
    if name.startswith("walk_"):
        kind = name[5:]
        return walk_table("span" if kind == "shift" else kind, shift=WALK_SHIFT if kind == "shift" else 0)
    if name in ("tier", "tier_cut"):
        return tier_table(full=name == "tier")
    return {"block": block_table, "seam": seam_table, "tie": tie_table, "edge": edge_table}[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> (host batch of the int64 store, the C oracle's trimmed result, brute_dr of it): the two yardsticks, computed once"""
    from oracle import oracle
    st, _ = table(name)
    hb = st.host_batch(st.tasks(), PARAMS)
    want = oracle.cluster_batch(hb, per_sig=True).trimmed()
    return hb, want, brute_dr(st, PARAMS, hb.segments, want)
