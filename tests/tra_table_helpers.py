"""Helpers of tests/test_tra_reads_table.py: a brute-force sequential statement of call_gt / count_coverage over the reads table
(cuteSV_resolveTRA.py:258-309, cuteSV_genotype.py:62-93), a CPU model of the ROUTE k_genotype_tra takes (the two 64-ary
searches, the steps of 64 rows, the lane that ends a step, the set fill at every step start, the set tier), so that a table can
assert the geometry it claims, and the builders of the crafted tables.

A TRA call is a cluster of `k` identical TRA signatures with distinct read names: bp1 / bp2 are then the crafted positions and
the windows [bp - BIAS, bp + BIAS), clamped to [0, contig_len].  On a `Lanes` chromosome the last row is a long secondary read
far behind every window: it sets the device's maxlen, every window's walk then starts at the chromosome's first row, and a row's
lane is its index in the chromosome mod 64.  Starts are strictly increasing inside a chromosome, so that the start order of the
table is unique (the walk depends on the order of the rows, unlike the cover search)."""
import dataclasses
import functools

import numpy as np

from cutesv_amd import _abi
from cutesv_amd.columns import Params, SigStore
from cutesv_amd.genotype import gl_index

import cover_helpers as ch

BIAS = 800                     # max_cluster_bias_TRA of every table: half-width of a window
TG_LIMIT = 3072                # 3/4 of the 4096-slot LDS set
TRA_GRID = 256                 # workgroups of k_genotype_tra: one slice of the global pool each
BND = "ABCD"
FAR = 50_000_000               # start of the long secondary row of a Lanes chromosome
FAR_LEN = 60_000_000


def params(gt_round=500):
    return Params(min_support=2, genotype=True, genotype_tra=True, max_cluster_bias_TRA=BIAS, gt_round=gt_round,
                  max_cluster_bias_DEL=100, max_cluster_bias_INS=100)


def up_bound(num):             # threshold_ref_count, cuteSV_genotype.py:62-70
    if num <= 2:
        return 20 * num
    if num <= 5:
        return 9 * num
    if num <= 15:
        return 7 * num
    return 5 * num


def tra_bits_for(ns):
    need = ns + 2 * (up_bound(ns) + 64) + 128
    bits = 10
    while (3 << bits) // 4 < need + 64:
        bits += 1
    return bits


# ------------------------------------------------------------------------------------------------ the calls of a result
def tra_calls(st, segments, result):
    """[dict(c, genotyped, chr1, chr2, bp1, bp2, sup = support read ids)] of every TRA call of a trimmed result"""
    out = []
    off, sig = result["support_off"], result["support_sig"]
    for c in range(len(result["call_seg"])):
        sg = segments[int(result["call_seg"][c])]
        if int(sg["svtype"]) != _abi.TRA:
            continue
        out.append(dict(c=c, genotyped=bool(sg["genotype"]), chr1=int(sg["chrom"]), chr2=int(result["call_aux"][c]) >> 3, code=int(result["call_aux"][c]) & 7,
                        bp1=int(result["bp1"][c]), bp2=int(result["bp2"][c]), sup=[int(x) for x in st.read_id[sig[int(off[c]):int(off[c + 1])]]]))
    return out


def window(st, chrom, pos):
    return max(pos - BIAS, 0), min(pos + BIAS, int(st.contig_len[chrom]))


def rows_of(st, chrom):
    """the chromosome's rows as a list of (start, end, primary, id) tuples (kept on the store)"""
    cache = st.__dict__.setdefault("_rows_of", {})
    if chrom not in cache:
        r0, r1 = int(st.reads_off[chrom]), int(st.reads_off[chrom + 1])
        cache[chrom] = list(zip(st.r_start[r0:r1].tolist(), st.r_end[r0:r1].tolist(), st.r_primary[r0:r1].tolist(), st.r_id[r0:r1].tolist()))
    return cache[chrom]


# ------------------------------------------------------------------------------------------------ yardstick 1: the sequential walk
def brute_window(rows, s, e, names, bound, itround, ratio_lt=False):
    """count_coverage (cuteSV_genotype.py:72-93) over every row of the chromosome, one after the other"""
    if s >= e:
        return 0
    iteration = primary = 0
    for start, end, prim, name in rows:
        if not (start < e and end > s):                      # fetch(): the alignments that overlap [s, e)
            continue
        iteration += 1
        if prim != 1:
            continue
        primary += 1
        if start < s and end > e:
            names.add(name)
            if len(names) >= bound:
                return 1
        if iteration >= itround:
            if ratio_lt:
                return 1 if 5 * primary < iteration else -1
            return 1 if 5 * primary <= iteration else -1      # float(primary_num / iteration) <= 0.2
    return 0


def brute_call(st, call, itround, ratio_lt=False):
    """call_gt (cuteSV_resolveTRA.py:258-309) -> (dr, status); dr -1 with status -1"""
    names = set()
    sup = set(call["sup"])
    bound = up_bound(len(sup))
    s, e = window(st, call["chr1"], call["bp1"])
    status = brute_window(rows_of(st, call["chr1"]), s, e, names, bound, itround, ratio_lt)
    if status == -1:
        return -1, -1
    if status == 0:
        s, e = window(st, call["chr2"], call["bp2"])
        brute_window(rows_of(st, call["chr2"]), s, e, names, bound, itround, ratio_lt)
    return sum(1 for q in names if q not in sup), status


def brute(st, segments, result, itround, ratio_lt=False):
    """every genotyped TRA call of the result -> dict(call=, dr=, dv=, gl_idx=, status=)"""
    calls = [k for k in tra_calls(st, segments, result) if k["genotyped"]]
    got = [brute_call(st, k, itround, ratio_lt) for k in calls]
    dv = [len(set(k["sup"])) for k in calls]
    return dict(call=np.array([k["c"] for k in calls], np.int64), dr=np.array([g[0] for g in got], np.int64), dv=np.array(dv, np.int64),
                gl_idx=np.array([-1 if g[1] == -1 else gl_index(g[0], v) for g, v in zip(got, dv)], np.int64), status=np.array([g[1] for g in got], np.int64))


def twin(st, segments, result, itround):
    """yardstick 3: aln.tra_genotype_host (tra_bam.window_status over a stub fetch) on the same rows -> (dr, status)"""
    from cutesv_amd import aln
    calls = [k for k in tra_calls(st, segments, result) if k["genotyped"]]
    per = []
    for c in range(len(st.chroms)):
        r0, r1 = int(st.reads_off[c]), int(st.reads_off[c + 1])
        per.append((st.r_start[r0:r1], st.r_end[r0:r1], st.r_primary[r0:r1] == 1, st.r_id[r0:r1]))
    dr, status = aln.tra_genotype_host(aln.Table.from_chroms(per), chrom1=[k["chr1"] for k in calls], pos1=[k["bp1"] for k in calls], chrom2=[k["chr2"] for k in calls],
                                       pos2=[k["bp2"] for k in calls], support_off=np.r_[0, np.cumsum([len(k["sup"]) for k in calls])].astype(np.int64),
                                       support=np.array([x for k in calls for x in k["sup"]], np.int64), contig_len=st.contig_len, bias=BIAS, gt_round=itround)
    return np.asarray(dr, np.int64), np.asarray(status, np.int64)


# ------------------------------------------------------------------------------------------------ the route, modelled on the CPU
def pp_wave(lo, hi, pred, floor=False):
    """partition_point_wave: first index of [lo, hi) at which pred turns false, 64 probes a round -> (index, rounds of the loop).
    floor: the mutation whose probe stride is rounded down (the 64 probes then do not reach the end of the range)"""
    rounds = 0
    while hi - lo > 64:
        rounds += 1
        step = (hi - lo) // 64 if floor else (hi - lo + 63) // 64
        t = sum(1 for lane in range(64) if lo + lane * step < hi and pred(lo + lane * step))
        if t == 0:
            return lo, rounds
        lo, hi = lo + (t - 1) * step + 1, min(lo + t * step, hi)
    return lo + sum(1 for lane in range(64) if lo + lane < hi and pred(lo + lane)), rounds


def model_window(st, chrom, s, e, S, bound, itround, limit, mutate):
    """tra_window on the CPU.  S: the call's running state (ids = names in the set, q = names of querydata, sup, nq, dr, filled,
    overflow).  -> (status, dict(lo, hi, r0, rounds = (first search, second search), fills = filled at every step start, stop =
    None | (kind, row)))"""
    info = dict(s=s, e=e, lo=None, hi=None, rounds=None, fills=[], stop=None, walked=False)
    if s >= e:
        return 0, info
    r0, r1 = int(st.reads_off[chrom]), int(st.reads_off[chrom + 1])
    info["r0"] = r0
    if r1 <= r0:
        return 0, info
    rows = rows_of(st, chrom)
    maxlen = ch.device_maxlen(st, chrom)
    le = mutate == "edge_le"                                  # the mutation that takes every strict comparison of an edge as <=
    hi, k1 = pp_wave(r0, r1, lambda i: rows[i - r0][0] < e + le, floor=mutate == "floorstep")
    lo, k2 = pp_wave(r0, hi, lambda i: rows[i - r0][0] + maxlen <= s, floor=mutate == "floorstep")
    info.update(lo=lo, hi=hi, rounds=(k1, k2), walked=True)
    iteration = primary = 0
    for base in range(lo, hi, 64):
        info["fills"].append(S["filled"])
        if S["filled"] + 64 > limit - (mutate == "fill_ge"):   # (the mutation that gives up a step early)
            S["overflow"] = True
            return 0, info
        lanes = []                                            # (row, ov, prim, span, dup, id)
        seen = set()
        for i in range(base, min(base + 64, hi)):
            start, end, p, name = rows[i - r0]
            ov = end > s - le
            prim = ov and p == 1
            span = prim and start < s + le and end > e - le
            dup = span and name in seen and mutate != "nodup"
            if span:
                seen.add(name)
            lanes.append((i, ov, prim, span, dup, name))
        for _, _, _, span, dup, name in lanes:                # every spanning lane of the step enters the set, committed or not
            if span and not dup and name not in S["ids"]:
                S["ids"].add(name)
                S["filled"] += 1
        q0 = set(S["q"])
        it_i, pn_i, nq_i, stop = iteration, primary, S["nq"], None
        new, firsts = [], {}
        for i, ov, prim, span, dup, name in lanes:
            isnew = span and not dup and name not in q0
            it_i += ov; pn_i += prim; nq_i += isnew
            new.append(isnew)
            if span and nq_i >= bound:
                firsts.setdefault("A", i)
            if prim and it_i >= itround:
                firsts.setdefault("B", i)
            if stop is None and ((span and nq_i >= bound) or (prim and it_i >= itround)):
                stop = (i, "A" if (span and nq_i >= bound) else "B", it_i, pn_i, nq_i)
        last = stop[0] if stop else base + 63
        for (i, _, _, _, _, name), isnew in zip(lanes, new):
            if isnew and (i <= last or mutate == "behind"):
                S["q"].add(name)
                S["dr"] += name not in S["sup"]
        if stop:
            i, kind, it_t, pn_t, nq_t = stop
            S["nq"] = nq_t
            info["stop"], info["firsts"] = (kind, i), firsts          # (firsts: the first lane of the step at which each exit holds)
            if kind == "A":
                return 1, info
            if mutate == "ratio":
                return (1 if 5 * pn_t < it_t else -1), info
            return (1 if 5 * pn_t <= it_t else -1), info
        iteration, primary, S["nq"] = it_i, pn_i, nq_i
    return 0, info


def model_call(st, call, itround, limit=TG_LIMIT, mutate=None):
    """tra_call on the CPU with a set of `limit` usable slots -> dict(dr, status, overflow, w1, w2 = the windows' infos)"""
    sup = sorted(set(call["sup"]))
    ns = len(sup)
    S = dict(ids=set(), q=set(), sup=set(sup), nq=0, dr=0, filled=0, overflow=False)
    for base in range(0, ns, 64):
        if S["filled"] + 64 > limit:
            S["overflow"] = True
            break
        S["ids"].update(sup[base:base + 64])
        S["filled"] = len(S["ids"])
    out = dict(ns=ns, w1=None, w2=None, status=0)
    if not S["overflow"]:
        s, e = window(st, call["chr1"], call["bp1"])
        out["status"], out["w1"] = model_window(st, call["chr1"], s, e, S, up_bound(ns), itround, limit, mutate)
        if out["status"] == 0 and not S["overflow"]:
            s, e = window(st, call["chr2"], call["bp2"])
            _, out["w2"] = model_window(st, call["chr2"], s, e, S, up_bound(ns), itround, limit, mutate)
    out.update(overflow=S["overflow"], dr=-1 if out["status"] == -1 else S["dr"], filled=S["filled"])
    return out


def scan_visits(segments, result, mutate=None):
    """the call scan of k_genotype_tra on the CPU: workgroup b looks at the calls [64 b, 64 b + 64), then 64 * 256 further on; a
    ballot picks the genotyped TRA calls -> the calls visited, in any order.  Mutations: lane63 (the ballot loses its last lane),
    one_round (no grid stride), full_rounds (a round that is not full is dropped), any_tra (the genotype bit is not looked at)"""
    n = len(result["call_seg"])
    sg = segments[np.asarray(result["call_seg"], np.int64)]
    tra, gt = sg["svtype"] == _abi.TRA, sg["genotype"] != 0
    out = []
    for b in range(TRA_GRID):
        for c0 in range(64 * b, n, 64 * TRA_GRID):
            if mutate == "full_rounds" and c0 + 64 > n:
                continue
            out += [c for c in range(c0, min(c0 + 64 - (mutate == "lane63"), n)) if tra[c] and (gt[c] or mutate == "any_tra")]
            if mutate == "one_round":
                break
    return sorted(out)


def pool_ints(st, hb):
    """the global pool as the upload plans it: cover_helpers.pool_ints' rule, and 64 ints per signature of the longest genotyped
    TRA segment + 8192"""
    sg = hb.segments
    ln = sg["sig_end"] - sg["sig_begin"]
    tra = (sg["genotype"] != 0) & (sg["svtype"] == _abi.TRA)
    tra_len = int(ln[tra].max()) if tra.any() else 0
    n = ch.pool_ints(st, hb)
    while n < 64 * tra_len + 8192:
        n <<= 1
    return n


def route(st, hb, call, itround):
    """-> (tier, model of the call in that tier): "lds", "slice" (this workgroup's slice of the pool) or "huge" (the whole pool,
    by the last workgroup)"""
    m = model_call(st, call, itround)
    if not m["overflow"]:
        return "lds", m
    bits = tra_bits_for(m["ns"])
    pool = pool_ints(st, hb)
    tier = "slice" if (2 << bits) <= pool // TRA_GRID and bits <= 30 else "huge"
    assert (2 << bits) <= pool
    m = model_call(st, call, itround, limit=(3 << bits) // 4)
    assert not m["overflow"]
    return tier, m


# ------------------------------------------------------------------------------------------------ table builder
class Table(ch.Table):
    """cover_helpers.Table with TRA calls, reference lengths and claims: (key of a call, what the model must say about it)"""

    def __init__(self, chroms, contig_len):
        super().__init__(chroms)
        self.contig_len = dict(contig_len)
        self.claims = []
        self.extra_sigs = 0
        self.ungenotyped = []

    def tra(self, chr1, pos1, chr2, pos2, k=3, typ="A", twice=0, claim=None):
        """k identical TRA signatures -> the support read ids; `twice`: that many of the reads carry a second signature, two
        bases further on the mate (the call's DV stays k)"""
        ids = self._names(k)
        for j in ids:
            self.per["TRA"].append((typ, int(pos1), chr2, int(pos2), "s%08d" % j, "TRA", chr1))
        for j in ids[:twice]:
            self.per["TRA"].append((typ, int(pos1), chr2, int(pos2) + 2, "s%08d" % j, "TRA", chr1))
        self.extra_sigs += twice
        if claim is not None:
            self.claims.append(((chr1, chr2, BND.index(typ), int(pos1)), dict(claim, dv=k)))
        return ids

    def singles(self, chr1, chr2, first, n, gap=2 * BIAS + 400):
        """n TRA signatures, each alone in its cluster: they lengthen a segment and make no call"""
        ids = self._names(n)
        self.placed -= 1
        for i, j in enumerate(ids):
            self.per["TRA"].append(("A", first + gap * i, chr2, 1000, "s%08d" % j, "TRA", chr1))

    def store(self):
        st = SigStore.from_tuple_lists(self.per, chroms=self.chroms)
        assert st.n_sig == self.n_support + self.extra_sigs and int(st.read_id.max()) == self.n_support - 1
        off, cols = [0], [[], [], [], []]
        for c in self.chroms:
            if self.rows[c]:
                blk = [np.concatenate([r[i] for r in self.rows[c]]) for i in range(4)]
                o = np.argsort(blk[0], kind="stable")
                assert (np.diff(blk[0][o]) > 0).all(), "starts of %s are not strictly increasing" % c
                for i in range(4):
                    cols[i].append(blk[i][o])
            off.append(off[-1] + sum(len(r[0]) for r in self.rows[c]))
        s, e, p, i = [np.concatenate(x) if x else np.zeros(0, np.int64) for x in cols]
        i = np.where(i < 0, self.n_support + (-1 - i), i)
        return dataclasses.replace(st, reads_off=np.array(off, np.int64), r_start=s, r_end=e, r_primary=p.astype(np.uint8), r_id=i.astype(np.int32),
                                   contig_len=np.array([self.contig_len[c] for c in self.chroms], np.int64))


class Lanes:
    """a chromosome whose rows are laid one by one in start order; its last row is the long secondary read that pins every walk to
    the chromosome's first row"""

    def __init__(self, T, chrom):
        self.T, self.chrom, self.n = T, chrom, 0
        T.reads(chrom, FAR, FAR + FAR_LEN, primary=0)

    def row(self, start, end, primary=1, ids=None):
        self.n += 1
        return int(self.T.reads(self.chrom, start, end, primary=primary, ids=ids)[0])


class Region:
    """the rows around one window [P - BIAS, P + BIAS): they begin on lane 0 of a fresh step (filler rows that overlap nothing pad
    the step before), starts s - 3000 + i.  kinds: span = primary, starts before s and ends behind e; sec = the same, not primary;
    prim = primary, ends AT e; skip = ends at s (not fetched)"""
    CAP = 3000

    def __init__(self, L, P):
        self.L, self.P, self.s, self.e, self.i = L, P, P - BIAS, P + BIAS, 0
        pad = (-L.n) % 64
        for j in range(pad):
            L.row(self.s - self.CAP - 64 + j, self.s - self.CAP - 63 + j)
        self.first = L.n                                      # row of the chromosome at which the region begins: a multiple of 64

    def add(self, kind, n=1, ids=None):
        out = []
        for k in range(n):
            start = self.s - self.CAP + self.i
            assert start < self.s
            end = {"span": self.e + 7, "sec": self.e + 7, "prim": self.e, "skip": self.s}[kind]
            out.append(self.L.row(start, end, primary=0 if kind == "sec" else 1, ids=None if ids is None else ids[k]))
            self.i += 1
        return out


def _chroms(*names):
    """-> (chromosome names: a front chromosome of 100 reads first, "z" without reads last, contig lengths)"""
    names = ["0f"] + list(names) + ["z"]
    return names, {c: 200_000_000 for c in names}


def _table(*names):
    chroms, lens = _chroms(*names)
    T = Table(chroms, lens)
    ch._front(T, "0f")
    return T


SPACING = 10_000


# (a) ------------------------------------------------------------------------------------------- steps
def _stop_regions(T, L, G, P0):
    """exit A and exit B on lane 63, on lane 0 of the second step, on the last row of the window and on lane 10 with rows behind;
    the ratio rule at, above and below a fifth -> next free position"""
    P = P0
    # exit A: 2 supports, up_bound 40; the 40th name sits at the row the case names (all of these rows are primary: with a
    # gt_round below 64 exit B would fire first)
    for where in (63, 64, "last", 10) if G >= 64 else ():
        R = Region(L, P)
        at = 45 if where == "last" else where
        if at >= 39:
            R.add("skip", at - 39)
            R.add("span", 39)
        else:                                                 # lane 10: the names before it lie in a step of their own
            R.add("span", 39); R.add("skip", 25 + at)
        R.add("span")
        stop_row = R.first + R.i - 1
        if where != "last":
            R.add("span", 20)                                 # rows behind the stopping lane that would have spanned
        T.tra(L.chrom, P, "z", 500, k=2, claim=dict(stop1=("A", stop_row), lane=stop_row % 64, status=1, dr=40,
                                                  last=where == "last", step=(stop_row - R.first) // 64))
        P += SPACING
    # exit B: the first primary row at or after the G-th fetched row; N secondary rows in front of it
    for where in (63, 64, "last", 10):
        R = Region(L, P)
        N = max(G - 1, 4)
        if where == "last":
            N += 5
        else:
            while N % 64 != where % 64 or N < where:
                N += 1
        R.add("sec", N)
        R.add("span")
        stop_row = R.first + R.i - 1
        if where != "last":
            R.add("span", 20)
        T.tra(L.chrom, P, "z", 500, k=3, claim=dict(stop1=("B", stop_row), lane=stop_row % 64, status=1, dr=1, last=where == "last"))
        P += SPACING
    # the ratio rule: `it` fetched rows at the stop, of them p = it / 5 primary (status 1), one more (-1), one fewer (1)
    it = 5 * ((max(G, 5) + 4) // 5)
    for p, status in ((it // 5, 1), (it // 5 + 1, -1), (it // 5 - 1, 1)):
        if p < 1:
            continue
        R = Region(L, P)
        R.add("prim", p - 1)
        R.add("sec", it - p)
        R.add("prim")
        T.tra(L.chrom, P, "z", 500, k=3, claim=dict(stop1=("B", R.first + R.i - 1), status=status, dr=-1 if status == -1 else 0, ratio=(p, it)))
        P += SPACING
    return P


def steps_table(G):
    T = _table("a")
    L = Lanes(T, "a")
    _stop_regions(T, L, G, 20_000)
    return T


def ab_table():
    """gt_round 64: exit A and exit B in one step, A on the lower lane (status 1) and B on the lower lane (status -1)"""
    T = _table("a")
    L = Lanes(T, "a")
    P = 20_000
    R = Region(L, P)                                          # 3 supports: up_bound 27
    R.add("span", 26); R.add("sec", 14); R.add("span"); R.add("sec", 8); R.add("span", 6); R.add("sec", 8); R.add("prim"); R.add("span", 5)
    T.tra("a", P, "z", 500, k=3, claim=dict(stop1=("A", R.first + 40), lane=40, status=1, dr=27, other=("B", R.first + 63)))
    P += SPACING
    R = Region(L, P)
    R.add("sec", 40); R.add("skip", 24); R.add("span", 23); R.add("prim"); R.add("span", 6)
    T.tra("a", P, "z", 500, k=3, claim=dict(stop1=("B", R.first + 87), lane=23, status=-1, dr=-1, other=("A", R.first + 91)))
    return T


# (b) ------------------------------------------------------------------------------------------- names
def names_table():
    T = _table("a", "b")
    L, L2 = Lanes(T, "a"), Lanes(T, "b")
    P = 20_000
    # a name twice inside a step and across steps; in window 1 and again in window 2
    R = Region(L, P)
    x = R.add("span")[0]; R.add("span", ids=[x]); y = R.add("span")[0]
    R.add("skip", 61); R.add("span", ids=[y]); R.add("span", ids=[x])
    R2 = Region(L2, P)
    R2.add("span", ids=[x]); R2.add("span")
    T.tra("a", P, "b", P, k=3, claim=dict(status=0, dr=3, steps1=2, walked2=True))
    P += SPACING
    # the repeat decides the stop: 39 names, the first of them again, then the 40th (2 supports: up_bound 40) - inside one step ...
    R = Region(L, P)
    ids = R.add("span", 39); R.add("span", ids=ids[:1]); R.add("skip"); R.add("span"); R.add("span", 5)
    T.tra("a", P, "z", 500, k=2, claim=dict(stop1=("A", R.first + 41), status=1, dr=40))
    P += SPACING
    # ... and with the repeat on lane 0 of the next step
    R = Region(L, P)
    R.add("skip", 25); ids = R.add("span", 39); R.add("span", ids=ids[-1:]); R.add("span"); R.add("span", 5)
    T.tra("a", P, "z", 500, k=2, claim=dict(stop1=("A", R.first + 65), status=1, dr=40))
    P += SPACING
    # a spanning name that is a support: in querydata, not in DR; the supports listed twice
    R = Region(L, P)
    sup = T.tra("a", P, "z", 500, k=3, twice=2, claim=dict(stop1=("A", R.first + 26), status=1, dr=25))
    R.add("span", 10); R.add("span", ids=sup[:1]); R.add("span", 10); R.add("span", ids=sup[2:]); R.add("span", 10)
    P += SPACING
    # up_bound at each break of threshold_ref_count
    for ns in (2, 3, 5, 6, 15, 16):
        R = Region(L, P)
        R.add("span", up_bound(ns) + 10)
        T.tra("a", P, "z", 500, k=ns, claim=dict(stop1=("A", R.first + up_bound(ns) - 1), status=1, dr=up_bound(ns)))
        P += SPACING
    return T


# (c) ------------------------------------------------------------------------------------------- edges
EDGE_LEN = 100_000


def edges_table():
    """a chromosome without the long row (the walk starts where the second search says): window edges, clamps, empty windows,
    chromosomes without reads, a first window that ends the call"""
    chroms, lens = _chroms("e", "g")
    lens["e"] = lens["g"] = EDGE_LEN
    T = Table(chroms, lens)
    ch._front(T, "0f")
    P = 20_000
    s, e = P - BIAS, P + BIAS
    T.reads("e", [s - 900, s - 800, s - 700, s - 600, s - 500, s - 400, s, e - 1, e],
            [s, e, e + 1, e + 1, e + 1, s + 1, e + 9, e + 9, e + 9], primary=[1, 1, 1, 0, 1, 1, 1, 1, 1])
    # end == s: not fetched; end == e: fetched, does not span; two primaries that span and a secondary between them; a primary that
    # ends inside; start == s: does not span; start == e - 1: fetched; start == e: not fetched
    T.tra("e", P, "z", 500, k=3, claim=dict(status=0, dr=2, fetched1=7))
    # clamped at 0: rows from 0 on, nothing starts before 0
    T.reads("e", 10 * np.arange(30), 3000 + 10 * np.arange(30))
    T.tra("e", 300, "z", 500, k=3, claim=dict(status=0, dr=0, win1=(0, 1100)))
    # clamped at contig_len: rows that end at the contig's end do not span, rows before it do
    n = 12
    T.reads("e", EDGE_LEN - 3000 + 10 * np.arange(n), np.where(np.arange(n) % 2 == 0, EDGE_LEN, EDGE_LEN - 50))
    T.tra("e", EDGE_LEN - 300, "z", 500, k=3, claim=dict(status=0, dr=0, win1=(EDGE_LEN - 1100, EDGE_LEN)))
    # empty after the clamp (s == e, and s > e where the reference's fetch raises): window 2, on g, is walked
    T.reads("g", 40_000 - BIAS - 100 + 10 * np.arange(6), 40_000 + BIAS + 100)
    T.tra("e", EDGE_LEN + BIAS, "g", 40_000, k=3, claim=dict(status=0, dr=6, win1=(EDGE_LEN, EDGE_LEN), walked1=False, walked2=True))
    T.tra("e", EDGE_LEN + BIAS + 50, "g", 40_000, k=3, typ="B", claim=dict(status=0, dr=6, win1=(EDGE_LEN + 50, EDGE_LEN), walked1=False, walked2=True, raises=True))
    # chr2 without reads; both windows on the chromosome without reads
    T.tra("g", 40_000, "z", 500, k=3, claim=dict(status=0, dr=6, walked2=False))
    T.tra("z", 500, "z", 9000, k=3, claim=dict(status=0, dr=0, walked1=False, walked2=False))
    # window 1 ends the call with status 1 (27 names for 3 supports): the names of window 2 are not counted
    T.reads("g", 60_000 - BIAS - 100 + np.arange(30), 60_000 + BIAS + 100)
    T.tra("g", 60_000, "g", 40_000, k=3, claim=dict(status=1, dr=27, w2=None))
    # non-primary rows count in `iteration` only: 9 secondaries and a primary (gt_round 10 and below: exit B, a tenth primary)
    T.reads("g", 80_000 - BIAS - 100 + np.arange(10), 80_000 + BIAS + 100, primary=[0] * 9 + [1])
    T.tra("g", 80_000, "g", 40_000, k=3, claim=dict(nonprimary=True))
    return T


# (d) ------------------------------------------------------------------------------------------- search
SEARCH_SIZES = (1, 64, 65, 4096, 4097, 4160, 4161, 64 * 64 * 64 + 1, 266_304, 266_305)


def search_table():
    """chromosomes of 1 ... 266 305 rows (3 kb reads every 10 bases), a window at the first, a middle and the last row of each:
    every round count of the two 64-ary searches.  30 supports (up_bound 150): no exit, every row of [lo, hi) counts"""
    names = ["q%d" % k for k in range(len(SEARCH_SIZES))]
    chroms, lens = _chroms(*names)
    T = Table(chroms, lens)
    ch._front(T, "0f")
    for c, n in zip(names, SEARCH_SIZES):
        start = 5000 + 10 * np.arange(n)
        T.reads(c, start, start + 3000)
        for typ, row in zip("ABC", sorted(set((0, n // 2, n - 1)))):
            T.tra(c, int(start[row]) + BIAS + 5, "z", 500, k=30, typ=typ, claim=dict(search=(n, row), status=0, dr=min(row + 1, 140)))
    return T


# (e) ------------------------------------------------------------------------------------------- scan
def _small_calls(T, L, chrom, n, P0, typ="A"):
    """n TRA calls on one chromosome whose windows hold 1 + j % 7 spanning names -> next free position"""
    P = P0
    for j in range(n):
        R = Region(L, P)
        R.add("sec", 2); R.add("span", 1 + j % 7)
        T.tra(chrom, P, "z", 500, k=3, typ=typ, claim=dict(status=0, dr=1 + j % 7))
        P += SPACING
    return P


def scan_table(n_del, n_ins, n_tra, ungenotyped):
    """n_del DEL and n_ins INS calls (clusters of three signatures, genotyped by k_genotype) in front of n_tra genotyped TRA calls;
    `ungenotyped`: two calls of a TRA segment whose genotype flag the batch clears, on windows that hold spanning reads"""
    T = _table("a", "d", "x")
    T.reads("d", 100 + 40 * np.arange(50), 9000 + 40 * np.arange(50))          # (a chromosome without reads yields no DEL call)
    for i in range(n_del):
        T.call("d", 5_000 + 1000 * i, "DEL", k=3)
    for i in range(n_ins):
        T.call("d", 5_500 + 3000 * i, "INS", k=3)
    L = Lanes(T, "a")
    _small_calls(T, L, "a", n_tra, 20_000)
    if ungenotyped:
        Lx = Lanes(T, "x")
        _small_calls(T, Lx, "x", 2, 20_000)
        T.claims = [c for c in T.claims if c[0][0] != "x"]
        T.ungenotyped.append(("TRA", "x"))
    return T


# (f) ------------------------------------------------------------------------------------------- tiers
TIER_ROUND = 1_000_000


def _big(T, L, P, ns, names, typ="A", claim=None, mixed=False, chr2="z"):
    """a call of `ns` supports over `names` spanning rows.  mixed: every 199th row carries a support's name and every 211th the
    name of the row 130 rows (two steps) before it: what the set answers for them was written in an earlier step"""
    R = Region(L, P)
    sup = T.tra(L.chrom, P, chr2, P, k=ns, typ=typ, claim=claim)
    ids = []
    for i in range(names):
        if mixed and i % 199 == 60:
            ids += R.add("span", ids=[sup[i // 199]])
        elif mixed and i % 211 == 150:
            ids += R.add("span", ids=[ids[i - 130]])
        else:
            ids += R.add("span")
    return ids


def tier_table(kind):
    """lds_full: 576 supports and 39 steps of 64 names: the last step starts at filled + 64 == 3072; lds_over: one row more;
    huge1 / huge2: one / two calls of 520 supports (13 bits: 16 384 ints, more than a slice of 4096) over 2700 rows (exit A in the
    global set) and over 2580 rows and a second window on another chromosome that repeats names of the first;
    slice: the first of them beside a TRA segment of 32 700 lone signatures (pool 2^22, slice 16 384) and a call of 540 supports
    (14 bits: the whole pool)"""
    T = _table("a", "b", "f")
    L, L2 = Lanes(T, "a"), Lanes(T, "b")
    P = _small_calls(T, L, "a", 3, 20_000, typ="B")
    if kind in ("lds_full", "lds_over"):
        n = 39 * 64 + (kind == "lds_over")
        _big(T, L, P, 576, n, claim=dict(tier="lds" if kind == "lds_full" else "huge", status=0, dr=n, last_fill=3008 if kind == "lds_full" else None))
    else:
        _big(T, L, P, 520, 2700, mixed=True, claim=dict(tier="slice" if kind == "slice" else "huge", status=1, bits=13))
        if kind == "huge2":
            ids = _big(T, L, P + SPACING, 520, 2580, mixed=True, chr2="b", claim=dict(tier="huge", status=0, bits=13, walked2=True))
            R2 = Region(L2, P + SPACING)
            R2.add("span", 10, ids=ids[100:2100:200]); R2.add("span", 10)
        if kind == "slice":
            _big(T, L, P + SPACING, 540, 2800, mixed=True, claim=dict(tier="huge", status=1, bits=14))
            T.singles("f", "z", 10_000, 32_700)
    return T


# ------------------------------------------------------------------------------------------------ shared, computed once
STEP_ROUNDS = (2, 3, 12, 64, 65, 500)
TABLES = {"ab": (ab_table, 64), "names": (names_table, 500), "edges": (edges_table, 500), "edges_r10": (edges_table, 10), "edges_r4": (edges_table, 4),
          "search": (search_table, 500), "scan128": (lambda: scan_table(60, 3, 63, True), 500), "scan_far": (lambda: scan_table(16_400, 0, 3, False), 500)}
TABLES.update({"steps_r%d" % G: ((lambda G=G: steps_table(G)), G) for G in STEP_ROUNDS})
TIERS = ("lds_full", "lds_over", "huge1", "huge2", "slice")
TABLES.update({k: ((lambda k=k: tier_table(k)), TIER_ROUND) for k in TIERS})
ALL = tuple(TABLES)
RECORDED = tuple("steps_r%d" % G for G in STEP_ROUNDS) + ("ab", "names", "edges", "edges_r10", "edges_r4")      # golden/tra_edges.json.gz


@functools.lru_cache(maxsize=None)
def table(name):
    """-> (store, builder: its claims, ungenotyped segments and calls placed, gt_round)"""
    build, G = TABLES[name]
    T = build()
    return T.store(), T, G


def host_batch(st, T, G):
    hb = st.host_batch(st.tasks(), params(G))
    for k, t in enumerate(st.tasks()):
        if t in T.ungenotyped:
            hb.segments["genotype"][k] = 0
    return hb


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> (host batch of the int64 store, the C oracle's trimmed result, brute() of it)"""
    from oracle import oracle
    st, T, G = table(name)
    hb = host_batch(st, T, G)
    want = oracle.cluster_batch(hb, per_sig=True).trimmed()
    return hb, want, brute(st, hb.segments, want, G)


def claimed(name):
    """[(claim, call)] : every claim of the table with the call of the oracle's result it speaks of"""
    st, T, G = table(name)
    hb, want, _ = expected(name)
    calls = {(k["chr1"], k["chr2"], k["code"], k["bp1"]): k for k in tra_calls(st, hb.segments, want)}
    out = []
    for (c1, c2, code, pos), claim in T.claims:
        key = (st.chroms.index(c1), st.chroms.index(c2), code, pos)
        assert key in calls, (name, c1, c2, code, pos)
        out.append((claim, calls[key]))
    return out
