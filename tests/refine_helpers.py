"""Helpers of tests/test_refine_edges.py and tests/golden/make_golden_refine.py: a CPU model of the ROUTE a chained cluster takes
through the refine kernels (tier_of), closed-form builders that put clusters ON the thresholds of the refine rules at every size
beside a tier cut, and what each of them must show in the reference's rows (the landing checks).

Every value is built by integer arithmetic: no random numbers, so the tables are the same under any numpy.  A *site* is one case
of one rule at one size: a few hundred base pairs of one type's segment, more than the largest bias away from its neighbours, with
`expect` = what the reference's rows with POS inside the site must be (number of rows, supports in row order, positions, lengths).
Sites of all rules and sizes follow each other on ONE chromosome, so that small and large clusters share wavefronts and workgroups.
Sizes: the rule's minimum and LADDER_INDEL / LADDER_PAIR; above BIG = 257 signatures a rule keeps one or two of its cases per size (a
handful of 2048 / 2049 clusters per rule), chosen so that every rule still reaches the LDS and the global-scratch tier - which the
suite checks (claimed_cells).  A builder's docstring names the sizes at which its rule cannot be stated.

Float products that land off the exact value (found by a search over the two-decimal ratios, checked again by assertions here):
    0.7 * 90 = 62.99999999999999 and 0.35 * 180 = 62.99999999999999   a length gap of 63 splits an allele (DEL at 0.7, INS at 0.35)
    int(0.7 * n) = 0.7 n - 1 for n = 90, 170, 180, 330 ...             the members kept under remain_reads_ratio
    int(0.58 * 50) = 28, int(0.29 * 100) = 28
No two-decimal ratio r and m <= 2100 has fl(r * m) ABOVE an integer r * m, so TRA's `>= m * ratio` and `>= 0.5 * read_count` have
no case where float64 and exact arithmetic disagree: their cases sit on the exact products.  The keep count has no off-by-one
n below 50 for any two-decimal ratio: the clusters of fewer than 53 signatures state the keep count with exact products only.
Ties in |x - mean| on the SAME side of the mean are ties between equal values: whichever wins, every output is the same, so
only ties on opposite sides are stated."""
import hashlib
from fractions import Fraction

import numpy as np

from cutesv_amd.columns import Params, SigStore, TYPES

LADDER_INDEL = (16, 17, 32, 33, 64, 65, 256, 257, 2048, 2049)
LADDER_PAIR = (64, 65, 256, 257, 2048, 2049)
BIG = 257                          # above: one case per rule and size only (a handful of 2048 / 2049 clusters per rule)
SHIFT = (1 << 33) + 12345          # variant (b)
FAR = 270000                       # variant (c): the upper half of a site's signatures moves by this (> 2^18, < the bias)
FAR_BIAS = 300000
SUPPORT_IDX = {"DEL": 4, "INS": 4, "DUP": 4, "INV": 4, "TRA": 5}
DR_IDX = {"DEL": 7, "INS": 7, "DUP": 5, "INV": 5}
INS_HALF = 1000                    # half-width of an INS genotype window (INDEL:312)


# ------------------------------------------------------------------------------------------------ the route, modelled on the CPU
def tier_of(svtype, m, no_tiny=False):
    """the refine tier of a chained cluster of m signatures (close_gate, MID_CAP, the k_refine launches of stage_run.hip.h and
    `P <= CAP` in k_refine): DEL / INS register units of <= 16, 17 .. 32 and 33 .. 64 signatures (no_tiny: CSV_NO_TINY sends the
    first class through the paired units of 32), k_refine<64,64> for DUP / INV / TRA up to 64 (or the second phase of k_refine<64,256>),
    k_refine<64,256> up to 256, k_refine<256,2048> in LDS up to 2048 and in global scratch above"""
    if m > 2048:
        return "scratch"
    if m > 256:
        return "lds"
    if m > 64:
        return "mid"
    if svtype in ("DEL", "INS"):
        return "wave64" if m > 32 else "wave32" if (m > 16 or no_tiny) else "wave16"
    return "wave"


TIERS = {t: ("wave16", "wave32", "wave64", "mid", "lds", "scratch") if t in ("DEL", "INS") else ("wave", "mid", "lds", "scratch") for t in TYPES}


# ------------------------------------------------------------------------------------------------ tables
class Table:
    """sites of one parameter set; `far`: variant (c)"""

    def __init__(self, name, params, spacing=6000, far=False):
        self.name, self.params, self.spacing, self.far = name, params, spacing, far
        self.per = {t: [] for t in TYPES}
        self.sites = []
        # the types' sites do not share coordinates: a genotyped call sees the reads of its own site only
        self.origin = {t: k * (400000000 if far else 20000000) for k, t in enumerate(TYPES)}
        self.cur = {t: self.origin[t] + 10000 for t in TYPES}

    def bias(self, t):
        return getattr(self.params, "max_cluster_bias_" + t)

    def ratio(self, t):
        return getattr(self.params, "diff_ratio_merging_" + t)

    def add(self, t, rule, case, m, sigs, expect, at=None, strand="++", bnd="A", chr2="2", claim=True):
        """sigs: [(pos offset, length | pos2 offset, name index, sequence length or None)], offsets >= 0 from the site's base.
        expect: rows, support (row order), pos / pos2 (offsets), len (as printed), half2 (INV: doubled quotients, offsets),
        first_name (name index), seq_of (name index), search / search_alt (offsets; variant (d))"""
        sid = len(self.sites)
        if self.far and t in ("DEL", "INS") and rule != "chain":
            order = sorted(range(len(sigs)), key=lambda k: sigs[k][0])
            up = set(order[len(order) // 2:])
            sigs = [(s[0] + (FAR if k in up else 0),) + tuple(s[1:]) for k, s in enumerate(sigs)]
            expect = {k: v for k, v in expect.items() if k not in ("pos", "search", "search_alt")}
        assert len(set(s[:3] for s in sigs)) == len(sigs), ("the rebuild would drop an exact duplicate", t, rule, case, m)
        base = self.cur[t] if at is None else self.origin[t] + at
        span = max(s[0] for s in sigs)
        names = set()
        for dp, b, k, sl in sigs:
            nm = "n%04d_%05d" % (sid, k)
            names.add(nm)
            if t == "DEL":
                self.per[t].append((base + dp, b, nm, "DEL", "1"))
            elif t == "INS":
                sl = b if sl is None else sl
                self.per[t].append((base + dp, b, nm, ("ACGT" * (sl // 4 + 2))[k % 4:k % 4 + sl], "INS", "1"))
            elif t == "DUP":
                self.per[t].append((base + dp, base + b, nm, "DUP", "1"))
            elif t == "INV":
                self.per[t].append((strand, base + dp, base + b, nm, "INV", "1"))
            else:
                self.per[t].append((bnd, base + dp, chr2, base + b, nm, "TRA", "1"))
        e = dict(expect)
        for k in ("pos", "pos2"):
            if k in e:
                e[k] = [base + x for x in e[k]]
        for k in ("search", "search_alt"):
            if k in e:
                e[k] = base + e[k]
        if "half2" in e:
            e["half2"] = [2 * base + x for x in e["half2"]]
        for k in ("first_name", "seq_of"):
            if k in e:
                e[k] = "n%04d_%05d" % (sid, e[k])
        self.sites.append(dict(id=sid, type=t, rule=rule, case=case, m=m, lo=base, hi=base + span, n_sig=len(sigs), n_names=len(names),
                               expect=e, claim=claim))
        if at is None:
            self.cur[t] = base + span + self.spacing
        return sid


def shifted(per, reads, sites, delta):
    """variant (b): every position (and second position) moved by delta"""
    out = {t: [] for t in TYPES}
    for x in per["DEL"]:
        out["DEL"].append((x[0] + delta,) + x[1:])
    for x in per["INS"]:
        out["INS"].append((x[0] + delta,) + x[1:])
    for x in per["DUP"]:
        out["DUP"].append((x[0] + delta, x[1] + delta) + x[2:])
    for x in per["INV"]:
        out["INV"].append((x[0], x[1] + delta, x[2] + delta) + x[3:])
    for x in per["TRA"]:
        out["TRA"].append((x[0], x[1] + delta, x[2], x[3] + delta) + x[4:])
    rd = [(r[0] + delta, r[1] + delta) + r[2:] for r in reads]
    st = []
    for s in sites:
        e = dict(s["expect"])
        for k in ("pos", "pos2"):
            if k in e:
                e[k] = [x + delta for x in e[k]]
        for k in ("search", "search_alt"):
            if k in e:
                e[k] += delta
        if "half2" in e:
            e["half2"] = [x + 2 * delta for x in e["half2"]]
        st.append(dict(s, lo=s["lo"] + delta, hi=s["hi"] + delta, expect=e))
    return out, rd, st


# ------------------------------------------------------------------------------------------------ lengths with an exact mean
def levels(m, mean, tops):
    """m lengths with the exact mean `mean`: allele 0 = m - sum(counts) members whose largest is A, then for each (gap, count) of
    `tops` count members `gap` above the allele below.  Allele 0's members lie within a few units of A.  -> (lengths ascending, A)"""
    n0 = m - sum(c for _, c in tops)
    assert n0 >= 1
    off, at = 0, 0
    for g, c in tops:
        at += g
        off += at * c
    A = -((off - mean * m) // m)                       # ceil((mean m - off) / m)
    deficit = A * m + off - mean * m
    assert 0 <= deficit < m
    low = [A] * n0
    free = n0 - 1
    if deficit:
        assert free >= 1, "no free member to take the deficit"
        q, r = divmod(deficit, free)
        for k in range(free):
            low[k] -= q + (1 if k < r else 0)
        assert q + 1 <= 40
    assert min(low) >= 1, (m, mean, tops)
    out, at = sorted(low), A
    for g, c in tops:
        at += g
        out += [at] * c
    assert sum(out) == mean * m and len(out) == m
    return out, A


def inexact_mean(t):
    """(mean, ratio) of the type's table at which ratio * mean = 62.99999999999999"""
    return (90, 0.7) if t == "DEL" else (180, 0.35)


def check_products():
    assert 0.7 * 90 == 62.99999999999999 and 0.35 * 180 == 62.99999999999999 and 0.7 * 100 == 70.0 and 0.35 * 100 == 35.0
    assert int(0.7 * 90) == 62 and int(0.58 * 50) == 28 and int(0.29 * 100) == 28 and int(0.35 * 180) == 62
    assert [n for n in range(1, 7) if int(n * 0.4) == int(n * 0.6)] == [1, 3]


def off_by_one(rr, m):
    """largest n <= m with int(rr * n) one below the exact floor, or None"""
    fr = Fraction(str(rr))
    for n in range(m, 2, -1):
        if int(rr * n) != (fr * n).__floor__():
            return n
    return None


# ------------------------------------------------------------------------------------------------ INDEL rules
def _indel_types():
    return ("DEL", "INS")


def _len_print(t, v):
    return -v if t == "DEL" else v


def build_chain(T, sizes):
    """k_chain_count.  A gap equal to the bias stays, bias + 1 breaks (every type); a chained size of read_count - 1 against
    read_count; INV: the signed pos2 gap at bias / bias + 1 and a strand change; TRA: a BND-type change and a chr2 change (in the
    rebuild order a type or chr2 change comes with a position that falls back, so nothing else breaks the chain there)."""
    rc = T.params.min_support
    for t in TYPES:
        b = T.bias(t)
        ladder = (LADDER_INDEL if t in ("DEL", "INS") else LADDER_PAIR)
        for m in sorted(set((rc,) + tuple(s for s in ladder if s in sizes))):
            # m signatures a bias apart, then bias + 1, then read_count more: two clusters
            val = (lambda d: 100) if t in ("DEL", "INS") else (lambda d: d + 1000)
            sigs = [(i * b, val(i * b), i, None) for i in range(m)] + [(m * b + 1 + j, val(m * b + 1 + j), m + j, None) for j in range(rc)]
            e = dict(rows=2, support=[m, rc])
            if t == "DEL":
                e["pos"] = [(m - 1) * b // 2, m * b + 1 + (rc - 1) // 2]
            T.add(t, "chain", "bias", m, sigs, e)
        # read_count - 1 signatures, the break, read_count signatures: one row
        val = 100 if t in ("DEL", "INS") else 1000
        sigs = [(i, val, i, None) for i in range(rc - 1)] + [(rc - 2 + b + 1 + j, val, rc + j, None) for j in range(rc)]
        T.add(t, "chain", "count", rc, sigs, dict(rows=1, support=[rc]))
    b = T.bias("INV")
    # INV: pos2 rises by exactly the bias (stays), then by bias + 1 (breaks)
    sigs = [(0, 1000, i, None) for i in range(rc)] + [(1, 1000 + b, rc + i, None) for i in range(rc)] + [(2, 1000 + 2 * b + 1, 2 * rc + i, None) for i in range(rc)]
    T.add("INV", "chain", "pos2", 2 * rc, sigs, dict(rows=2, support=[2 * rc, rc]))
    # a strand change where both positions fall back
    T.add("INV", "chain", "strand", rc, [(i, 1000, i, None) for i in range(rc)], dict(rows=1, support=[rc]), at=2000, strand="--")
    # TRA: the last 'A' cluster is followed by this 'B' cluster at a lower position; then chr2 changes at a lower position still
    T.add("TRA", "chain", "bnd", rc, [(i, 500 + i, i, None) for i in range(rc)], dict(rows=1, support=[rc]), at=3000, bnd="B")
    T.add("TRA", "chain", "chr2", rc, [(i, 500 + i, i, None) for i in range(rc)], dict(rows=1, support=[rc]), at=2500, bnd="B", chr2="3")


def build_dedupe(T, sizes):
    """INDEL:124-134.  A read twice with equal lengths: the first is kept (strict >); the larger length first; the larger length
    second, where the kept element takes the read's FIRST place in the order of appearance (so it leads its equals after the stable
    length sort: the row's first name, and the INS sequence pick); distinct reads read_count - 1 against read_count.  Every unit
    but the last two has unique names otherwise: the hashed filter of the register tier must leave its fast route.
    Positions are 50 apart so that the kept element shows in POS.  Dropped sizes: none (minimum 4)."""
    rc = T.params.min_support
    for t in _indel_types():
        for m in sorted(set((rc + 1,) + tuple(sizes))):
            cases = ("eq_first", "larger_first", "larger_second") if m <= BIG else ("eq_first", "larger_second")
            for case in cases:
                l0, l1 = {"eq_first": (100, 100), "larger_first": (130, 100), "larger_second": (90, 100)}[case]
                sigs = [(0, l0, 0, None)] + [(50 * i, 100, i, None) for i in range(1, m - 1)] + [(50 * (m - 1), l1, 0, None)]
                e = dict(rows=1, support=[m - 1])
                if case == "larger_second":
                    e["first_name"] = 0
                    e["pos"] = [25 * m] if t == "DEL" else [50 * (m - 1)]
                elif t == "DEL":
                    e["pos"] = [25 * (m - 2)]
                elif case == "eq_first":
                    e["pos"] = [0]                      # INS: every member qualifies, the first in allele order is the first element
                T.add(t, "dedupe", case, m, sigs, e)
            for case, k in (("reads_below", rc - 1), ("reads_at", rc)):
                if m > BIG and case == "reads_at":
                    continue
                sigs = [(50 * i, 100, i % k, None) for i in range(m)]
                T.add(t, "dedupe", case, m, sigs, dict(rows=0) if k < rc else dict(rows=1, support=[rc]))


def build_split(T, sizes):
    """INDEL:136-162.  gap > ratio * mean with the mean EXACTLY 90 (DEL, 0.7) / 180 (INS, 0.35), where float64 gives
    62.99999999999999: gaps of 62 (one allele), 63 (splits in float64 only) and 64; the exact product 0.7 * 100 = 70.0 /
    0.35 * 100 = 35.0 with gaps on it (one allele) and one above; three alleles.  Dropped sizes: none (minimum 6, three alleles 9)."""
    gate = min(T.params.min_support, 5)
    for t in _indel_types():
        mean, ratio = inexact_mean(t)
        assert ratio == T.ratio(t) and ratio * mean == 62.99999999999999
        exact = int(ratio * 100)
        assert ratio * 100 == float(exact)
        for m in sorted(set((2 * gate,) + tuple(sizes))):
            cases = [("below", mean, 62), ("float", mean, 63), ("above", mean, 64), ("exact_on", 100, exact), ("exact_above", 100, exact + 1)]
            if m > BIG:
                cases = [cases[1]] if m % 2 == 0 else [cases[3], cases[1]]
            for case, mu, gap in cases:
                if case.startswith("exact") and mu * m - (mu + gap) * gate < m - gate:
                    continue
                lens, _ = levels(m, mu, [(gap, gate)])
                sigs = [(i, ln, i, None) for i, ln in enumerate(lens)]
                split = case in ("float", "above", "exact_above")
                T.add(t, "split", case, m, sigs, dict(rows=2, support=sorted([gate, m - gate])) if split else dict(rows=1, support=[m]))
            if m >= 3 * gate and m <= BIG:
                lens, _ = levels(m, mean, [(63, gate), (64, gate)])
                T.add(t, "split", "three", m, [(i, ln, i, None) for i, ln in enumerate(lens)],
                      dict(rows=3, support=sorted([gate, gate, m - 2 * gate])))


def _three(L, g, sizes):
    out = []
    for k, c in enumerate(sizes):
        out += [L + k * g] * c
    return out


def build_gate_order(T, sizes):
    """INDEL:163-166.  An allele of min(min_support, 5) - 1 members against one of min(min_support, 5); three alleles of
    equal (k, k, m - 2 k), ascending and descending size: emission is by count, stable.  The gaps are the smallest multiple of the
    lowest length that still splits (found per size with exact fractions).  Dropped sizes: none (order needs
    4 min(min_support, 5) + 3 signatures; a size where no gap below 50 times the lowest length splits would raise)."""
    gate = min(T.params.min_support, 5)
    rc = T.params.min_support
    for t in _indel_types():
        mean, ratio = inexact_mean(t)
        for m in sorted(set((max(rc, 2 * gate),) + tuple(sizes))):
            for case, c in (("gate_below", gate - 1), ("gate_at", gate)):
                if m > BIG and (case == "gate_at") != (m % 2 == 0):
                    continue
                if m - c < gate:
                    continue
                lens, _ = levels(m, mean, [(64, c)])
                e = dict(rows=2, support=sorted([c, m - c])) if c >= gate else dict(rows=1, support=[m - c])
                T.add(t, "gate", case, m, [(i, ln, i, None) for i, ln in enumerate(lens)], e)
        for m in sorted(set((max(rc, 4 * gate + 3),) + tuple(sizes))):
            if m < 4 * gate + 3:
                continue
            k = m // 3
            shapes = (("order_equal", (k, k, m - 2 * k)), ("order_ascending", (k - 1, k, m - 2 * k + 1)), ("order_descending", (m - 2 * k + 1, k, k - 1)))
            if m > BIG:
                shapes = shapes[:1] if m % 2 == 0 else shapes[2:]
            for case, cs in shapes:
                L = 100
                for j in range(1, 50):
                    lens = _three(L, j * L, cs)
                    if j * L > Fraction(str(ratio)) * Fraction(sum(lens), m) and j * L > ratio * (sum(lens) / m) + 1:
                        break
                else:
                    raise AssertionError(("no gap splits three alleles of these sizes", t, case, m))
                order = sorted(range(3), key=lambda a: cs[a])              # stable by count
                e = dict(rows=3, support=[cs[a] for a in order], len=[_len_print(t, L + a * j * L) for a in order])
                T.add(t, "order", case, m, [(i, ln, i, None) for i, ln in enumerate(lens)], e)


def build_remain(T, sizes):
    """INDEL:46-47, 169-187 under remain_reads_ratio rr < 1.  An allele of n members keeps K = max(int(rr n), 1).  By length: K core
    members at Lc, the others d = K + 2 below and above.  By position: K core members at P0 + d, the others at P0 and P0 + 2 d, and
    the core by position is not the core by length: the SHORTEST members (first in allele order) sit at P0 + 2 d.  So the cores are
    kept: POS = P0 + d, SVLEN = Lc - with K + 1 kept both move by more than 1.  n is the largest off-by-one n <= m - 3 of the table's
    ratio where there is one (`int`: int(rr n) is one below the exact floor: 0.7: 90, 170, 180 ...; 0.58: 50; 0.29: 100), and m
    (`whole`); the rest of the cluster is a second allele far above.  `tie`: one or two core members fewer and the others in equal
    numbers on both sides, so the last kept places are ties on opposite sides of the mean: the first in allele order wins - the
    upper position, the lower length.  `one`: rr n < 1 keeps the one member closest to the mean.
    Dropped sizes: `int` below n + 3 = 53 signatures (no such n exists, see the module text)."""
    rr = min(T.params.remain_reads_ratio, 1)
    gate = min(T.params.min_support, 5)
    for t in _indel_types():
        ratio = T.ratio(t)
        for m in sorted(set((T.params.min_support,) + tuple(sizes))):
            n_off = off_by_one(rr, m - gate) if m - gate >= 3 else None
            plans = []
            if n_off:
                plans.append(("int", n_off, 0))
            if m <= BIG or not n_off:
                plans.append(("whole", m, 0))
            if m <= BIG:
                plans.append(("tie", m, 1))
            for case, n, tie in plans:
                K = max(int(rr * n), 1)
                if case == "int":
                    assert K == (Fraction(str(rr)) * n).__floor__() - 1
                core = K - tie
                if tie and (n - core) % 2:
                    core -= 1
                slots = K - core
                lo = (n - core + 1) // 2
                hi = n - core - lo
                if K >= n or core < 1 or hi < slots or (tie and lo != hi):
                    continue
                d = K + 2
                Lc = int((d + 2) / ratio) + 2 * d + 20
                top = int((Lc + d) / (1 - ratio)) + Lc + 10                 # a second allele: its gap splits whatever the cluster's mean
                # members in length order: lo short ones (all at the upper position), core at Lc, hi long ones; the lower position
                # goes to the first `hi` members behind the short ones, the core position to the rest
                ln = [Lc - d] * lo + [Lc] * core + [Lc + d] * hi
                ps = [2 * d] * lo + [0] * hi + [d] * core
                rest = m - n
                sigs = [(ps[j], ln[j], j, None if j == n - 1 else 0) for j in range(n)]
                sigs += [(d, top, n + j, None if j == rest - 1 else 0) for j in range(rest)]
                pos = (K * d + slots * d) // K
                length = (K * Lc - slots * d) // K
                if rest < gate:
                    # (search_threshold is the first kept position: a core member, whatever the ties decide)
                    e = dict(rows=1, support=[n], len=[_len_print(t, length)], pos=[pos], search=d, search_alt=2 * d)
                elif rest < n:
                    e = dict(rows=2, support=[rest, n], len=[_len_print(t, top), _len_print(t, length)], pos=[d, pos])
                else:
                    e = dict(rows=2, support=[n, rest], len=[_len_print(t, length), _len_print(t, top)], pos=[pos, d])
                if t == "INS":
                    for k in ("pos", "search", "search_alt"):              # (POS and search are the position of the one member with a sequence)
                        e.pop(k, None)
                T.add(t, "remain", case, m, sigs, e)
            if rr * gate < 1 and gate == 3 and (m <= BIG or m % 2):
                # rr n < 1 keeps one: the member closest to the mean P0 + 27, the one at P0 + 31
                rest = m - 3
                sigs = [(0, 100, 0, None), (31, 100, 1, None), (50, 100, 2, None)] + [(25, 500, 3 + j, None) for j in range(rest)]
                e = dict(rows=1 + (rest >= gate), support=[3] + ([rest] if rest >= gate else []))
                e["pos"] = ([31] if t == "DEL" else [0]) + ([25] if rest >= gate else [])
                T.add(t, "remain", "one", m, sigs, e)


def build_kept(T, sizes):
    """rr >= 1 (clamped above 1): everything is kept, the mean is numpy's, and search_threshold is the member closest to the mean -
    on a tie the first in allele order.  `tie`: members at P0 - d and P0 + d only, the + d ones SHORTER (first in the allele's length
    order): search_threshold = P0 + d, the later position.  `mean`: an inexact mean (sizes 3, 7, 33, 63 besides the ladder)."""
    for t in _indel_types():
        for m in sorted(set((3, 7, 33, 63) + tuple(s for s in sizes if s <= BIG or s % 2))):
            # n - 1 members step 3 apart and one moved by 1: the mean is no integer multiple of 1 / 2
            sigs = [(3 * i + (1 if i == m - 1 else 0), 100 + (i % 3), i, None) for i in range(m)]
            tot = sum(s[0] for s in sigs)
            e = dict(rows=1, support=[m])
            if t == "DEL":
                e["pos"] = [tot // m]
                best = min(range(m), key=lambda i: (abs(Fraction(sigs[i][0]) - Fraction(tot, m)), (sigs[i][1], i)))
                e["search"] = sigs[best][0]
            T.add(t, "kept", "mean", m, sigs, e)
        for m in sorted(set((4,) + tuple(s for s in sizes if s <= BIG or s % 2 == 0))):
            if m % 2:
                continue
            d = 40
            sigs = [(0, 110, i, None) for i in range(m // 2)] + [(2 * d, 100, m // 2 + i, None) for i in range(m // 2)]
            e = dict(rows=1, support=[m])
            if t == "DEL":
                e.update(pos=[d], search=2 * d, search_alt=0)
            T.add(t, "kept", "tie", m, sigs, e)


def build_ins_pick(T, sizes):
    """INDEL:398-405 (INS only).  len(seq) == int(signalLen) against one less: members 0 .. j - 1 carry 99 bases, member j = 3 m // 4
    exactly 100, POS moves to ITS position and search_threshold with it; an allele without a qualifying sequence is dropped while
    its neighbours stay."""
    gate = min(T.params.min_support, 5)
    for m in sorted(set((3,) + tuple(sizes))):
        j = 3 * m // 4
        sigs = [(50 * i, 100, i, 99 if i < j else 100) for i in range(m)]
        T.add("INS", "pick", "first", m, sigs, dict(rows=1, support=[m], pos=[50 * j], len=[100], seq_of=j, search=50 * j, search_alt=25 * (m - 1)))
    for m in sorted(set((3 * gate,) + tuple(s for s in sizes if s <= BIG))):
        if m < 3 * gate:
            continue
        k = m // 3
        cs = (k, k, m - 2 * k)
        lens = _three(100, 300, cs)
        mid = set(range(k, 2 * k))
        sigs = [(i, ln, i, (ln - 1) if i in mid else None) for i, ln in enumerate(lens)]
        T.add("INS", "pick", "none", m, sigs, dict(rows=2, support=[k, m - 2 * k], len=[100, 700]))


# ------------------------------------------------------------------------------------------------ DUP / INV / TRA rules
def _q(vals):
    """the DUP quantile rule (DUP:99-109) on a list in pos2 order, in integers"""
    n = len(vals)
    lo, hi = (4 * n) // 10, (6 * n) // 10
    assert lo == int(n * 0.4) and hi == int(n * 0.6)
    return vals[lo] if lo == hi else sum(vals[lo:hi]) // (hi - lo)


def build_dup(T, sizes):
    """DUP:79-131.  `gap`: sub-clusters by pos2 - m - 7 signatures at Q, one at Q + bias (stays), three at Q + 2 bias + 1 (breaks;
    a row), three more a bias + 1 further from TWO reads (read_count signatures, read_count - 1 reads: no row).  `reads`: m
    signatures of read_count - 1 reads.  `quant`: one sub-cluster of m, the quantile rule in integers; with min_support = 1 every n
    in 1 .. 20 (int(0.4 n) == int(0.6 n) at 1 and 3 only).  `size`: bp2 - bp1 at min_size - 1, min_size, max_size, max_size + 1.
    Dropped sizes: none (minimum read_count + 7 for `gap`)."""
    p = T.params
    rc, b = p.min_support, p.max_cluster_bias_DUP
    ladder = tuple(s for s in LADDER_PAIR if s in sizes)
    if rc == 1:
        for n in range(1, 21):
            p1 = [11 * j + (j * j) % 5 for j in range(n)]
            p2 = [2000 + 3 * j for j in range(n)]
            T.add("DUP", "quant", "n%d" % n, n, [(p1[j], p2[j], j, None) for j in range(n)], dict(rows=1, support=[n], pos=[_q(p1)], len=[_q(p2) - _q(p1)]))
        return
    for m in sorted(set((rc + 7,) + ladder)):
        Q = 3000
        sigs = [(i, Q, i, None) for i in range(m - 7)] + [(m - 7, Q + b, m - 7, None)] + [(m - 6 + j, Q + 2 * b + 1, m - 6 + j, None) for j in range(3)]
        sigs += [(m - 3 + j, Q + 3 * b + 2, m - 3 + (j % 2), None) for j in range(3)]
        n0 = m - 6
        lo, hi = (4 * n0) // 10, (6 * n0) // 10
        bp1 = lo if lo == hi else (lo + hi - 1) // 2
        T.add("DUP", "dup_gap", "gap", m, sigs, dict(rows=2, support=[m - 6, 3], pos=[bp1, m - 5], len=[Q - bp1, Q + 2 * b + 1 - (m - 5)]))
    for m in sorted(set((rc,) + ladder)):
        T.add("DUP", "dup_reads", "reads", m, [(i, 3000, i % (rc - 1), None) for i in range(m)], dict(rows=0))
        p1 = [11 * j + (j * j) % 5 for j in range(m)]
        p2 = [40000 + 3 * j for j in range(m)]
        T.add("DUP", "quant", "ladder", m, [(p1[j], p2[j], j, None) for j in range(m)], dict(rows=1, support=[m], pos=[_q(p1)], len=[_q(p2) - _q(p1)]))
    _size_filter(T, "DUP", ladder)


def _size_filter(T, t, ladder):
    p = T.params
    rc = p.min_support
    for m in sorted(set((rc,) + ladder)):
        cases = [("min_below", p.min_size - 1, 0), ("min_at", p.min_size, 1)]
        if p.max_size == -1:
            cases += [("unlimited", 100001, 1)]
        else:
            cases += [("max_at", p.max_size, 1), ("max_above", p.max_size + 1, 0)]
        if m > BIG:
            cases = cases[:2] if m % 2 == 0 else cases[2:]
        for case, ln, rows in cases:
            T.add(t, "size", case, m, [(0, ln, i, None) for i in range(m)], dict(rows=rows, support=[m], pos=[0], len=[ln]) if rows else dict(rows=0))


def _half_even(x2):
    """round(x2 / 2) as Python rounds: half to even"""
    q, r = divmod(x2, 2)
    return q if r == 0 else q + (q & 1)


def build_inv(T, sizes):
    """INV:101-203.  `half`: the quotients temp_sum / temp_count land on x.5 (half of an even number of signatures at (P, Q), half at
    (P + 1, Q + 1)) with x even for one breakpoint and odd for the other, both ways round; an odd m adds one signature whose pos2
    falls back by more than the bias (no chain break: the gap is signed; its own sub-cluster, dropped).  `reads_sub`: a sub-cluster
    of read_count signatures from read_count - 1 reads beside a good one.  `reads`: the whole cluster so (up to 257 signatures).  `size`: as for DUP.
    Dropped sizes: none (an x.5 quotient needs an even count: an odd m is m - 1 such signatures and the one more)."""
    p = T.params
    rc, b = p.min_support, p.max_cluster_bias_INV
    ladder = tuple(s for s in LADDER_PAIR if s in sizes)
    for m in sorted(set((4,) + ladder)):
        for case, par in (("even_odd", 0), ("odd_even", 1)):
            if m > BIG and par != m % 2:
                continue
            n = m - (m % 2)
            base = T.cur["INV"]
            P = (par - base) % 2                                       # base + P has parity par
            Q = 5000 + ((1 - par - base - 5000) % 2)                    # base + Q has the other parity
            sigs = [(P, Q, i, None) for i in range(n // 2)] + [(P + 1, Q + 1, n // 2 + i, None) for i in range(n // 2)]
            if m % 2:
                sigs.append((P + 2, Q - b - 100, n, None))
            T.add("INV", "half", case, m, sigs, dict(rows=1, support=[n], half2=[2 * P + 1, 2 * Q + 1]))
    for m in sorted(set((2 * rc,) + ladder)):
        sigs = [(i % 2, 5000, i, None) for i in range(m - rc)] + [(2, 5000 - b - 1 - j, m - rc + (j % (rc - 1)), None) for j in range(rc)]
        T.add("INV", "inv_reads", "reads_sub", m, sigs, dict(rows=1, support=[m - rc]))
    for m in sorted(set((rc,) + tuple(s for s in ladder if s <= BIG))):
        T.add("INV", "inv_reads", "reads", m, [(i, 5000, i % (rc - 1), None) for i in range(m)], dict(rows=0))
    _size_filter(T, "INV", ladder)


def build_tra(T, sizes):
    """TRA:106-254.  `double`: one sub-cluster whose first element in pos2 order (the LAST position) is counted twice: both
    breakpoints are int((sum + first) / (n + 1)).  `tie`: two sub-clusters with equal distinct counts, the first maximum (the lower
    pos2) leads and is the one with the doubled element.  `su`: the second allele at 0.5 read_count - su = ceil(rc / 2) - 1 (odd rc:
    (rc - 1) / 2) gives one row, su = ceil(rc / 2) two.  `ratio`: distinct reads on m * ratio, m counting repeated reads, and one
    below, for one allele (bu) and for two (bu + su).  `unknown`: a BND code above 3 gives nothing (up to 65 signatures).
    Dropped sizes: `sum_*` where ceil(ratio m) - su leaves the first allele smaller than the second or above m - su."""
    p = T.params
    rc, b, ratio = p.min_support, p.max_cluster_bias_TRA, p.diff_ratio_filtering_TRA
    ladder = tuple(s for s in LADDER_PAIR if s in sizes)
    fr = Fraction(str(ratio))
    for m in sorted(set((rc,) + ladder)):
        # pos2 falls as pos1 rises
        sigs = [(j, 900 + (m - 1 - j), j, None) for j in range(m)]
        bp1 = (sum(range(m)) + (m - 1)) // (m + 1)
        bp2 = (sum(900 + j for j in range(m)) + 900) // (m + 1)
        T.add("TRA", "double", "double", m, sigs, dict(rows=1, support=[m], pos=[bp1], pos2=[bp2]))
    for m in sorted(set((2 * rc,) + ladder)):
        if m <= BIG or m % 2:
            k1 = m // 2
            k0 = m - k1
            # sub-cluster 0 at pos2 = 900 .. (k0 elements, one repeated read when m is odd), sub-cluster 1 a bias + 1 above
            s0 = [(2 * j, 900 + (j % 7), min(j, k1 - 1), None) for j in range(k0)]
            s1 = [(2 * j + 1, 900 + 6 + b + 1 + (j % 5), k0 + j, None) for j in range(k1)]
            first = min(range(k0), key=lambda j: (s0[j][1], s0[j][0]))
            bp1_0 = (sum(s[0] for s in s0) + s0[first][0]) // (k0 + 1)
            bp2_0 = (sum(s[1] for s in s0) + s0[first][1]) // (k0 + 1)
            bp1_1 = sum(s[0] for s in s1) // k1
            bp2_1 = sum(s[1] for s in s1) // k1
            T.add("TRA", "tie", "tie", m, s0 + s1, dict(rows=2, support=[k1, k1], pos=[bp1_0, bp1_1], pos2=[bp2_0, bp2_1]))
    su_hi = (rc + 1) // 2
    for m in sorted(set((max(rc, 4 * su_hi),) + ladder)):
        for case, su in (("su_below", su_hi - 1), ("su_at", su_hi)):
            if (m > BIG and (case == "su_at") != (m % 2 == 0)) or su < 1:
                continue
            assert (su >= 0.5 * rc) == (case == "su_at")
            s0 = [(j, 900 + (j % 7), j, None) for j in range(m - su)]
            s1 = [(m - su + j, 900 + 6 + b + 1, m - su + j, None) for j in range(su)]
            assert m - su >= fr * m
            T.add("TRA", "su", case, m, s0 + s1, dict(rows=2, support=[m - su, su]) if case == "su_at" else dict(rows=1, support=[m - su]))
    for m in sorted(set((10,) + ladder)):
        need = -((-fr * m).__floor__())                                 # ceil(ratio m)
        assert (need >= ratio * m) and not (need - 1 >= ratio * m)
        for case, u, two in (("bu_at", need, 0), ("bu_below", need - 1, 0), ("sum_at", need, 1), ("sum_below", need - 1, 1)):
            if m > BIG and case != ("bu_at", "bu_below")[m % 2]:
                continue
            if two:
                su = su_hi
                bu = u - su
                if bu < su or bu < 1 or m - su < bu:
                    continue
                s0 = [(j, 900 + (j % 7), j % bu, None) for j in range(m - su)]
                s1 = [(m - su + j, 900 + 6 + b + 1, bu + j, None) for j in range(su)]
                e = dict(rows=2, support=[bu, su]) if u >= need else dict(rows=0)
                sigs = s0 + s1
            else:
                if u < rc:
                    continue
                sigs = [(j, 900 + (j % 7), j % u, None) for j in range(m)]
                e = dict(rows=1, support=[u]) if u >= need else dict(rows=0)
            T.add("TRA", "ratio", case, m, sigs, e)
    for m in sorted(set((rc,) + tuple(s for s in ladder if s <= 65))):
        T.add("TRA", "unknown", "code", m, [(j, 900, j, None) for j in range(m)], dict(rows=0), bnd="X", chr2="3")


# ------------------------------------------------------------------------------------------------ the tables
def _params(**kw):
    base = dict(min_support=3, min_size=30, max_size=100000, max_cluster_bias_DEL=100, max_cluster_bias_INS=100, diff_ratio_merging_DEL=0.7,
                diff_ratio_merging_INS=0.35, max_cluster_bias_DUP=500, max_cluster_bias_INV=500, max_cluster_bias_TRA=50,
                diff_ratio_filtering_TRA=0.6, remain_reads_ratio=1.0)
    base.update(kw)
    return Params(**base)


ALL = tuple(sorted(set(LADDER_INDEL + LADDER_PAIR)))
SMALL = tuple(s for s in ALL if s <= BIG)
WIDE = dict(max_cluster_bias_DEL=3000, max_cluster_bias_INS=3000)


def tables(variant="a"):
    """the tables of a variant: "a" as built, "b" = "a" shifted (applied by case_inputs), "c" the INDEL rules with two position
    groups 270 000 apart under a bias of 300 000, "d" genotyped"""
    check_products()
    out = []
    if variant == "c":
        T = Table("far", _params(max_cluster_bias_DEL=FAR_BIAS, max_cluster_bias_INS=FAR_BIAS), spacing=2 * FAR_BIAS + 100000, far=True)
        build_chain_indel_only(T, SMALL)
        for f in (build_dedupe, build_split, build_gate_order, build_kept, build_ins_pick):
            f(T, SMALL)
        T2 = Table("far_keep", _params(max_cluster_bias_DEL=FAR_BIAS, max_cluster_bias_INS=FAR_BIAS, remain_reads_ratio=0.7), spacing=2 * FAR_BIAS + 100000, far=True)
        build_remain(T2, SMALL)
        return [T, T2]
    gt = dict(genotype=True) if variant == "d" else {}
    sizes = SMALL if variant == "d" else ALL
    T = Table("base", _params(**gt))
    for f in (build_chain, build_dedupe, build_split, build_gate_order, build_kept, build_ins_pick, build_dup, build_inv, build_tra):
        f(T, sizes)
    out.append(T)
    T = Table("support10", _params(min_support=10, **gt))
    for f in (build_chain, build_gate_order, build_dedupe, build_tra):
        f(T, SMALL)
    out.append(T)
    for name, rr in (("keep70", 0.7), ("keep58", 0.58), ("keep29", 0.29)):
        T = Table(name, _params(remain_reads_ratio=rr, **dict(WIDE, **gt)), spacing=12000)
        build_remain(T, sizes if name == "keep70" else SMALL)
        out.append(T)
    T = Table("clamp", _params(remain_reads_ratio=1.5, **gt))
    build_kept(T, SMALL)
    build_dedupe(T, (16, 33, 65))
    out.append(T)
    T = Table("unlimited", _params(max_size=-1, min_support=1, **gt))
    build_dup(T, ())
    _size_filter(T, "DUP", (64, 65))
    _size_filter(T, "INV", (64, 65))
    out.append(T)
    return out


def build_chain_indel_only(T, sizes):
    rc = T.params.min_support
    for t in ("DEL", "INS"):
        b = T.bias(t)
        for m in sorted(set((rc,) + tuple(sizes))):
            sigs = [(i * b, 100, i, None) for i in range(m)] + [((m - 1) * b + b + 1 + j, 100, m + j, None) for j in range(rc)]
            T.add(t, "chain", "bias", m, sigs, dict(rows=2, support=[m, rc]))


# ------------------------------------------------------------------------------------------------ reads tables of variant (d)
def site_reads(T):
    """every signature's read spans its site; three reads more per site that support nothing; and per DEL / INS site a ladder of
    eight non-supporting reads whose starts step across the left ends of the windows the site's calls can have, so that DR
    says where search_threshold is.  No window has zero width (the biases are positive)."""
    reads = []
    for s in T.sites:
        lo, hi, sid = s["lo"], s["hi"], s["id"]
        names = sorted({x[{"DEL": 2, "INS": 2, "DUP": 2, "INV": 3, "TRA": 4}[s["type"]]] for x in T.per[s["type"]]
                        if ("n%04d_" % sid) == x[{"DEL": 2, "INS": 2, "DUP": 2, "INV": 3, "TRA": 4}[s["type"]]][:6]})
        right = hi + 3000
        for nm in names:
            reads.append((max(lo - 3000, 0), right, 1, nm, "1"))
        for j in range(3):
            reads.append((max(lo - 3000 - j, 0), right, 1, "x%04d_%d" % (sid, j), "1"))
        for k, start in enumerate(ladder_starts(T, s)):
            reads.append((start, right, 1, "y%04d_%d" % (sid, k), "1"))
    return reads


def ladder_starts(T, s):
    if s["type"] not in ("DEL", "INS"):
        return []
    half = T.bias("DEL") if s["type"] == "DEL" else INS_HALF
    step = max(1, (s["hi"] - s["lo"]) // 7)
    out = [max(s["lo"] - half + k * step, 0) for k in range(8)]
    e = s["expect"]
    if "search_alt" in e:                                   # one read starts on the left end of the later of the two windows
        out[7] = max(e["search"], e["search_alt"]) - half
    return out


def expected_dr(T, s, search, support):
    """DR of a call of site s whose window is centred on `search`: the site's reads that are not in the support, the three spanning
    reads and the ladder reads that start at or left of the window"""
    half = T.bias("DEL") if s["type"] == "DEL" else INS_HALF
    left = max(search - half, 0)
    return s["n_names"] - support + 3 + sum(1 for x in ladder_starts(T, s) if x <= left)


# ------------------------------------------------------------------------------------------------ cases
VARIANTS = ("a", "b", "c", "d")
_FULL = ("base", "support10", "keep70", "keep58", "keep29", "clamp", "unlimited")
TABLE_NAMES = {"a": _FULL, "b": _FULL, "c": ("far", "far_keep"), "d": _FULL}
CASE_NAMES = tuple("%s_%s" % (v, n) for v in VARIANTS for n in TABLE_NAMES[v])


def _build_cases():
    out = []
    for v in VARIANTS:
        for T in tables("a" if v == "b" else v):
            reads = site_reads(T) if v == "d" else []
            per, sites = T.per, T.sites
            if v == "b":
                per, reads, sites = shifted(per, reads, sites, SHIFT)
            out.append(dict(name="%s_%s" % (v, T.name), variant=v, table=T, params=T.params, per=per, reads=reads, sites=sites))
    return out


_CASES = []


def cases():
    """[dict(name, variant, table, params, per, reads, sites)] of every table and variant, built once"""
    if not _CASES:
        _CASES.extend(_build_cases())
        assert tuple(c["name"] for c in _CASES) == CASE_NAMES
    return _CASES


def case(name):
    return cases()[CASE_NAMES.index(name)]


_STORES = {}


def store_of(case):
    if case["name"] not in _STORES:
        _STORES[case["name"]] = SigStore.from_tuple_lists(case["per"], case["reads"] or None, chroms=["1", "2", "3"])
    return _STORES[case["name"]]


def input_digest(st):
    h = hashlib.sha256()
    for k in ("a", "b", "read_id", "aux", "reads_off", "r_start", "r_end", "r_primary", "r_id"):
        v = getattr(st, k)
        h.update(k.encode())
        if v is not None:
            h.update(np.ascontiguousarray(v, dtype=np.int64).tobytes())
    h.update(repr(sorted((t, c, int(b), int(e)) for (t, c), (b, e) in st.seg_index.items())).encode())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------ rows
LONG = 64                           # read lists longer than this are recorded as a hash of their sorted names


def slim_row(t, row):
    """a row with a long read list replaced by sha256 of its sorted names; DUP / TRA lists (Python set order in the reference) sorted"""
    from helpers import READS_FIELD, SET_ORDER_TYPES
    row = list(row)
    k = READS_FIELD[t]
    names = row[k].split(",")
    if t in SET_ORDER_TYPES:
        names = sorted(names)
        row[k] = ",".join(names)
    if len(names) > LONG:
        row[k] = "sha256:" + hashlib.sha256(",".join(sorted(names)).encode()).hexdigest()
    return row


def rows_of_site(rows, s):
    return [r for r in rows if s["lo"] <= int(r[2]) <= s["hi"]]


def check_landing(case, rows_by_type, collect=None):
    """every site's expectation against rows {type: [row]} (read lists may be hashed); returns the number of checks made.
    collect: a list that takes the failures' messages instead of the first one being raised"""
    n = 0
    for s in case["sites"]:
        try:
            n += _check_site(case, s, rows_of_site(rows_by_type.get(s["type"], []), s))
        except AssertionError as err:
            if collect is None:
                raise
            collect.append(str(err))
    return n


def _check_site(case, s, got):
    from helpers import READS_FIELD
    T, t, e = case["table"], s["type"], s["expect"]
    where = "%s site %d %s/%s/%s m=%d" % (case["name"], s["id"], t, s["rule"], s["case"], s["m"])
    assert len(got) == e["rows"], "%s: %d rows, expected %d: %s" % (where, len(got), e["rows"], [r[:6] for r in got])
    if "support" in e and e["rows"]:
        assert [int(r[SUPPORT_IDX[t]]) for r in got] == e["support"], "%s: supports %s, expected %s" % (where, [r[SUPPORT_IDX[t]] for r in got], e["support"])
    if "pos" in e:
        assert [int(r[2]) for r in got] == e["pos"], "%s: POS %s, expected %s" % (where, [r[2] for r in got], e["pos"])
    if "len" in e:
        assert [int(r[3]) for r in got] == e["len"], "%s: lengths %s, expected %s" % (where, [r[3] for r in got], e["len"])
    if "half2" in e:
        bp1, bp2 = _half_even(e["half2"][0]), _half_even(e["half2"][1])
        assert (2 * bp1 < e["half2"][0]) != (2 * bp2 < e["half2"][1]), "%s: both quotients round the same way" % where
        assert [int(got[0][2]), int(got[0][3])] == [bp1, bp2 - bp1], "%s: POS, length %s, expected %s" % (where, got[0][2:4], [bp1, bp2 - bp1])
    if "pos2" in e:
        assert [int(r[4]) for r in got] == e["pos2"], "%s: second positions %s, expected %s" % (where, [r[4] for r in got], e["pos2"])
    if "first_name" in e and not got[0][READS_FIELD[t]].startswith("sha256:"):
        assert got[0][READS_FIELD[t]].split(",")[0] == e["first_name"], "%s: first name %s" % (where, got[0][READS_FIELD[t]][:40])
    if "seq_of" in e:
        k = int(e["seq_of"][-5:])
        assert got[0][13] == ("ACGT" * 30)[k % 4:k % 4 + 100], "%s: sequence" % where
    if "search" in e and case["variant"] == "d" and len(got) == 1:
        sup = int(got[0][SUPPORT_IDX[t]])
        want = expected_dr(T, s, e["search"], sup)
        assert int(got[0][DR_IDX[t]]) == want, "%s: DR %s, expected %d" % (where, got[0][DR_IDX[t]], want)
        if "search_alt" in e:
            assert expected_dr(T, s, e["search_alt"], sup) != want, "%s: the other search_threshold gives the same DR" % where
    return len(e)


def cluster_cells(case, st, cluster_id):
    """{(rule, type, tier)} of the sites whose claimed cluster is there: a chained cluster of exactly m signatures among the site's"""
    cells, missing = set(), []
    sizes = np.bincount(cluster_id[cluster_id >= 0])
    for s in case["sites"]:
        if not s["claim"]:
            continue
        beg, end = st.seg_index[(s["type"], "1")]
        a = st.a[beg:end]
        idx = beg + np.flatnonzero((a >= s["lo"]) & (a <= s["hi"]))
        assert len(idx) == s["n_sig"], (case["name"], s["id"], len(idx), s["n_sig"])
        ms = set(sizes[np.unique(cluster_id[idx])].tolist())
        if s["m"] in ms:
            cells.add((s["rule"], s["type"], tier_of(s["type"], s["m"])))
        else:
            missing.append((s["id"], s["rule"], s["case"], s["m"], sorted(ms)))
    return cells, missing


# what every variant's tables together must cover: rule -> types; every tier of the type's ladder, every rule
RULES = {"chain": TYPES, "dedupe": ("DEL", "INS"), "split": ("DEL", "INS"), "gate": ("DEL", "INS"), "order": ("DEL", "INS"),
         "remain": ("DEL", "INS"), "kept": ("DEL", "INS"), "pick": ("INS",), "dup_gap": ("DUP",), "dup_reads": ("DUP",), "quant": ("DUP",),
         "size": ("DUP", "INV"), "half": ("INV",), "inv_reads": ("INV",), "double": ("TRA",), "tie": ("TRA",), "su": ("TRA",), "ratio": ("TRA",)}


def claimed_cells(variant):
    """the (rule, type, tier) cells a variant claims: every tier for "a" and "b", the tiers up to 257 signatures for "c" (INDEL rules
    only) and "d\""""
    out = set()
    for rule, types in RULES.items():
        for t in types:
            if variant == "c" and t not in ("DEL", "INS"):
                continue
            for tier in TIERS[t]:
                if variant in ("c", "d") and tier == "scratch":
                    continue
                out.add((rule, t, tier))
    return out
