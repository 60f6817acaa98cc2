"""Crafted batches for the last stage every call passes through - order, emit, publish (k_items_scan, k_emit with emit_item_serial,
k_publish) - and a plain restatement of the order the calls and their support lists must come out in ("Emit seams").

A table is a list of clusters in input order, every one of them a work item (at least read_count signatures), so the position of a
cluster in the list IS its item index: the 8-item tile of a k_emit wavefront, the 512-item piece and the 4096-item chunk of
k_items_scan and the 65th chunk (item 266 240, the first whose tile folds more than 64 chunk totals) can be aimed at by counting.
The small tables (A - D, F) are built as the reference's tuple lists (a SigStore: read names, INS sequences, a reads table for F), so
that the reference's own resolvers can be run on them (tests/golden/make_golden_emit.py); the large ones (E) as numpy columns.  Both
are chain_helpers.Case objects: chain_helpers.restate gives the clusters and the work items, expected_calls applies
oracle/py_restatement.py's indel_cluster / dup_cluster / inv_cluster / tra_cluster to each and lists the calls (segment, cluster, bp1,
bp2, support) and each call's support rows in emit order: items in input order, the calls of an item in slot order.

Which alleles / sub-clusters occupy a temp slot (kernels.hip.h: `npass` of refine_indel and of the register tier, `carry_slot` of the
DUP / INV path, `ne` of TRA):
  * DEL / INS: an allele below min(min_support, 5) reads gets NO slot - the slot index is the rank among the passing alleles only and
    nslots = npass.  An INS allele that passes the count but has no sequence of the wanted length keeps its slot with valid = 0.
  * DUP / INV: a sub-cluster below read_count (reads; INV also signatures) gets NO slot (`pass`); one that passes and then fails the
    size filter (min_size / max_size) keeps its slot with valid = 0.
  * TRA: one slot per emitted group (1 or 2), all valid.
So nslots >= the number of valid calls, the serial path (nslots > 8) is reached by 9 valid calls, and an invalid slot BETWEEN valid
ones exists only as an INS allele without a sequence (any rank) or a DUP / INV sub-cluster at the low (min_size) or high (max_size)
end.  The tables hold both kinds: groups below the count (no slot) and invalid slots, each as the lowest, a middle and the highest.

Every landing check is evaluated on the ORACLE's result (items_of), not on what the builders meant."""
import hashlib

import numpy as np

from cutesv_amd.columns import Params, SigStore, TYPES, segment_record
import chain_helpers as ch

EM_TILE, PIECE, CHUNK = 8, 512, 4096
FOLD = 65 * CHUNK                                          # item 266 240: the first whose tile has nchunk > 64
KS = (1, 2, 3, 7, 8, 9, 16, 63, 64, 65, 130)               # calls per item (cell A)
INV_KS = (2, 9)
LENGTHS = (1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 257)            # support-list lengths (cell D)
E_SIZES = (1, 7, 8, 9, 511, 512, 513, 4095, 4096, 4097, 8192, 8193, 266239, 266240, 266241, 270337)
E_SEAMS = (EM_TILE, PIECE, CHUNK, 2 * CHUNK, FOLD)
E_ROUTED = tuple(n for n in E_SIZES if n <= 8193)          # through oneshot / int32 / resident; the others through int32 / resident
SMALL_TABLES = ("A", "B", "C1", "C7", "C8", "D", "F")      # recorded against the reference (emit_edges.json.gz)
LONG = 64                                                  # read lists / sequences longer than this are recorded as a hash


def base_params(**kw):
    d = dict(min_support=3, diff_ratio_merging_DEL=0.005, diff_ratio_merging_INS=0.005, max_size=-1)
    d.update(kw)
    return Params(**d)


# ------------------------------------------------------------------------------------------------ the case
class EmitCase(ch.Case):
    """a chain_helpers.Case whose segments carry the table's Params (columns.segment_record) and whose read ids are the store's;
    store: the SigStore of a small table (None for the numpy-built ones); memo: expected_calls may restate one cluster per shape"""

    def __init__(self, name, params, segs, a, b, aux, rid, cells, checks, store=None, reads=None, only32=False, memo=False):
        super().__init__(name, 0, name, segs, a, b, aux, cells, checks, reads=reads, only32=only32)
        self.params, self.store, self.memo = params, store, memo
        self.rid = np.asarray(rid, np.int32)

    def segment_table(self):
        from cutesv_amd import _abi
        recs = [segment_record(s["type"], s["chrom"], beg, end, self.params) for s, (beg, end) in zip(self.segs, self.bounds())]
        return np.array(recs, dtype=_abi.SEGMENT_DTYPE)


def seg_of(params, t, n, chrom=0):
    return dict(type=t, n=int(n), bias=getattr(params, "max_cluster_bias_" + t), rc=params.min_support, chrom=chrom,
                genotype=bool(params.genotype and (t != "TRA" or params.genotype_tra)))


def case_from_store(name, st, params, cells, checks):
    segs, w = [], 0
    for t, c in st.tasks():
        beg, end = st.seg_index[(t, c)]
        assert beg == w, (name, t, c)
        segs.append(seg_of(params, t, end - beg, st.chroms.index(c)))
        w = end
    assert w == st.n_sig
    reads = None
    if params.genotype and st.reads_off is not None:
        reads = (len(st.chroms), st.reads_off, st.r_start, st.r_end, st.r_primary, st.r_id)
    return EmitCase(name, params, segs, st.a, st.b, st.aux, st.read_id, cells, checks, store=st, reads=reads)


# ------------------------------------------------------------------------------------------------ the plain restatement of the order
class Nm(str):
    """a read name that remembers the row it came from (equal and hashed as the name: the rules dedupe by read)"""


def _nm(rid, row):
    x = Nm("%d" % rid)
    x.row = row
    return x


def _cluster_calls(case, t, first, size, cols):
    """[(bp1, bp2, support, [support rows])] of one cluster in slot order, by oracle/py_restatement.py's rule of the type"""
    from oracle import py_restatement as py
    a, b, x, rid = cols
    p, rc, out = case.params, case.params.min_support, []
    rows = range(first, first + size)
    if t in ("DEL", "INS"):
        seq = (lambda i: "A" * x[i]) if t == "INS" else (lambda i: None)
        members = [(a[i], b[i], _nm(rid[i], i), seq(i)) for i in rows]
        py.indel_cluster(members, "c", t, rc, getattr(p, "diff_ratio_merging_" + t), min(rc, 5), min(p.remain_reads_ratio, 1), True, out)
        return [(o[2], abs(o[3]), o[4], [n.row for n in o[8]]) for o in out]
    if t == "DUP":
        py.dup_cluster([(a[i], b[i], _nm(rid[i], i)) for i in rows], "c", rc, p.max_cluster_bias_DUP, p.min_size, p.max_size, True, out)
        # (the rule keeps a set of names: the support rows are each read's first signature in the sub-cluster's pos2 order)
        return [(o[2], o[3], len(o[4]), sorted((n.row for n in o[4]), key=lambda r: (b[r], r))) for o in out]
    if t == "INV":
        py.inv_cluster([(a[i], b[i], _nm(rid[i], i), x[i]) for i in rows], "c", rc, p.max_cluster_bias_INV, p.min_size, p.max_size, True, out)
        return [(int(o[2]), int(o[7]), o[4], [n.row for n in o[6]]) for o in out]
    members = [(a[i], b[i], _nm(rid[i], i), "ABCDXXXX"[x[i] & 7], x[i] >> 3) for i in rows]
    py.tra_cluster(members, "c", "c2", rc, p.diff_ratio_filtering_TRA, p.max_cluster_bias_TRA, out)
    seen = {}
    for e in sorted(members, key=lambda e: e[1]):
        seen.setdefault(str(e[2]), e[2].row)
    return [(int(o[2]), int(o[4]), int(o[5]), sorted((seen[n] for n in o[11].split(",")), key=lambda r: (b[r], r))) for o in out]


def expected_calls(case, r):
    """(calls: int64 array [n, 5] of (segment, cluster, bp1, bp2, support); support rows of all calls back to back) in emit order.
    case.memo (the large DEL tables): a cluster's calls depend on its positions only through their differences (the means are of exact
    integer sums and lie at least 1 / n off an integer or on it), so one cluster per shape is restated and moved."""
    cols = (case.a.tolist(), case.b.tolist(), case.aux.tolist(), case.rid.tolist())
    a, b = cols[0], cols[1]
    calls, sup, memo = [], [], {}
    for first, size, k in r["items"]:
        t = case.segs[k]["type"]
        cid = r["cluster_id"][first]
        if case.memo and t == "DEL":
            key = (tuple(a[i] - a[first] for i in range(first, first + size)), tuple(b[first:first + size]))
            if key not in memo:
                memo[key] = [(b1 - a[first], b2, n, [w - first for w in rows]) for b1, b2, n, rows in _cluster_calls(case, t, first, size, cols)]
            got = [(b1 + a[first], b2, n, [w + first for w in rows]) for b1, b2, n, rows in memo[key]]
        else:
            got = _cluster_calls(case, t, first, size, cols)
        for b1, b2, n, rows in got:
            assert n == len(rows)
            calls.append((k, cid, b1, b2, n))
            sup += rows
    return np.array(calls, np.int64).reshape(-1, 5), np.array(sup, np.int64)


def assert_order_is_expected(res, want_calls, want_sup, where=""):
    """a trimmed result against expected_calls, directly"""
    got = np.stack([np.asarray(res[f], np.int64) for f in ("call_seg", "call_cluster", "bp1", "bp2", "support")], axis=1) if len(res["bp1"]) else np.zeros((0, 5), np.int64)
    assert got.shape == want_calls.shape, "%s: %d calls, the restatement has %d" % (where, len(got), len(want_calls))
    bad = np.flatnonzero((got != want_calls).any(axis=1))
    assert len(bad) == 0, "%s: call %d is %s, the restatement says %s" % (where, bad[0], got[bad[0]].tolist(), want_calls[bad[0]].tolist())
    off = np.concatenate([[0], np.cumsum(want_calls[:, 4])])
    assert np.array_equal(np.asarray(res["support_off"], np.int64), off), "%s: support_off" % where
    gs = np.asarray(res["support_sig"], np.int64)
    assert gs.shape == want_sup.shape and np.array_equal(gs, want_sup), "%s: support rows differ from the restatement (first at %s)" % (
        where, np.flatnonzero(gs != want_sup)[:3] if gs.shape == want_sup.shape else "len")


# ------------------------------------------------------------------------------------------------ landing, from the oracle's result
def items_of(case, want):
    """the work items as the ORACLE's result shows them: the clusters (cluster_id) of at least read_count signatures of their segment, in
    order -> dict(cid, seg, first, size, ncalls: arrays per item; sup: per item the supports of its calls in call order)"""
    cid = np.asarray(want["cluster_id"])
    assert (cid >= 0).all() and (np.diff(cid) >= 0).all()
    ids, first, size = np.unique(cid, return_index=True, return_counts=True)
    ends = np.cumsum([s["n"] for s in case.segs])
    seg = np.searchsorted(ends, first, side="right")
    rc = np.array([s["rc"] for s in case.segs])[seg]
    item = size >= rc
    ids, first, size, seg = ids[item], first[item], size[item], seg[item]
    cc = np.asarray(want["call_cluster"])
    assert np.isin(cc, ids).all(), "a call names a cluster that is no work item"
    ncalls = np.bincount(cc, minlength=int(want["n_clusters"]))[ids]
    order = np.argsort(cc, kind="stable")
    cut = np.concatenate([[0], np.cumsum(ncalls)])
    support = np.asarray(want["support"])[order]
    return dict(cid=ids, seg=seg, first=first, size=size, ncalls=ncalls, sup=lambda i: support[cut[i]:cut[i + 1]].tolist())


def check_landing(case, want):
    """every check of the case on the oracle's trimmed result; returns how many were made"""
    it = items_of(case, want)
    n = len(it["cid"])
    gt = np.array([s["genotype"] for s in case.segs])[it["seg"]]
    for chk in case.checks:
        kind, arg = chk[0], chk[1:]
        if kind == "n_items":
            assert n == arg[0], (case.name, chk, n)
        elif kind == "calls":                                # item i has exactly K calls
            assert it["ncalls"][arg[0]] == arg[1], (case.name, chk, int(it["ncalls"][arg[0]]))
        elif kind == "calls_all":                            # the calls per item, all of them
            assert np.array_equal(it["ncalls"], arg[0]), (case.name, kind, np.flatnonzero(it["ncalls"] != arg[0])[:5])
        elif kind == "supports":                             # the supports of item i's calls, in order
            assert it["sup"](arg[0]) == list(arg[1]), (case.name, chk, it["sup"](arg[0]))
        elif kind == "sup_first":                            # an item of at most 8 calls whose first call has L supports
            assert 1 <= it["ncalls"][arg[0]] <= 8 and it["sup"](arg[0])[0] == arg[1], (case.name, chk, it["sup"](arg[0]))
        elif kind == "sup_later":
            assert 2 <= it["ncalls"][arg[0]] <= 8 and arg[1] in it["sup"](arg[0])[1:], (case.name, chk, it["sup"](arg[0]))
        elif kind == "sup_serial":                           # an item of more than 8 calls, one of them with L supports
            assert it["ncalls"][arg[0]] > 8 and arg[1] in it["sup"](arg[0]), (case.name, chk, it["sup"](arg[0]))
        elif kind == "type":
            assert case.segs[it["seg"][arg[0]]]["type"] == arg[1], (case.name, chk)
        elif kind == "tile_mix":                             # one tile of 8 items holds two types / chromosomes / genotyped and not
            tile = arg[1]
            lo, hi = tile * EM_TILE, min(n, (tile + 1) * EM_TILE)
            vals = {"type": [case.segs[k]["type"] for k in it["seg"][lo:hi]], "chrom": [case.segs[k]["chrom"] for k in it["seg"][lo:hi]],
                    "genotype": gt[lo:hi].tolist()}[arg[0]]
            assert len(set(vals)) > 1 and (it["ncalls"][lo:hi] > 0).all(), (case.name, chk, vals)
        elif kind == "big_in_tile":                          # the items of the tile with more than 8 calls sit at exactly these places
            lo = arg[0] * EM_TILE
            assert np.flatnonzero(it["ncalls"][lo:lo + EM_TILE] > 8).tolist() == list(arg[1]), (case.name, chk, it["ncalls"][lo:lo + EM_TILE])
        elif kind == "last_tile":
            assert (n - 1) % EM_TILE + 1 == arg[0], (case.name, chk, n)
        elif kind == "max_calls_ge":
            assert it["ncalls"].max() >= arg[0], (case.name, chk)
        elif kind == "fold":                                 # a tile behind chunk 64 exists: k_emit folds item_chunk[64 ..] for it
            assert ((n - 1) // EM_TILE) // (CHUNK // EM_TILE) > 64, (case.name, chk, n)
        else:
            raise KeyError(kind)
    return len(case.checks)


# ------------------------------------------------------------------------------------------------ small tables: a layout of clusters
class Layout:
    """clusters added in input order (type by type as columns.TYPES, chromosomes ascending); every cluster is one work item, so the value
    add() returns is its item index.  groups: [(signatures, value, sequence deficit)] - DEL / INS: `signatures` reads with length
    `value` at one position (INS: sequences `deficit` shorter than that); DUP: one start, end = start + value; INV: start + the group's
    index, end = start + value; TRA: starts one apart, second position `value`"""

    def __init__(self, name, params, with_reads=False):
        self.name, self.params, self.with_reads = name, params, with_reads
        self.per, self.reads, self.n, self.last = {t: [] for t in TYPES}, [], 0, (0, "")
        self.cur, self.cells, self.checks = {}, set(), []

    def add(self, t, groups, chrom="1", cells=(), checks=()):
        key = (TYPES.index(t), chrom)
        assert key >= self.last, (self.name, t, chrom)
        self.last = key
        base = self.cur.get(key, 10000)
        self.cur[key] = base + 5000 + len(groups)
        sid, k, names = self.n, 0, []
        assert sum(g[0] for g in groups) >= self.params.min_support
        for gi, (cnt, val, short) in enumerate(groups):
            for _ in range(cnt):
                nm = "c%05d_%04d" % (sid, k)
                names.append(nm)
                if t == "DEL":
                    self.per[t].append((base, val, nm, "DEL", chrom))
                elif t == "INS":
                    self.per[t].append((base, val, nm, ("ACGT" * (val // 4 + 1))[:val - short], "INS", chrom))
                elif t == "DUP":
                    self.per[t].append((base, base + val, nm, "DUP", chrom))
                elif t == "INV":
                    self.per[t].append(("++", base + gi, base + val, nm, "INV", chrom))
                else:
                    self.per[t].append(("A", base + k, "2", val, nm, "TRA", chrom))
                k += 1
        if self.with_reads:                                  # every signature's read spans the site, three more support nothing
            for nm in names + ["x%05d_%d" % (sid, j) for j in range(3)]:
                self.reads.append((base - 3000, base + 3000, 1, nm, chrom))
        self.cells |= set(cells)
        self.checks += [(c[0], sid) + tuple(c[1:]) for c in checks]
        self.n += 1
        return sid

    def case(self):
        st = SigStore.from_tuple_lists(self.per, self.reads or None, chroms=["1", "2"])
        return case_from_store(self.name, st, self.params, self.cells, self.checks + [("n_items", self.n)])


def dels(counts, step=1000):
    return [(c, 20000 + step * k, 0) for k, c in enumerate(counts)]


def inss(counts, noseq=()):
    return [(c, 2000 + 100 * k, 1 if k in noseq else 0) for k, c in enumerate(counts)]


def dups(counts):
    return [(c, 60000 + 2000 * k, 0) for k, c in enumerate(counts)]


def invs(counts):
    return [(c, 20000 - 600 * k, 0) for k, c in enumerate(counts)]           # the end falls by more than the bias as the start rises: no chain break


def reads_of(K):
    return [3 + k % 3 for k in range(K)]                    # 3 - 5 reads per allele: ties and the stable by-count order both occur


def by_count(counts, least):
    return sorted(c for c in counts if c >= least)


def table_A(genotype=False):
    """K calls from one cluster for every K of KS (DEL, INS, DUP), 2 and 9 (INV), 1 and 2 (TRA); F: the same, genotyped, with a reads table"""
    fam = "F" if genotype else "A"
    L = Layout(fam, base_params(genotype=genotype), with_reads=genotype)
    for t, mk in (("DEL", dels), ("INS", inss)):
        for K in KS:
            L.add(t, mk(reads_of(K)), cells={(fam, t, K)}, checks=[("calls", K), ("supports", by_count(reads_of(K), 3)), ("type", t)])
    for K in INV_KS:
        L.add("INV", invs(reads_of(K)), cells={(fam, "INV", K)}, checks=[("calls", K), ("supports", reads_of(K)[::-1]), ("type", "INV")])
    for K in KS:
        L.add("DUP", dups(reads_of(K)), cells={(fam, "DUP", K)}, checks=[("calls", K), ("supports", reads_of(K)), ("type", "DUP")])
    L.add("TRA", [(5, 900, 0)], cells={(fam, "TRA", 1)}, checks=[("calls", 1), ("type", "TRA")])
    i = L.add("TRA", [(5, 900, 0), (5, 1200, 0)], cells={(fam, "TRA", 2)}, checks=[("calls", 2), ("supports", [5, 5])])
    L.checks.append(("max_calls_ge", 130))
    if genotype:                                             # the tile of the last DUP items and the TRA items: genotyped next to not genotyped
        L.cells.add(("C", "span", "genotype"))
        L.checks.append(("tile_mix", "genotype", i // EM_TILE))
    return L.case()


NOCALL = [(1, 20000, 0), (1, 30000, 0), (1, 40000, 0)]       # a DEL cluster of three reads, three single-read alleles: a work item without a call


def table_B():
    """groups below the count (no slot), invalid slots and items without a call"""
    L = Layout("B", base_params(max_size=100000))
    L.add("DEL", NOCALL, cells={("B", "nocall", "item0")}, checks=[("calls", 0)])
    for where, counts in (("lowest", (2, 3, 4)), ("middle", (3, 2, 4)), ("highest", (3, 4, 2))):
        L.add("DEL", dels(counts), cells={("B", "below", "DEL", where)}, checks=[("supports", by_count(counts, 3))])
    L.add("DEL", dels((4,)), checks=[("calls", 1)])
    L.add("DEL", NOCALL, cells={("B", "nocall", "between")}, checks=[("calls", 0)])
    L.add("DEL", dels((3, 5)), checks=[("calls", 2)])
    L.add("DEL", dels((3,)), checks=[("calls", 1)])
    assert L.n == EM_TILE
    for _ in range(EM_TILE):                                 # a whole tile without a call
        L.add("DEL", NOCALL, cells={("B", "nocall", "tile")}, checks=[("calls", 0)])
    # INS alleles that pass the count and have no sequence of the wanted length: a slot with valid = 0 at the lowest, a middle and the highest rank
    for where, k in (("lowest", 0), ("middle", 1), ("highest", 2)):
        counts = (3, 4, 5)
        L.add("INS", inss(counts, noseq=(k,)), cells={("B", "invalid", "INS", where)}, checks=[("supports", [c for j, c in enumerate(counts) if j != k])])
    L.add("INS", inss((4,), noseq=(0,)), cells={("B", "nocall", "invalid_slot")}, checks=[("calls", 0)])
    counts = (3, 4, 5, 3, 4, 5, 3, 4, 5, 3, 4, 5)            # twelve slots, nine valid: the serial path over invalid slots (ranks 0, 5, 11)
    L.add("INS", inss(counts, noseq=(0, 4, 11)), cells={("B", "invalid", "INS", "serial")}, checks=[("supports", sorted(c for j, c in enumerate(counts) if j not in (0, 4, 11)))])
    counts = (3, 2, 4, 1, 3, 5, 2, 4, 3, 3, 4, 5, 3)         # thirteen alleles, nine with a slot
    L.add("INS", inss(counts), cells={("B", "below", "INS", "serial")}, checks=[("supports", by_count(counts, 3))])
    # INV: a sub-cluster of two signatures between two that pass
    L.add("INV", invs((3, 2, 4)), cells={("B", "below", "INV", "middle")}, checks=[("supports", [4, 3])])
    # DUP: sub-clusters below read_count (no slot) and slots that fail min_size (the lowest end) / max_size (the highest end)
    for where, counts in (("lowest", (2, 3, 4)), ("middle", (3, 2, 4)), ("highest", (3, 4, 2))):
        L.add("DUP", dups(counts), cells={("B", "below", "DUP", where)}, checks=[("supports", [c for c in counts if c >= 3])])
    L.add("DUP", [(3, 10, 0), (4, 60000, 0), (5, 62000, 0)], cells={("B", "invalid", "DUP", "lowest")}, checks=[("supports", [4, 5])])
    L.add("DUP", [(3, 60000, 0), (4, 62000, 0), (5, 200000, 0)], cells={("B", "invalid", "DUP", "highest")}, checks=[("supports", [3, 4])])
    L.add("DUP", [(3, 10, 0)] + dups(reads_of(9)) + [(4, 200000, 0)], cells={("B", "invalid", "DUP", "serial")}, checks=[("supports", reads_of(9))])
    L.add("TRA", [(5, 900, 0)], checks=[("calls", 1)])
    L.add("TRA", [(1, 900, 0), (1, 1200, 0), (1, 1500, 0)], cells={("B", "nocall", "last")}, checks=[("calls", 0)])
    return L.case()


def table_C(r):
    """tile composition: the item of more than 8 calls first, in the middle and last in its tile, two of them in one tile, neighbours of 1,
    2 and 8 calls; tiles that span a chromosome and a type change; the last tile holds r items"""
    L = Layout("C%d" % r, base_params())
    one = lambda **kw: L.add("DEL", dels((3,)), **kw)
    k2, k8, k9, k16 = dels((3, 4)), dels(reads_of(8)), dels(reads_of(9)), dels(reads_of(16))
    plan = [[k9, k2, k8, None, None, None, None, None], [None, None, None, k16, k2, None, None, None], [None, k2, None, None, None, None, k8, k9],
            [None, k9, None, None, dels(reads_of(65)), None, None, None], [None, k2, k8, None, None, None, None, None]]
    marks = [("first", [0]), ("middle", [3]), ("last", [7]), ("two", [1, 4]), ("none", [])]
    for tile, (row, (label, big)) in enumerate(zip(plan, marks)):
        for g in row:
            if g is None:
                one(checks=[("calls", 1)])
            else:
                L.add("DEL", g, checks=[("supports", by_count([c for c, _, _ in g], 3))])
        L.cells |= {("C", "big_at", label)} | ({("C", "neighbour", 1), ("C", "neighbour", 2), ("C", "neighbour", 8)} if label == "first" else set())
        L.checks.append(("big_in_tile", tile, big))
    for chrom in ("1", "2"):                                 # tile 5: four DEL items of chromosome 1, four of chromosome 2
        for q in range(4):
            L.add("DEL", k9 if (chrom, q) == ("2", 0) else k2, chrom=chrom)
    L.cells.add(("C", "span", "chrom"))
    L.checks.append(("tile_mix", "chrom", 5))
    for q in range(4):                                       # tile 6: DEL of chromosome 2, INS of chromosome 1
        L.add("DEL", dels((4,)), chrom="2")
    for q in range(4):
        L.add("INS", inss(reads_of(9)) if q == 0 else inss((3, 4)))
    L.cells.add(("C", "span", "type"))
    L.checks.append(("tile_mix", "type", 6))
    assert L.n == 7 * EM_TILE
    for q in range(r):                                       # the last tile: r DUP items, the last of them with 9 calls
        L.add("DUP", dups(reads_of(9)) if q == r - 1 else dups((3, 4)), checks=[("calls", 9 if q == r - 1 else 2)])
    L.cells.add(("C", "last_tile", r))
    L.checks.append(("last_tile", r))
    return L.case()


def table_D():
    """support lists of every length of LENGTHS: for an item's first slot (DEL and DUP), a later slot, and a slot of an item of more than 8"""
    L = Layout("D", base_params(min_support=1))
    for n in LENGTHS:
        L.add("DEL", dels((n, n + 1)), cells={("D", "first", n)}, checks=[("sup_first", n), ("supports", [n, n + 1])])
        L.add("DEL", dels((1, n)), cells={("D", "later", n)}, checks=[("sup_later", n)])
        L.add("DEL", dels((1,) * 4 + (n,) + (1,) * 5), cells={("D", "serial", n)}, checks=[("sup_serial", n), ("calls", 10)])
    for n in LENGTHS:
        L.add("DUP", dups((n, n + 1)), cells={("D", "first_dup", n)}, checks=[("sup_first", n), ("supports", [n, n + 1])])
    return L.case()


# ------------------------------------------------------------------------------------------------ large tables: n items, numpy
def _nine():
    out = []
    for k in range(9):
        out += [20000 + 1000 * k] * (2 + k % 2)
    return out


E_SHAPES = {"one2": [20000] * 2, "none": [20000, 30000], "two": [20000] * 2 + [30000] * 3, "one3": [20000] * 3,
            "three": [20000] * 2 + [30000] * 2 + [40000] * 3, "nine": _nine()}
E_CALLS = {"one2": 1, "none": 0, "two": 2, "one3": 1, "three": 3, "nine": 9}
E_CYCLE = ("one2", "one2", "none", "one2", "two", "one2", "one3", "one2", "three", "one2")      # (period 10: not a divisor of the tile)


def table_E(n):
    """n DEL items under read_count 2: mostly two signatures and one call, items of 0, 1, 2 and 3 calls with 2 .. 7 supports along the table, and a
    no-call item and a 9-call item on each side of every seam the table reaches (tile, piece, chunk, second chunk, chunk 65) and at its end"""
    p = base_params(min_support=2)
    names = list(E_SHAPES)
    kind = np.array([names.index(E_CYCLE[i % len(E_CYCLE)]) for i in range(min(n, len(E_CYCLE)))], np.int64)
    kind = np.resize(kind, n)
    special = {}
    for s in E_SEAMS + (n,):
        if s <= n:
            special.update({s - 2: "none", s - 1: "nine", s: "none", s + 1: "nine"})
    special.update({n - 2: "none", n - 1: "nine"})
    special = {i: k for i, k in special.items() if 0 <= i < n}
    for i, k in special.items():
        kind[i] = names.index(k)
    sizes = np.array([len(E_SHAPES[k]) for k in names], np.int64)[kind]
    start = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    a = ch.from_sizes(sizes.tolist(), bias=p.max_cluster_bias_DEL)
    b = np.zeros(len(a), np.int64)
    for q, k in enumerate(names):
        at = start[kind == q]
        if len(at):
            b[(at[:, None] + np.arange(len(E_SHAPES[k]))[None, :]).ravel()] = np.tile(E_SHAPES[k], len(at))
    ncalls = np.array([E_CALLS[k] for k in names], np.int64)[kind]
    checks = [("n_items", n), ("calls_all", ncalls), ("last_tile", (n - 1) % EM_TILE + 1)] + [("calls", i, E_CALLS[k]) for i, k in sorted(special.items())]
    cells = {("E", n)}
    if n > FOLD:
        cells.add(("E", "fold"))
        checks.append(("fold",))
    return EmitCase("E%d" % n, p, [seg_of(p, "DEL", len(a))], a, b, np.zeros(len(a), np.int64), np.arange(len(a)), cells, checks, only32=n > 8193, memo=True)


# ------------------------------------------------------------------------------------------------ publish plans (cell G)
def publish_plans(want):
    """[(cell, keywords of cluster_batch, is the capacity retry taken?)] for a table whose oracle result is `want`: capacities equal to the
    produced counts and one below them, and the slim forms of the result"""
    nc, ns = len(want["bp1"]), len(want["support_sig"])
    assert nc > 1 and ns > 1
    return [(("G", "cap_calls", "equal"), dict(cap_calls=nc, cap_support=ns + 5), False), (("G", "cap_calls", "below"), dict(cap_calls=nc - 1, cap_support=ns + 5), True),
            (("G", "cap_support", "equal"), dict(cap_calls=nc + 5, cap_support=ns), False), (("G", "cap_support", "below"), dict(cap_calls=nc + 5, cap_support=ns - 1), True),
            (("G", "slim", "no_support"), dict(no_support=True), False), (("G", "slim", "coord32"), dict(coord32=True), False),
            (("G", "slim", "fields"), dict(no_support=True, coord32=True, fields=("call_aux", "cipos", "seq_pick")), False),
            (("G", "slim", "support32"), dict(), False)]


# ------------------------------------------------------------------------------------------------ the registry
BUILDERS = {"A": table_A, "B": table_B, "C1": lambda: table_C(1), "C7": lambda: table_C(7), "C8": lambda: table_C(8), "D": table_D,
            "F": lambda: table_A(genotype=True)}
_CASES = {}


def case(name):
    """a table by name ("A" .. "F", "E<n>"), built once"""
    if name not in _CASES:
        _CASES[name] = table_E(int(name[1:])) if name[0] == "E" else BUILDERS[name]()
        ch.assert_order(_CASES[name])
        if name[0] == "E" and int(name[1:]) > 8193:          # (one large table at a time is kept)
            for k in [k for k in _CASES if k[0] == "E" and k != name and int(k[1:]) > 8193]:
                del _CASES[k]
    return _CASES[name]


def required_cells():
    """every cell of the issue's list, written down independently of the builders"""
    need = set()
    for fam in ("A", "F"):
        need |= {(fam, t, K) for t in ("DEL", "INS", "DUP") for K in KS} | {(fam, "INV", K) for K in INV_KS} | {(fam, "TRA", 2)}
    need |= {("B", "below", "DEL", w) for w in ("lowest", "middle", "highest")} | {("B", "nocall", w) for w in ("item0", "last", "between", "tile")}
    need |= {("B", "invalid", "INS", w) for w in ("lowest", "middle", "highest", "serial")} | {("B", "invalid", "DUP", w) for w in ("lowest", "highest")}
    need |= {("C", "big_at", w) for w in ("first", "middle", "last", "two")} | {("C", "neighbour", k) for k in (1, 2, 8)}
    need |= {("C", "last_tile", r) for r in (1, 7, 8)} | {("C", "span", w) for w in ("type", "chrom", "genotype")}
    need |= {("D", w, n) for w in ("first", "later", "serial") for n in LENGTHS}
    need |= {("E", n) for n in E_SIZES} | {("E", "fold")}
    need |= {("G", "cap_calls", w) for w in ("equal", "below")} | {("G", "cap_support", w) for w in ("equal", "below")}
    need |= {("G", "slim", w) for w in ("no_support", "coord32", "fields", "support32")}
    return need


# ------------------------------------------------------------------------------------------------ recorded rows
def input_digest(c):
    h = hashlib.sha256()
    for k in ("a", "b", "rid", "aux"):
        h.update(k.encode())
        h.update(np.ascontiguousarray(getattr(c, k), dtype=np.int64).tobytes())
    for v in (c.reads[1:] if c.reads is not None else ()):
        h.update(np.ascontiguousarray(v, dtype=np.int64).tobytes())
    h.update(repr([(s["type"], s["chrom"], s["n"]) for s in c.segs]).encode())
    return h.hexdigest()


def slim_row(t, row):
    """a row as it is recorded: DUP / TRA read lists sorted (Python set order in the reference), read lists of more than LONG names and
    INS sequences of more than LONG bases as their sha256"""
    from helpers import READS_FIELD, SET_ORDER_TYPES
    row = list(row)
    k = READS_FIELD[t]
    names = row[k].split(",")
    if t in SET_ORDER_TYPES:
        names = sorted(names)
        row[k] = ",".join(names)
    if len(names) > LONG:
        row[k] = "sha256:" + hashlib.sha256(",".join(sorted(names)).encode()).hexdigest()
    if t == "INS" and len(row[13]) > LONG:
        row[13] = "sha256:%d:" % len(row[13]) + hashlib.sha256(row[13].encode()).hexdigest()
    return row
