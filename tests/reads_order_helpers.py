"""Helpers of tests/test_reads_order_seams.py: reads tables laid out in FILE order (runs that the reads-order stage has to find,
order and move), an exact restatement of the verdict k_reads_runs + k_reads_plan reach on such a table, and a stab query that
trusts the order it is given - what the genotype kernels would answer on a table the stage packed wrongly.

A layout is, per chromosome, a list of runs in file order; a run is a start-sorted array of starts.  Every run that asks for one
gets a probe: a DEL call (cover_helpers.Table.call) whose window [L, L + 2 BIAS] begins AT one of the run's own starts and is
covered by rows of that run alone, 3 + (run index mod 5) of them where the run has that many rows at or below L.  A run that
the stage misplaces therefore changes the DR of a call."""
import dataclasses
import functools

import numpy as np

import cover_helpers as ch

TILE, TCAP, CAP = ch.RO_TILE, ch.RO_TCAP, ch.RO_CAP     # rows per tile, run starts a tile may hold, runs + chromosomes of a plan
GA_TAB, RP_THREADS, SPAN = 512, 1024, 512               # runs k_reads_gather keeps in LDS, threads of the plan, rows per gather wavefront
LIMIT = 1 << 32                                         # the plan's run records hold starts in 32 bits
REORDER, IDENTITY, GENERAL = 0, 1, 2                    # ro_state, as the counters line prints it
READ_LEN, GAP = 300, 5000


# ------------------------------------------------------------------------------------------------ layouts
@dataclasses.dataclass
class Run:
    starts: np.ndarray
    length: np.ndarray
    probe: bool
    anchor: int            # row of the run whose start is the probe's L (None: the last row - rows of a later run that land inside this one lie below it)


def run(starts, length=READ_LEN, probe=True, anchor=None):
    starts = np.atleast_1d(np.asarray(starts, np.int64))
    assert len(starts) and (np.diff(starts) >= 0).all(), "a run is start-sorted"
    return Run(starts, np.broadcast_to(np.asarray(length, np.int64), starts.shape).copy(), probe, anchor)


@dataclasses.dataclass
class Layout:
    store: object          # reads table in file order
    sorted: object         # the same rows as Table.store() leaves them: every block in stable start order
    gap: int
    runs: list             # (chromosome, first row, end row (exclusive), probe index or -1) in file order
    probes: list           # (chromosome, call position, run index)

    @property
    def n_runs(self):
        return len(self.runs)

    @functools.cached_property
    def covers(self):
        """the true covering set of every probe: cover_ids, which looks at every row of the chromosome"""
        return [ch.cover_ids(self.store, c, L2, R2) for c, L2, R2 in probe_windows(self)]


def layout(blocks, gap=GAP, names=None):
    """blocks: per chromosome the list of its runs in file order (an empty list: a chromosome without reads) -> Layout"""
    names = names or ["c%05d" % k for k in range(len(blocks))]
    T = ch.Table(names)
    cols = [[], [], []]                                   # start, end, id in file order
    off, runs, probes, row, want = [0], [], [], 0, []
    for c, blk in enumerate(blocks):
        for r in blk:
            s, e = r.starts, r.starts + r.length
            k = -1
            if r.probe:
                j = len(s) - 1 if r.anchor is None else r.anchor
                L = int(s[j])
                R = L + 2 * ch.BIAS
                cand = np.flatnonzero(s <= L)              # rows of the run that may cover: the last `depth` of them do
                depth = min(3 + len(runs) % 5, len(cand))
                e = e.copy()
                e[cand[:-depth]] = np.minimum(e[cand[:-depth]], R - 1)
                e[cand[-depth:]] = np.maximum(e[cand[-depth:]], R + 50)
                k = len(probes)
                probes.append((c, L + ch.BIAS, len(runs)))
                want.append(depth)
            ids = T.reads(names[c], s, e)
            for i, x in enumerate((s, e, ids)):
                cols[i].append(x)
            runs.append((c, row, row + len(s), k))
            row += len(s)
        off.append(row)
    for c, pos, _ in probes:
        T.call(names[c], pos)
    st = T.store()
    s, e, i = [np.concatenate(x) if x else np.zeros(0, np.int64) for x in cols]
    i = np.where(i < 0, T.n_support + (-1 - i), i)
    assert np.array_equal(st.reads_off, off)
    filed = dataclasses.replace(st, r_start=s, r_end=e, r_primary=np.ones(len(s), np.uint8), r_id=i.astype(np.int32))
    lay = Layout(filed, st, int(gap), runs, probes)
    # every probe: covered by rows of its own run only, as many as asked; no two calls of a chromosome close enough to chain
    for (c, pos, r), d in zip(probes, want):
        got = ch.cover_ids(filed, c, 2 * (pos - ch.BIAS), 2 * (pos + ch.BIAS))
        own = filed.r_id[runs[r][1]:runs[r][2]]
        assert len(got) == d and np.isin(got, own).all(), ("probe of run %d" % r, len(got), d)
    by = sorted((c, pos) for c, pos, _ in probes)
    assert all(a[0] != b[0] or b[1] - a[1] >= 1000 for a, b in zip(by, by[1:])), "probes of one chromosome closer than 1000"
    return lay


def probe_windows(lay):
    """[(chromosome, L2, R2)] of the probes, in doubled coordinates"""
    return [(c, 2 * (pos - ch.BIAS), 2 * (pos + ch.BIAS)) for c, pos, _ in lay.probes]


# ------------------------------------------------------------------------------------------------ the stage's verdict
def plan_model(store, gap):
    """What k_reads_runs + k_reads_plan decide about a table -> dict(n_found = run starts the tiles list, n_runs = runs the plan
    orders (None where it gives up before it has counted them), state = ro_state, mode = 1, or 2 after the host's fallback, why).

    A row starts a run when its start is smaller than its predecessor's or more than `gap` above it; a block start is the
    plan's own business and never listed.  The plan holds `CAP` entries: one per chromosome (empty ones included) beside the
    listed starts, and one more.  A tile lists at most TCAP starts.  Every start the plan looks at - a listed row and the row
    before it, the first row of a block and the row before it, the table's last row - must fit 32 bits.  The runs of a
    chromosome, ordered by (first start, position), must not interleave: the last start of one is at most the first of the next,
    and on equality the earlier one in the file comes first, as in a stable sort.  A table whose runs all stay is left as it is."""
    s, off = np.asarray(store.r_start, np.int64), np.asarray(store.reads_off, np.int64)
    n, nc = len(s), len(off) - 1
    cut = np.zeros(n, bool)
    d = s[1:] - s[:-1]
    cut[1:] = (d < 0) | (d > gap)
    cut[off[:-1][off[:-1] < n]] = False
    at = np.flatnonzero(cut)
    n_found = len(at)

    def verdict(state, why, n_runs=None):
        return dict(n_found=n_found, n_runs=n_runs, state=state, mode=2 if state == GENERAL else 1, why=why)

    def outside(v):
        return bool(((v < 0) | (v >= LIMIT)).any())

    if nc + 1 > CAP:
        return verdict(GENERAL, "more chromosomes than the plan holds")
    if n_found + nc > CAP:
        return verdict(GENERAL, "more run starts and chromosomes than the plan holds")
    if n_found and np.bincount(at // TILE).max() > TCAP:
        return verdict(GENERAL, "more than %d run starts in a tile" % TCAP)
    if outside(s[-1:]):
        return verdict(GENERAL, "the last start outside [0, 2^32)")
    if outside(s[at]) or outside(s[at - 1]):
        return verdict(GENERAL, "a run boundary outside [0, 2^32)")
    blocks = np.flatnonzero(off[1:] > off[:-1])
    first = off[blocks]
    n_runs = n_found + len(blocks)
    if outside(s[first]) or outside(s[first[first > 0] - 1]):
        return verdict(GENERAL, "a block boundary outside [0, 2^32)", n_runs)
    beg = np.sort(np.concatenate([at, first]))
    end = np.r_[beg[1:], n]                                # (exclusive: a run ends where the next one of the file begins)
    chrom = np.searchsorted(off, beg, side="right") - 1
    order = np.lexsort((beg, s[beg], chrom))
    a, b = order[:-1], order[1:]
    same = chrom[a] == chrom[b]
    last, nxt = s[end[a] - 1], s[beg[b]]
    if (same & ((last > nxt) | ((last == nxt) & (a > b)))).any():
        return verdict(GENERAL, "runs of a chromosome interleave", n_runs)
    if np.array_equal(order, np.arange(len(beg))):
        return verdict(IDENTITY, "no run moves", n_runs)
    return verdict(REORDER, "", n_runs)


# ------------------------------------------------------------------------------------------------ a query that trusts the order
def stab_sorted(start, end, primary, ids, lo, hi, L2, R2):
    """distinct ids of the primary rows a stab query finds in rows [lo, hi) when it takes them for start-sorted: a binary search
    for the last row with 2 start <= L2, then every row below it with 2 end >= R2"""
    top = lo + int(np.searchsorted(start[lo:hi], L2 // 2, side="right"))      # (2 start <= L2 <=> start <= floor(L2 / 2))
    m = (primary[lo:top] == 1) & (end[lo:top] >= -(-R2 // 2))                 # (2 end >= R2 <=> end >= ceil(R2 / 2))
    return np.unique(ids[lo:top][m])


class Packing:
    """a reads table as a sequence of slices of the file-order rows (what moving whole runs produces)"""

    def __init__(self, lay, slices):
        st = lay.store
        self.slices = [(int(a), int(b)) for a, b in slices if b > a]
        assert sum(b - a for a, b in self.slices) == st.n_reads
        self.start, self.end, self.ids = [np.concatenate([col[a:b] for a, b in self.slices]) for col in (st.r_start, st.r_end, st.r_id)]
        self.primary = np.ones(st.n_reads, np.uint8)
        self.off = st.reads_off

    def cover(self, c, L2, R2):
        return stab_sorted(self.start, self.end, self.primary, self.ids, int(self.off[c]), int(self.off[c + 1]), L2, R2)


def sorted_runs(lay):
    """the runs of the layout in (chromosome, first start, file position) order -> run indices"""
    st = lay.store
    return sorted(range(lay.n_runs), key=lambda r: (lay.runs[r][0], int(st.r_start[lay.runs[r][1]]), lay.runs[r][1]))


def runs_are_disjoint(lay):
    """moving whole runs gives the stable (chromosome, start) order of the rows"""
    st = lay.store
    p = Packing(lay, [lay.runs[r][1:3] for r in sorted_runs(lay)])
    chrom = np.repeat(np.arange(len(st.reads_off) - 1), np.diff(st.reads_off))
    o = np.lexsort((np.arange(st.n_reads), st.r_start, chrom))
    return np.array_equal(p.start, st.r_start[o]) and np.array_equal(p.ids, st.r_id[o])


def _split(slices, at):
    """cut a slice list at packed row `at` -> (head, tail)"""
    head, tail, done = [], [], 0
    for a, b in slices:
        k = min(max(at - done, 0), b - a)
        head.append((a, a + k)); tail.append((a + k, b))
        done += b - a
    return head, tail


def mutants(lay, sample=64, seed=20):
    """wrongly packed tables of a layout whose runs are disjoint -> [(what, run indices to look at first, Packing)]: the table
    left as it is; one run left at its file position while the rest is ordered; two runs that are neighbours in the right
    order, swapped.  Every run that carries a probe when there are at most `sample`, else `sample` drawn ones and the first and
    last of the file (a run without a probe lies on a chromosome nobody looks at, or is one shuffled row)."""
    order = sorted_runs(lay)
    sl = lambda rs: [lay.runs[r][1:3] for r in rs]
    picks = [r for r in range(lay.n_runs) if lay.runs[r][3] >= 0]
    if len(picks) > sample:
        rng = np.random.default_rng(seed)
        picks = sorted(set(rng.choice(picks, sample, replace=False).tolist()) | {picks[0], picks[-1]})
    out = []
    if order != list(range(lay.n_runs)):
        out.append(("as is", [], Packing(lay, [(0, lay.store.n_reads)])))
    where = {r: q for q, r in enumerate(order)}
    for r in picks:
        q = where[r]
        dest = sum(lay.runs[x][2] - lay.runs[x][1] for x in order[:q])
        if dest != lay.runs[r][1]:
            head, tail = _split(sl(order[:q] + order[q + 1:]), lay.runs[r][1])
            out.append(("run %d stays" % r, [r], Packing(lay, head + sl([r]) + tail)))
        if q + 1 < len(order) and lay.runs[order[q + 1]][0] == lay.runs[r][0]:
            out.append(("runs %d and %d swapped" % (r, order[q + 1]), [r, order[q + 1]], Packing(lay, sl(order[:q] + [order[q + 1], r] + order[q + 2:]))))
    return out


def seen(lay, packing, first=()):
    """does a probe's covering set on `packing` differ from the true one (cover_ids)?  `first`: runs whose probes are tried first"""
    wins = probe_windows(lay)
    idx = [lay.runs[r][3] for r in first if lay.runs[r][3] >= 0]
    chroms = set(lay.runs[r][0] for r in first)
    idx += [k for k in range(len(wins)) if k not in idx and (not chroms or wins[k][0] in chroms)]
    for k in idx:
        c, L2, R2 = wins[k]
        if not np.array_equal(packing.cover(c, L2, R2), lay.covers[k]):
            return True
    return False


# ------------------------------------------------------------------------------------------------ builders
def spaced(n, base=10_000, step=10):
    return base + step * np.arange(n, dtype=np.int64)


def descending_pieces(n, cuts, base=10_000, step=10, big=100_000, ranks=None):
    """n evenly spaced rows cut at the rows `cuts` into pieces that lie in the file in DESCENDING order of their coordinates
    (piece j of k begins big * (k - 1 - j) above the base; `ranks`: another order): every cut is a descent, or a jump of more
    than the gap, and every piece has to move"""
    edges = [0] + sorted(cuts) + [n]
    assert len(set(edges)) == len(edges) and step * max(b - a for a, b in zip(edges, edges[1:])) + 2 * READ_LEN + GAP < big
    k = len(edges) - 1
    ranks = list(range(k - 1, -1, -1)) if ranks is None else ranks
    assert sorted(ranks) == list(range(k)) and all(ranks[j + 1] != ranks[j] + 1 for j in range(k - 1))
    return [run(spaced(b - a, base + big * ranks[j], step)) for j, (a, b) in enumerate(zip(edges, edges[1:]))]


def small_block(c, n):
    """a chromosome of n reads without a probe (cases with thousands of blocks)"""
    return [run(1000 + 1000 * np.arange(n), probe=False)] if n else []


def two_out_of_order(base=10_000):
    """a chromosome of two runs that have to change places, a probe in each"""
    return [run(spaced(40, base + 50_000)), run(spaced(30, base))]


SLICE_8 = (0, 7, 8, 15, 64, 200, 448, 511)        # run starts inside a 512-row slice: lane 0, rows 8k + 7 and 8k, the slice's last row


def tile_case(kind, k):
    """one chromosome of 3 tiles whose tile 1 lists exactly k (32 or 33) run starts -> (blocks, facts)"""
    n = 3 * TILE
    if kind == "slices":
        cuts = [TILE + SPAN * w + o for w in range(4) for o in SLICE_8] + ([TILE + 2 * SPAN + 100] if k == 33 else [])
        return [descending_pieces(n, cuts)], dict(tile1=k)
    # k one-row runs in descending order at the end of tile 1 (8 per lane); the table's main run resumes on row 0 of tile 2
    head, tail = 2 * TILE - k, TILE
    ones = [run(5_000_000 - 2000 * j) for j in range(k)]
    return [[run(spaced(head, 200_000))] + ones + [run(spaced(tail, 10_000))]], dict(tile1=k)


def cut_rows_case(n):
    """a table of n rows with a moved run starting on row 0 of tile 1, on the first row of every other wavefront slice of tile 0,
    on a row 8k and a row 8k + 7, and on the table's last row"""
    cuts = [512, 1024, 1536, TILE, TILE + 16, TILE + 23, n - 1]
    return [descending_pieces(n, cuts)], dict(cuts=cuts)


def gap_case(seam):
    """regions A and B glued in the file with a seam of `seam` bases, and behind them region C, which belongs in between"""
    a = spaced(3000, 10_000)
    b = spaced(2000, int(a[-1]) + seam)
    c = spaced(200, int(a[-1]) + 1000)
    return [[run(a), run(b), run(c)]], dict(seam=seam)


def capacity_case(total, empties):
    """n_found + n_chrom == total: 4 000 chromosomes (`empties` of them empty, spread evenly) of 1 to 3 reads and one of four tiles in
    total - 4 000 + 1 pieces"""
    nc = 4000
    k = total - nc
    blocks = []
    for c in range(nc - 1):
        empty = empties and c % (nc // empties) == 5 and c // (nc // empties) < empties
        blocks.append([] if empty else small_block(c, 1 + c % 3))
    blocks.insert(2000, descending_pieces(4 * TILE, [80 * (j + 1) for j in range(k)]))
    return blocks, dict(total=total, n_chrom=nc, empties=empties)


def sorted_chroms_case(nc):
    """a start-sorted table of nc chromosomes; probes on the first, one in the middle and the last"""
    blocks = [small_block(c, 1 + c % 3) for c in range(nc)]
    for c in (0, nc // 2, nc - 1):
        blocks[c] = [run(spaced(40, 10_000))]
    return blocks, dict(n_chrom=nc)


def gather_case(n_runs):
    """one chromosome of 20 tiles in n_runs pieces of 64 rows (the last one longer): 32 run starts in every tile they reach"""
    return [descending_pieces(20 * TILE, [64 * (j + 1) for j in range(n_runs - 1)])], dict(runs=n_runs)


def span_case(first):
    """six runs of `first`, 1, 200, 1, 150 and 2 000 rows in the right order, reversed in the file.  first == 512: the span
    [512, 1024) receives exactly the five others; first == 700: it also receives the end of the first, which straddles row 512"""
    sizes = [first, 1, 200, 1, 150, 2000]
    runs, base = [], 10_000
    for k in sizes:
        runs.append(run(spaced(k, base)))
        base += 10 * k + 2000
    return [runs[::-1]], dict(sizes=sizes)


def blocks_case(nc):
    """nc chromosomes of 0 to 3 reads (every tenth one empty); the last and the middle one hold two runs out of order (for nc
    = 2 500: the chromosomes 1 030 and 2 400)"""
    blocks = [small_block(c, 0 if c % 10 == 0 else 1 + c % 3) for c in range(nc)]
    special = (1030, 2400) if nc == 2500 else (nc // 2 + 1, nc - 1)
    for c in special:
        blocks[c] = two_out_of_order()
    return blocks, dict(n_chrom=nc, special=special)


def tie_case(kind):
    """runs that meet in one start.  Beside the chromosome of the tie lies one whose two runs simply change places."""
    far = run(spaced(30, 900_000))
    if kind == "equal_first_ok":        # A and B begin at 50 000, A lies first in the file and also ends first
        a = run([50_000] * 3)
        b = run(np.r_[50_000, 51_000 + 50 * np.arange(20)], length=np.r_[150, [READ_LEN] * 20], anchor=12)
        t = [a, far, b]
    elif kind == "equal_first_bad":     # A = [50 000, 54 000] and behind it B = [50 000]: B belongs between A's rows
        t = [run([50_000, 54_000], anchor=1), run([50_000], length=150, probe=False)]
    elif kind == "last_is_first_ok":    # A ends at 52 000, where B begins; A lies first in the file
        t = [run(spaced(21, 50_000, 100), anchor=8), far, run(spaced(30, 52_000, 100), anchor=20)]
    else:                               # ... and with A behind B: a stable sort puts B's 52 000 first
        assert kind == "last_is_first_bad"
        t = [run(spaced(30, 52_000, 100), anchor=20), run(spaced(21, 50_000, 100), anchor=8)]
    return [t, two_out_of_order()], dict(kind=kind)


def interleave_case():
    """two runs of one chromosome whose start ranges overlap, beside a chromosome that is fine"""
    x = run(spaced(400, 10_000), anchor=50)                 # 10 000 .. 13 990, probe at its low end
    y = run(spaced(400, 12_005), anchor=390)                # 12 005 .. 15 995, probe at its high end
    return [[y, x], two_out_of_order()], dict()


def limit_case(kind):
    """starts around 2^32 on one chromosome of a table with int64 columns.  "cut_below" / "cut_at": a listed run start of 2^32 - 1
    / 2^32 (one row, moved in front of nothing: two runs below it change places); "last": a start-sorted last chromosome that
    climbs past 2^32 in steps below the gap, so that the table's last start is the only one the plan sees beyond the limit"""
    if kind == "last":
        return [two_out_of_order(), [run(spaced(600, LIMIT - 3000 * 400, 3000), anchor=100)]], dict(kind=kind)
    top = LIMIT - 1 if kind == "cut_below" else LIMIT
    hi = [run(spaced(40, LIMIT - 400_000)), run(spaced(30, LIMIT - 800_000)), run([top])]
    return [hi, two_out_of_order()], dict(kind=kind, top=top)


def identity_case():
    """a start-sorted chromosome that the gap cuts into 41 pieces, and a second one"""
    return [[run(np.concatenate([spaced(100, 10_000 + 50_000 * j) for j in range(41)]), anchor=2050)], [run(spaced(50))]], dict(pieces=41)


def shuffled_case(nc, seed=5):
    """every block in random order (one row per run), nc chromosomes; three of them hold two probed runs among the shuffled rows.
    Up to a few hundred chromosomes they have 20 reads each, beyond that one"""
    rng = np.random.default_rng(seed)
    per = 20 if nc <= 1000 else 1
    blocks = []
    for c in range(nc):
        if c in (0, nc // 2, nc - 1):
            noise = [run(500_000 + 1000 * int(v), probe=False) for v in rng.permutation(40)]
            blocks.append(noise[:20] + two_out_of_order() + noise[20:])
        else:
            blocks.append([run(1000 + 1000 * int(v), probe=False) for v in rng.permutation(per)])
    return blocks, dict(n_chrom=nc)


LONG_TILES = 8193
LONG_N = LONG_TILES * TILE + 5


def long_case():
    """8 193 full tiles and a tail of five rows: a plan thread owns nine tiles.  Evenly spaced starts in seven pieces, six of them
    moved; the cuts lie in the NINTH tile of the threads 0, 499 and 909, in the tail tile and in two ordinary ones"""
    cuts = [8 * TILE + 100, 3000 * TILE + 7, (9 * 499 + 8) * TILE + 1000, 6000 * TILE, (9 * 909 + 8) * TILE + 2047, LONG_TILES * TILE + 2]
    return [descending_pieces(LONG_N, cuts, big=70_000_000, ranks=[1, 0, 3, 2, 5, 4, 6])], dict(cuts=cuts)


CASES = {}
for _kind in ("ones", "slices"):
    for _k in (32, 33):
        CASES["tile_%s_%d" % (_kind, _k)] = functools.partial(tile_case, _kind, _k)
for _n in (2 * TILE + 1, 2 * TILE + 5, 2 * TILE):
    CASES["cut_rows_%d" % _n] = functools.partial(cut_rows_case, _n)
CASES["gap_exact"] = functools.partial(gap_case, GAP)
CASES["gap_plus_1"] = functools.partial(gap_case, GAP + 1)
for _t in (CAP, CAP + 1):
    for _e in (0, 100):
        CASES["capacity_%d_empty_%d" % (_t, _e)] = functools.partial(capacity_case, _t, _e)
for _n in (CAP - 1, CAP):
    CASES["sorted_chroms_%d" % _n] = functools.partial(sorted_chroms_case, _n)
for _n in (GA_TAB, GA_TAB + 1):
    CASES["gather_%d" % _n] = functools.partial(gather_case, _n)
CASES["span_five_runs"] = functools.partial(span_case, 512)
CASES["span_straddle"] = functools.partial(span_case, 700)
for _n in (RP_THREADS - 1, RP_THREADS, RP_THREADS + 1, 2500):
    CASES["blocks_%d" % _n] = functools.partial(blocks_case, _n)
for _kind in ("equal_first_ok", "equal_first_bad", "last_is_first_ok", "last_is_first_bad"):
    CASES["tie_" + _kind] = functools.partial(tie_case, _kind)
CASES["interleave"] = interleave_case
for _kind in ("cut_below", "cut_at", "last"):
    CASES["limit_" + _kind] = functools.partial(limit_case, _kind)
CASES["identity"] = identity_case
for _n in (256, 257, 65536, 65537):
    CASES["shuffled_%d" % _n] = functools.partial(shuffled_case, _n)
SMALL = tuple(CASES)
CASES["long"] = long_case

# what the stage must say about each case: (ro_state, mode)
EXPECT = {name: (REORDER, 1) for name in CASES}
for _name in ("tile_ones_33", "tile_slices_33", "gap_exact", "capacity_%d_empty_0" % (CAP + 1), "capacity_%d_empty_100" % (CAP + 1), "sorted_chroms_%d" % CAP,
              "tie_equal_first_bad", "tie_last_is_first_bad", "interleave", "limit_cut_at", "limit_last", "shuffled_256", "shuffled_257", "shuffled_65536", "shuffled_65537"):
    EXPECT[_name] = (GENERAL, 2)
for _name in ("sorted_chroms_%d" % (CAP - 1), "identity"):
    EXPECT[_name] = (IDENTITY, 1)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (Layout, facts the geometry test asserts)"""
    blocks, facts = CASES[name]()
    return layout(blocks), facts


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> (the C oracle's trimmed result on the start-sorted store, brute_dr of it): the two yardsticks, computed once"""
    from oracle import oracle
    lay, _ = case(name)
    st = lay.sorted
    hb = st.host_batch(st.tasks(), ch.PARAMS)
    want = oracle.cluster_batch(hb, per_sig=True).trimmed()
    return want, ch.brute_dr(st, ch.PARAMS, hb.segments, want)
