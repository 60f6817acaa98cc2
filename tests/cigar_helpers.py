"""Crafted CIGARs for the per-read scan (cigar.hip.h), shared by the generator of tests/golden/cigar_edges.json.gz and by
tests/test_cigar_edges.py: the families (one base read, ONE quantity moved across a rule's threshold), the dense random reads,
the counters that say what a set of reads covers, and the lane sweep (k single-base M operations in front of a read).

Nothing here knows the rules' outcome: the families only place pieces; what the reference made of them is in the fixture."""
import json
import zlib

import numpy as np

M, I, D, N, S, H, P, EQ, X = range(9)
PARAM_SETS = dict(default=dict(min_siglength=10, mi=100, md=0), small=dict(min_siglength=4, mi=8, md=8), mid=dict(min_siglength=10, mi=30, md=40))
DENSE_SETS = (dict(min_siglength=3, mi=4, md=4), dict(min_siglength=4, mi=8, md=8), dict(min_siglength=3, mi=0, md=8))
DENSE_COUNTS = (1, 2, 3, 10, 63, 64, 65, 66, 127, 128, 129, 130, 200)
GAP_KINDS = ("M", "EQX", "smallD", "N", "bigD")
SEAM_PAIRS = ((62, 63), (63, 64), (64, 65), (127, 128))          # adjacent pieces: distance 0 (INS) / 0 behind the end (DEL)
SEAM_FIRST = (61, 62, 63, 126, 127)                             # first piece's index when one gap operation lies between the two
FAMILY_KINDS = ("len", "ins_gap", "ins_chain", "ins_below", "del_first", "del_merged", "del_after_cut", "shift", "seam")
MERGE_FAMILIES = ("ins_gap", "ins_chain", "ins_below", "del_first", "del_merged", "del_after_cut", "seam")
HOST_PARAMS = dict(min_mapq=20, min_read_len=50)
SIG_KEYS = ("ins_read", "ins_pos", "ins_len", "ins_piece0", "ins_npiece", "piece_qoff", "piece_len", "del_read", "del_pos", "del_len")


def _ops(*parts):
    return [[int(op), int(ln)] for op, ln in parts if ln > 0]


def gap(kind, g, ms):
    """operations that advance the reference by g"""
    if kind == "M":
        return _ops((M, g))
    if kind == "EQX":
        return _ops((EQ, g // 2), (X, g - g // 2))
    if kind == "N":
        return _ops((N, g))
    if kind == "smallD":                                      # a D below min_siglength: no piece, but it moves the position
        d = min(ms - 1, g)
        return _ops((M, g - d), (D, d))
    if kind == "bigD":                                        # a DEL PIECE between two INS pieces
        assert g >= ms
        return _ops((D, ms), (M, g - ms))
    raise ValueError(kind)


def query_len_of(cigar):
    """as make_golden_cigar.random_read: every operation but D counts (a superset of the query), + 8"""
    return sum(ln for op, ln in cigar if op != D) + 8


class Builder:
    def __init__(self, set_name, key_base):
        self.set_name, self.reads, self.key = set_name, [], key_base

    def add(self, family, step, cigar, seq_len=None, flag=0, mapq=60, start=1000, same_seq=False):
        """same_seq: the steps of the family cut their slices out of ONE sequence, so that two strings differ only when the slices do"""
        if not (same_seq and self.reads and self.reads[-1]["family"] == family):
            self.key += 1
        self.reads.append(dict(name="%s/%s/%s" % (self.set_name, family, step), family=family, step=str(step), flag=flag, mapq=mapq, start=start,
                               cigar=[list(x) for x in cigar], seq_len=query_len_of(cigar) if seq_len is None else seq_len, seq_key=self.key))


def around(t):
    return [x for x in (t - 1, t, t + 1) if x >= 0]


def merge_pairs(ms, mi, md):
    """the deciding pair of every merge family, as (tag, head operations, lambda g: the pair's operations with the distance g that
    decides, the threshold g is moved around - None where every distance is beyond it)"""
    p = ms + 2
    out = [("ins", [], lambda g: _ops((I, p), (M, g), (I, p + 1)), mi),
           ("del_first", [], lambda g: _ops((D, p), (M, g), (D, p + 1)), md),
           ("del_merged", _ops((D, p), (M, md), (D, p)), lambda g: _ops((M, g), (D, p + 1)), md)]
    if md - ms >= 0:                                          # after a cut the distance is g + Lb, Lb >= min_siglength
        out.append(("del_after_cut", _ops((D, p), (M, md + 50)), lambda g: _ops((D, ms), (M, g - ms), (D, p + 1)), md))
    else:                                                     # every distance is beyond md: only the instance g <= md < g + Lb exists
        out.append(("del_after_cut", _ops((D, p), (M, md + 50)), lambda g: _ops((D, ms), (M, g - ms), (D, p + 1)), None))
    return out


def families(set_name, params, key_base):
    """the crafted reads of one parameter set"""
    ms, mi, md = params["min_siglength"], params["mi"], params["md"]
    p = ms + 2
    b = Builder(set_name, key_base)
    m20 = [[M, 20]]
    for ln in (ms - 1, ms, ms + 1):
        b.add("len", ln, m20 + _ops((I, ln)) + m20 + _ops((D, ln)) + m20)
    for kind in GAP_KINDS:
        for g in around(mi):
            if kind == "bigD" and g < ms:
                continue
            b.add("ins_gap_" + kind, g, m20 + _ops((I, p)) + gap(kind, g, ms) + _ops((I, p + 1)) + m20)
    for g2 in (mi, mi + 1):
        b.add("ins_chain", "%d_%d" % (mi, g2), m20 + _ops((I, p), (M, mi), (I, p + 1), (M, g2), (I, p + 2)) + m20)
    for g in around(mi):
        if g >= 2:
            b.add("ins_below", g, m20 + _ops((I, p), (M, g // 2), (I, ms - 1), (M, g - g // 2), (I, p + 1)) + m20)
    for g in around(md):
        b.add("del_first", g, m20 + _ops((D, p), (M, g), (D, p + 1)) + m20)
        b.add("del_merged", g, m20 + _ops((D, p), (M, md), (D, p), (M, g), (D, p + 1)) + m20)
    # D a, a cut, D b (length lb), gap g, D c: the reference measures c from b's START; then a fourth piece, from the END of c again
    cut = md + 50
    if md - ms >= 1:
        for lb, g in ((ms, md - 1 - ms), (ms, md - ms), (ms, md + 1 - ms), (md, 0), (md + 1, 0)):
            b.add("del_after_cut", "lb%d_g%d" % (lb, g), m20 + _ops((D, p), (M, cut), (D, lb), (M, g), (D, p + 1)) + m20)
        for g4 in (md, md + 1):
            b.add("del_after_cut_fourth", g4, m20 + _ops((D, p), (M, cut), (D, ms), (M, md - ms), (D, p + 1), (M, g4), (D, p + 2)) + m20)
    else:
        for g in (0, 1):
            b.add("del_after_cut", "lb%d_g%d" % (ms, g), m20 + _ops((D, p), (M, cut), (D, ms), (M, g), (D, p + 1)) + m20)
    # the shift counter of the INS slice
    for tag, head in (("none", []), ("H", [[H, 7]]), ("S", [[S, 7]])):
        b.add("shift_lead", tag, head + m20 + _ops((I, p)) + m20, same_seq=True)
    for tag, mid in (("none", []), ("N", [[N, 5]]), ("P", [[P, 3]]), ("NP", [[N, 5], [P, 3]])):
        b.add("shift_skip", tag, m20 + mid + _ops((I, p)) + m20, same_seq=True)
    for tag, tail in (("none", []), ("S", [[S, 9]]), ("H", [[H, 9]])):
        b.add("shift_tail", tag, m20 + _ops((I, p)) + m20 + tail, same_seq=True)
    for ql in (20 + p + 28, 20 + p, 20 + p - 1, 20 + 1, 20, 5):   # the slice [20, 20 + p) against the query's end: whole ... empty
        b.add("shift_cut", ql, m20 + _ops((I, p)) + m20, seq_len=ql)
    for ql in (20 + p + 5 + p + 1, 20 + p + 5 + 3, 20 + p + 5, 20 + p - 2):  # two merged pieces, the query ends inside the 2nd / between / in the 1st
        if mi >= 5:
            b.add("shift_cut2", ql, m20 + _ops((I, p), (M, 5), (I, p + 1)) + m20, seq_len=ql)
    # the seams of the 64-operation step: k single-base M operations put the pair's pieces on chosen operation indices
    ones = lambda k: [[M, 1]] * k                                                 # noqa: E731
    for tag, head, pair, t in merge_pairs(ms, mi, md):
        for g in ([t, t + 1] if t is not None else [ms, ms + 1]):
            ops = head + pair(g)
            # index (in head + pair) of the two pieces that decide
            pieces = [k for k, (op, ln) in enumerate(ops) if op in (I, D) and ln >= ms]
            i0, i1 = pieces[-2], pieces[-1]
            for first in SEAM_FIRST:
                if first - i0 >= 0:
                    b.add("seam_%s" % tag, "g%d_at%d_%d" % (g, first, first + i1 - i0), ones(first - i0) + ops + [[M, 5]])
    for a, c in SEAM_PAIRS:                                  # adjacent pieces, nothing between them
        b.add("seam_adjacent_ins", "%d_%d" % (a, c), ones(a) + _ops((I, p), (I, p + 1)) + [[M, 5]])
        b.add("seam_adjacent_del", "%d_%d" % (a, c), ones(a) + _ops((D, p), (D, p + 1)) + [[M, 5]])
        b.add("seam_adjacent_del_cut", "%d_%d" % (a, c), ones(a - 2) + _ops((D, p), (M, md + 50), (D, ms), (D, p + 1)) + [[M, 5]])
    # the carried state crosses a whole step without a piece: a gap of 100+ single-base operations
    for g in (mi, mi + 1):
        fill = ones(g) + [[P, 1]] * max(0, 100 - g) if g <= 130 else ones(100) + [[M, g - 100]]
        b.add("seam_empty_step_ins", g, ones(3) + _ops((I, p)) + fill + _ops((I, p + 1)) + [[M, 5]])
    for g in (md, md + 1):
        fill = ones(g) + [[P, 1]] * max(0, 100 - g)
        b.add("seam_empty_step_del", g, ones(3) + _ops((D, p)) + fill + _ops((D, p + 1)) + [[M, 5]])
        if md >= ms:
            b.add("seam_empty_step_del_cut", g, ones(3) + _ops((D, p), (M, md + 50), (D, ms)) + ones(g - ms) + [[P, 1]] * max(0, 100 - (g - ms)) + _ops((D, p + 1)) + [[M, 5]])
    return b.reads


def host_family(set_name, params, key_base):
    """the gates that are the caller's (extract.parse_reads): mapq, query length, flags"""
    ms = params["min_siglength"]
    b = Builder(set_name, key_base)
    cig = [[M, 30]] + _ops((I, ms + 2)) + [[M, 30]] + _ops((D, ms + 3)) + [[M, 30]]
    for mq in (HOST_PARAMS["min_mapq"] - 1, HOST_PARAMS["min_mapq"]):
        b.add("host_mapq", mq, cig, mapq=mq)
    for ql in (HOST_PARAMS["min_read_len"] - 1, HOST_PARAMS["min_read_len"]):
        b.add("host_qlen", ql, [[M, 10]] + _ops((I, ms + 2)) + [[M, 10]] + _ops((D, ms + 3)) + [[M, 10]], seq_len=ql)
    for flag in (0, 16, 256, 2048, 2064):
        b.add("host_flag", flag, cig, flag=flag)
    return b.reads


def kind_of(family):
    for k in sorted(FAMILY_KINDS + ("host",), key=len, reverse=True):
        if family.startswith(k):
            return k
    raise KeyError(family)


# ------------------------------------------------------------------------------------------------ what a family must show
def expectations(params):
    """{family: what the reference's output must do across the family's steps} - the exact set of families of a parameter set.
    "change": the decision shape (`outcome`) differs between two neighbouring steps; "pair": a seam family - per distance g the shape
    is the same on every placement, and the two distances differ; "slice": the shape stays, the INS strings (cut out of one sequence)
    do not; "same": the shape stays (positions and bases may move); "fixed": the shape and the strings stay - stated, not left to chance.  A sub-family a parameter set cannot have is absent:
    del_after_cut_fourth and seam_empty_step_del_cut need md >= min_siglength (+ 1), the default set's md is 0."""
    ms, mi, md = params["min_siglength"], params["mi"], params["md"]
    e = {f: "change" for f in ("len", "ins_chain", "ins_below", "del_first", "del_merged", "shift_cut", "seam_empty_step_ins", "seam_empty_step_del")}
    e.update({"ins_gap_" + k: "change" for k in GAP_KINDS if k != "bigD" or mi >= ms})
    e.update(shift_lead="slice", shift_skip="slice", shift_tail="fixed")
    if mi >= 5:
        e["shift_cut2"] = "change"
    e.update(seam_ins="pair", seam_del_first="pair", seam_del_merged="pair", seam_adjacent_ins="same", seam_adjacent_del="same", seam_adjacent_del_cut="same")
    if md - ms >= 1:
        e.update(del_after_cut="change", del_after_cut_fourth="change")
    else:                                                     # every distance after a cut is beyond md: g = 0 and 1 both stay apart
        e["del_after_cut"] = "same"
    e["seam_del_after_cut"] = "pair" if md - ms >= 0 else "same"
    if md >= ms:
        e["seam_empty_step_del_cut"] = "change"
    return e


HOST_EXPECTATIONS = dict(host_mapq="change", host_qlen="change", host_flag="same")


def outcome(ins, dele):
    """the decision shape of a read's rows, free of names, positions and bases: (length, length of the recorded string) per INS row,
    the length per DEL row"""
    return tuple((x[1], len(x[3])) for x in ins), tuple(x[1] for x in dele)


def check_families(reads, per_read, expect):
    """reads with their recorded rows per read [(INS rows, DEL rows)] against `expect` (see expectations): AssertionError when a family
    is missing, is not expected, or does not do across its steps what it is there to show"""
    by = {}
    for r, (ins, dele) in zip(reads, per_read):
        by.setdefault(r["family"], []).append((r["step"], outcome(ins, dele), [x[3] for x in ins]))
    assert set(by) == set(expect), "families %s are missing, %s are not expected" % (sorted(set(expect) - set(by)), sorted(set(by) - set(expect)))
    for fam, steps in by.items():
        what, shapes = expect[fam], [o for _, o, _ in steps]
        assert len(steps) >= 2, "family %s has a single step" % fam
        if what == "change":
            assert any(x != y for x, y in zip(shapes, shapes[1:])), "family %s: the reference's output does not change across its steps" % fam
        elif what == "pair":
            per_g = {}
            for step, o, _ in steps:
                per_g.setdefault(step.split("_at")[0], set()).add(o)
            assert len(per_g) == 2 and all(len(v) == 1 for v in per_g.values()), "family %s: the output depends on where the pair lies" % fam
            a, b = per_g.values()
            assert a != b, "family %s: the reference's output does not change between its two distances" % fam
        else:
            assert len(set(shapes)) == 1, "family %s: the decision shape changes across its steps" % fam
            strings = {tuple(x) for _, _, x in steps}
            assert what == "same" or (len(strings) > 1) == (what == "slice"), "family %s: the INS strings %s across its steps" % (fam, "do not change" if what == "slice" else "change")


def rows_per_read(reads, ins, dele):
    """the recorded lists of a case -> [(INS rows, DEL rows)] per read (read names are unique)"""
    rows = {r["name"]: ([], []) for r in reads}
    for x in ins:
        rows[x[2]][0].append(x)
    for x in dele:
        rows[x[2]][1].append(x)
    return [rows[r["name"]] for r in reads]


# ------------------------------------------------------------------------------------------------ dense random reads
def dense_reads(seed, n, tag="d"):
    """n reads of the dense distribution: operation lengths 1..6, counts from DENSE_COUNTS, codes 0..8 with about a quarter each of
    M, I and D.  numpy's legacy generator: its stream is frozen, the fixture stores the seed and a checksum of what it made."""
    rng = np.random.RandomState(seed)
    table = np.array([M, I, D, M, I, D, M, I, D, N, S, H, P, EQ, X, M, I, D, M, I, D, M, I, D], np.int64)    # 6/24 each of M I D, 1/24 the others
    reads = []
    for i in range(n):
        k = int(DENSE_COUNTS[rng.randint(0, len(DENSE_COUNTS))])
        ops = table[rng.randint(0, len(table), k)]
        lens = rng.randint(1, 7, k)
        cigar = [[int(o), int(ln)] for o, ln in zip(ops, lens)]
        ql = query_len_of(cigar)
        if rng.randint(0, 10) == 0:                          # one in ten: the query ends early, slices are cut or empty
            ql = max(1, ql - int(rng.randint(8, 40)))
        reads.append(dict(name="%s%05d" % (tag, i), flag=0, mapq=60, start=int(rng.randint(0, 1000000)), cigar=cigar, seq_len=ql, seq_key=seed * 100000 + i))
    return reads


def long_reads(seed, counts=(4095, 4096, 4097, 8193)):
    rng = np.random.RandomState(seed)
    out = []
    for j, k in enumerate(counts):
        ops = rng.randint(0, 3, k)
        lens = rng.randint(1, 7, k)
        cigar = [[int(o), int(ln)] for o, ln in zip(ops, lens)]
        out.append(dict(name="L%d" % k, flag=0, mapq=60, start=int(rng.randint(0, 1000000)), cigar=cigar, seq_len=query_len_of(cigar), seq_key=seed * 100000 + 90000 + j))
    return out


def reads_checksum(reads):
    h = 0
    for r in reads:
        h = zlib.crc32(json.dumps([r["name"], r["start"], r["seq_len"], r["seq_key"], r["cigar"]], separators=(",", ":")).encode(), h)
    return h


def expand_case(case):
    """a fixture case -> the same case with its reads present (a dense case stores the seed of its reads, not the reads)"""
    if "dense" in case and "reads" not in case:
        case = dict(case, reads=dense_reads(case["dense"]["seed"], case["dense"]["n"]))
        assert reads_checksum(case["reads"]) == case["dense"]["checksum"], "the random stream is not the one the fixture was recorded with"
    return case


def per_read_digests(reads, ins, dele):
    """8 hex digits per read over its INS and DEL rows (the dense cases record these and a digest of the whole lists: the rows of
    3 x 3 000 dense reads would be megabytes)"""
    rows = {r["name"]: ([], []) for r in reads}
    for x in ins:
        rows[x[2]][0].append(list(x))
    for x in dele:
        rows[x[2]][1].append(list(x))
    return "".join("%08x" % zlib.crc32(json.dumps(rows[r["name"]], separators=(",", ":")).encode()) for r in reads)


# ------------------------------------------------------------------------------------------------ what a set of reads covers
def counters(reads, params):
    """how often the reads sit ON a decision of the scan.  A plain walk of the pieces of every read, for COUNTING only."""
    ms, mi, md = params["min_siglength"], params["mi"], params["md"]
    c = dict(piece_eq=0, piece_below=0, ins_eq=0, ins_plus1=0, del_eq=0, del_plus1=0, merge_after_cut=0, start_end_differ=0, merge_across_step=0)
    for r in reads:
        pos = r["start"]
        ins_last = del_last = None                            # (distance anchor, operation index, opened after a cut, end of the piece)
        for k, (op, ln) in enumerate(r["cigar"]):
            if op in (I, D):
                c["piece_eq"] += ln == ms
                c["piece_below"] += ln == ms - 1
            if op == I and ln >= ms:
                if ins_last is not None:
                    d = pos - ins_last[0]
                    c["ins_eq"] += d == mi; c["ins_plus1"] += d == mi + 1
                    merged = d <= mi
                    c["merge_across_step"] += merged and k // 64 != ins_last[1] // 64
                    c["merge_after_cut"] += merged and ins_last[2]
                    ins_last = (pos, k, not merged, pos)
                else:
                    ins_last = (pos, k, False, pos)
            elif op == D and ln >= ms:
                if del_last is not None:
                    d = pos - del_last[0]
                    c["del_eq"] += d == md; c["del_plus1"] += d == md + 1
                    merged = d <= md
                    c["merge_across_step"] += merged and k // 64 != del_last[1] // 64
                    c["merge_after_cut"] += merged and del_last[2]
                    c["start_end_differ"] += del_last[2] and merged != (pos - del_last[3] <= md)
                    del_last = (pos + ln, k, False, pos + ln) if merged else (pos, k, True, pos + ln)
                else:
                    del_last = (pos + ln, k, False, pos + ln)
            if op in (M, D, N, EQ, X):
                pos += ln
    return {k: int(v) for k, v in c.items()}


# ------------------------------------------------------------------------------------------------ the lane sweep
def prefixed(read, k):
    """k single-base M operations in front of the read's CIGAR: every piece moves k operations, k reference bases and k query bases on.
    A leading H stops being the first operation (its negative shift would go), so the sweep leaves such reads out."""
    assert not read["cigar"] or read["cigar"][0][0] != H
    return dict(read, name="%s+%d" % (read["name"], k), cigar=[[M, 1]] * k + read["cigar"], seq_len=read["seq_len"] + k)


def shifted(sig, n_reads, k_of_read):
    """the scan's arrays of the unprefixed reads -> what the prefixed reads must give: positions + k, piece offsets + k"""
    out = {key: np.array(sig[key]).copy() for key in SIG_KEYS}
    k = np.asarray(k_of_read, np.int64)
    out["ins_pos"] += k[out["ins_read"]]
    out["del_pos"] += k[out["del_read"]]
    piece_read = np.repeat(out["ins_read"], out["ins_npiece"])
    out["piece_qoff"] = (out["piece_qoff"] + k[piece_read]).astype(out["piece_qoff"].dtype)
    return out


def batch_arrays(reads):
    """(cig_off, cigar, ref_start) of a list of read dicts"""
    lens = np.fromiter((len(r["cigar"]) for r in reads), np.int64, len(reads))
    off = np.zeros(len(reads) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    flat = np.fromiter(((ln << 4) | op for r in reads for op, ln in r["cigar"]), np.uint32, int(off[-1]))
    return off, flat, np.array([r["start"] for r in reads], np.int64)


def sweep_batch(base_reads, ks=range(131)):
    """every base read behind k single-base M operations, for every k, base-major, as ONE batch
    -> (cig_off, cigar, ref_start, index of the base read per read, k per read)"""
    assert all(not r["cigar"] or r["cigar"][0][0] != H for r in base_reads)
    parts, lens, start, which, kk = [], [], [], [], []
    for j, r in enumerate(base_reads):
        own = np.array([(ln << 4) | op for op, ln in r["cigar"]], np.uint32)
        for k in ks:
            parts += [np.full(k, (1 << 4) | M, np.uint32), own]
            lens.append(k + len(own)); start.append(r["start"]); which.append(j); kk.append(k)
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return off, np.concatenate(parts), np.array(start, np.int64), np.array(which), np.array(kk, np.int64)


def tile_sig(sig, which, n_base):
    """the arrays of the base reads, repeated as the sweep batch orders its reads (read j of the sweep = base read which[j])"""
    ins_by = [np.flatnonzero(sig["ins_read"] == j) for j in range(n_base)]
    del_by = [np.flatnonzero(sig["del_read"] == j) for j in range(n_base)]
    out = {k: [] for k in SIG_KEYS}
    n_piece = 0
    for new, j in enumerate(which.tolist()):
        for i in ins_by[j].tolist():
            p0, npc = int(sig["ins_piece0"][i]), int(sig["ins_npiece"][i])
            out["ins_read"].append(new); out["ins_pos"].append(sig["ins_pos"][i]); out["ins_len"].append(sig["ins_len"][i])
            out["ins_piece0"].append(n_piece); out["ins_npiece"].append(npc)
            out["piece_qoff"] += sig["piece_qoff"][p0:p0 + npc].tolist(); out["piece_len"] += sig["piece_len"][p0:p0 + npc].tolist()
            n_piece += npc
        for i in del_by[j].tolist():
            out["del_read"].append(new); out["del_pos"].append(sig["del_pos"][i]); out["del_len"].append(sig["del_len"][i])
    return {k: np.asarray(v, np.asarray(sig[k]).dtype) for k, v in out.items()}


def assert_sig_equal(got, want, where=""):
    for k in SIG_KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and np.array_equal(g, w), (where, k, len(g), len(w))
