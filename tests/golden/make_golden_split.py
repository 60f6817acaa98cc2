"""split_sigs.json.gz: the reference's organize_split_signal / analysis_split_read (main script :50-513) driven with
synthetic primary alignments and SA-tag entries (see make_golden_main.py, which imports the main script and calls
split_golden).  split_edges.json.gz: the same functions on CRAFTED reads - one family per rule, one quantity moved across the
rule's threshold - and on small-coordinate random reads, where slices leave [0, L] (split_edges)."""
import gzip
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from cutesv_amd import synth                                  # noqa: E402  (pseudo_sequence: the fixtures store its key, not the bases)

CHROMS = ["1", "10", "2", "X"]                                # (string order != numeric order: analysis_bnd compares names)


def sa_cigar(rng, clip0, span, clip1):
    """a CIGAR text whose leading / trailing clips and reference span are the given numbers; hard clips, insertions and
    skipped regions are thrown in (acquire_clip_pos counts only S clips and M / D / = / X spans)"""
    ops = []
    hard = rng.random() < 0.1
    if clip0:
        ops.append("%d%s" % (clip0, "H" if hard else "S"))
    left = span
    while left > 0:
        k = int(min(left, rng.integers(1, 4000)))
        ops.append("%d%s" % (k, rng.choice(["M", "M", "M", "=", "X", "D"])))
        left -= k
        if left > 0 and rng.random() < 0.3:
            ops.append("%d%s" % (int(rng.integers(1, 50)), rng.choice(["I", "N"])))
    if clip1:
        ops.append("%d%s" % (clip1, "H" if hard else "S"))
    return "".join(ops), (0 if hard else clip0), (0 if hard else clip1)


def random_split_read(rng, name, key, kind):
    """segments that roughly tile the read; `kind` steers how consecutive segments relate on the reference"""
    L = int(rng.integers(800, 20000))
    n = int(rng.choice([1, 2, 2, 2, 3, 3, 3, 4, 5, 6, 9]))
    cuts = np.sort(rng.integers(0, L, size=2 * n))
    segs = []
    chrom = str(rng.choice(CHROMS)); strand = str(rng.choice(["+", "-"])); ref = int(rng.integers(10_000, 5_000_000))
    for k in range(n):
        rs, re = int(cuts[2 * k]), int(cuts[2 * k + 1])
        if rng.random() < 0.35:                               # abutting / overlapping on the read
            rs = max(0, (segs[-1][1] if segs else rs) + int(rng.integers(-40, 120)))
            re = max(rs + 1, re)
        span = max(1, re - rs + int(rng.integers(-30, 30)))
        u = rng.random()
        if kind == "tra" and u < 0.5 or u < 0.12:
            chrom = str(rng.choice(CHROMS)); ref = int(rng.integers(10_000, 5_000_000))
        if kind == "inv" and u < 0.6 or u > 0.9:
            strand = "-" if strand == "+" else "+"
        step = {"del": int(rng.choice([0, 40, 300, 5000, 200000])), "ins": int(rng.integers(-20, 20)), "dup": -int(rng.choice([0, 50, 800, 20000])),
                "inv": int(rng.integers(-3000, 3000)), "tra": int(rng.integers(-100, 100)), "mix": int(rng.integers(-6000, 6000))}[kind]
        fs = max(0, ref + step)
        segs.append([rs, re, fs, fs + span, chrom, strand])
        ref = fs + span
    order = rng.permutation(n)                                # the SA tag lists the other alignments in no particular order
    segs = [segs[i] for i in order]
    mapq = [int(rng.choice([0, 5, 20, 60, 60])) for _ in segs]
    # the first one is the record itself (primary_info when its mapq passes)
    p = segs[0]
    primary = list(p) if mapq[0] >= 20 else []
    sa = ""
    for s, q in zip(segs[1:], mapq[1:]):
        rs, re, fs, fe, ch, st = s
        c0, c1 = (rs, L - re) if st == "+" else (L - re, rs)
        text, _, _ = sa_cigar(rng, c0, fe - fs, c1)
        sa += "%s,%d,%s,%s,%d,%d;" % (ch, fs + 1, st, text, q, int(rng.integers(0, 50)))
    return dict(name=name, primary=primary, sa=sa, qlen=L, key=key)


def ins_inside_tra_read(rng, name, key):
    """first and last segment continue each other on one chromosome, the middle of the read maps elsewhere: the rule at the
    end of analysis_split_read (main script :436-460) that reports the middle as an insertion"""
    L = int(rng.integers(3000, 12000))
    a = int(rng.integers(300, L // 3)); b = int(rng.integers(2 * L // 3, L - 300))
    mid = [(a + int(rng.integers(0, 30)), b - int(rng.integers(0, 30)))]
    if rng.random() < 0.4:                                    # two middle pieces
        m = (mid[0][0] + mid[0][1]) // 2
        mid = [(mid[0][0], m), (m + int(rng.integers(0, 20)), mid[0][1])]
    chrom = str(rng.choice(CHROMS)); other = str(rng.choice([c for c in CHROMS if c != chrom])); strand = str(rng.choice(["+", "-"]))
    ref = int(rng.integers(100_000, 5_000_000))
    gap = int(rng.choice([0, 3, -3, 25, -25, 200, -400, -5000]))
    first = [0, a, ref, ref + a, chrom, strand]
    last = [b, L, ref + a + gap, ref + a + gap + (L - b), chrom, strand]
    if strand == "-":                                         # on the reverse strand the read runs down the reference
        first, last = [0, a, ref + a + gap, ref + a + gap + a, chrom, strand], [b, L, ref - (L - b) + a, ref + a, chrom, strand]
    segs = [first] + [[rs, re, int(rng.integers(10_000, 5_000_000)), 0, other, str(rng.choice(["+", "-"]))] for rs, re in mid] + [last]
    for s in segs[1:-1]:
        s[3] = s[2] + (s[1] - s[0])
    order = rng.permutation(len(segs))
    segs = [segs[i] for i in order]
    mapq = [60] + [int(rng.choice([20, 60, 60, 5])) for _ in segs[1:]]
    sa = ""
    for s, q in zip(segs[1:], mapq[1:]):
        rs, re, fs, fe, ch, st = s
        c0, c1 = (rs, L - re) if st == "+" else (L - re, rs)
        text, _, _ = sa_cigar(rng, c0, fe - fs, c1)
        sa += "%s,%d,%s,%s,%d,%d;" % (ch, fs + 1, st, text, q, 0)
    return dict(name=name, primary=list(segs[0]), sa=sa, qlen=L, key=key)


def split_golden(main):
    cases = []
    for name, seed, n, kind, params in (("deletions", 21, 300, "del", dict(sv=30, max_size=100000, min_mapq=20, parts=7)),
                                        ("insertions", 22, 300, "ins", dict(sv=30, max_size=100000, min_mapq=20, parts=7)),
                                        ("duplications", 23, 300, "dup", dict(sv=30, max_size=100000, min_mapq=20, parts=7)),
                                        ("inversions", 24, 300, "inv", dict(sv=30, max_size=100000, min_mapq=20, parts=7)),
                                        ("translocations", 25, 300, "tra", dict(sv=30, max_size=100000, min_mapq=20, parts=7)),
                                        ("mixture", 26, 600, "mix", dict(sv=30, max_size=100000, min_mapq=20, parts=7)),
                                        ("no_limits", 27, 300, "mix", dict(sv=1, max_size=-1, min_mapq=0, parts=-1)),
                                        ("tight", 28, 300, "del", dict(sv=500, max_size=3000, min_mapq=30, parts=3)),
                                        ("ins_inside_tra", 29, 200, "instra", dict(sv=30, max_size=100000, min_mapq=20, parts=7))):
        rng = np.random.default_rng(seed)
        reads = [(ins_inside_tra_read(rng, "sr%05d" % i, seed * 100000 + i) if kind == "instra" else
                  random_split_read(rng, "sr%05d" % i, seed * 100000 + i, kind)) for i in range(n)]
        cand = {t: [] for t in ("DEL", "INS", "DUP", "INV", "TRA")}
        for r in reads:
            query = synth.pseudo_sequence(r["qlen"], r["key"])
            main.organize_split_signal(list(r["primary"]), r["sa"].split(";")[:-1], r["qlen"], params["sv"], params["min_mapq"], params["parts"],
                                       r["name"], cand, params["max_size"], query)
        cases.append(dict(name=name, params=params, reads=reads, **{t: [list(x) for x in cand[t]] for t in cand}))
    with gzip.open(os.path.join(HERE, "split_sigs.json.gz"), "wt") as f:
        json.dump(cases, f)
    print("split_sigs.json.gz: %d cases; candidates %s" % (len(cases), {t: sum(len(c[t]) for c in cases) for t in ("DEL", "INS", "DUP", "INV", "TRA")}))


# ------------------------------------------------------------------------------------------------ split_edges.json.gz
# Crafted reads: a FAMILY is one base read and one quantity moved over threshold - 1, threshold, threshold + 1 (and over the
# neighbouring residues where the rule divides by 2 or 5); `step` is the offset from the threshold.  Reads are explicit segment
# lists [read_start, read_end, ref_start, ref_end, chr, strand] with coordinates of a few hundred; one segment is the record
# itself (primary_info), the others become SA text "chr,ref_start + 1,strand,<c0>S<span>M<c1>S,mapq,0;".
TYPES5 = ("DEL", "INS", "DUP", "INV", "TRA")
EDGE_CASES = dict(edges=dict(sv=30, max_size=100000, min_mapq=20, parts=7),
                  edges_tight=dict(sv=30, max_size=40, min_mapq=20, parts=3),
                  edges_no_limits=dict(sv=30, max_size=-1, min_mapq=20, parts=-1),
                  edges_sv0=dict(sv=0, max_size=100000, min_mapq=20, parts=7))
SV = 30


def seg(rs, re, fs, fe, ch="1", st="+"):
    return [rs, re, fs, fe, ch, st]


def minus(segs, L):
    """the same alignments seen from a reverse-strand read: read coordinates flipped, order reversed (the analysis flips them back)"""
    return [[L - s[1], L - s[0], s[2], s[3], s[4], "-" if s[5] == "+" else "+"] for s in reversed(segs)]


def sa_entry(s, L, mapq):
    rs, re, fs, fe, ch, st = s
    c0, c1 = (rs, L - re) if st == "+" else (L - re, rs)
    assert c0 >= 0 and c1 >= 0 and fe > fs, s
    return "%s,%d,%s,%s%dM%s,%d,0;" % (ch, fs + 1, st, "%dS" % c0 if c0 else "", fe - fs, "%dS" % c1 if c1 else "", mapq)


class Edges:
    def __init__(self):
        self.reads = {c: [] for c in EDGE_CASES}
        self.n = 0

    def add(self, family, step, segs, L=600, primary=0, mapq=None, case="edges"):
        """primary: the index in `segs` of the record itself (None: the read has no primary_info); mapq: per segment, for the SA text"""
        mapq = mapq or [60] * len(segs)
        sa = "".join(sa_entry(s, L, q) for k, (s, q) in enumerate(zip(segs, mapq)) if k != primary)
        self.reads[case].append(dict(name="e%04d" % self.n, primary=list(segs[primary]) if primary is not None else [], sa=sa, qlen=L, key=770000 + self.n,
                                     family=family, step=step))
        self.n += 1


def edge_families(E):
    # ---- organize_split_signal (:483-513)
    a, b = seg(0, 200, 1000, 1200), seg(250, 550, 1500, 1800)
    for st in (-1, 0):
        E.add("org_mapq", st, [a, b], primary=None, mapq=[60, 20 + st])
    E.add("org_no_primary", 0, [a, b], mapq=[60, 19])                                  # the primary lifts the gate ...
    E.add("org_no_primary", 1, [a, b], primary=None, mapq=[60, 19])                    # ... without one it stays up
    chain = [seg(100 * k, 100 * k + 100, 1000 + 135 * k, 1100 + 135 * k) for k in range(4)]
    E.add("org_parts", 0, chain[:3], case="edges_tight")
    E.add("org_parts", 1, chain, case="edges_tight")
    E.add("org_parts", 2, chain, case="edges_no_limits")                               # (the same four segments with parts == -1)
    E.add("org_n01", 0, [], primary=None)
    E.add("org_n01", 1, [a])
    E.add("org_n01", 2, [a, b])
    A, B, C = seg(100, 300, 1000, 1200), seg(100, 400, 1500, 1800), seg(100, 350, 2000, 2300)
    for k, order in enumerate(([A, B], [B, A])):
        E.add("org_equal_rs2", k, order)
    for k, order in enumerate(([A, B, C], [B, A, C], [C, B, A], [A, C, B])):
        E.add("org_equal_rs3", k, order)
    # ---- analysis_inv on two segments (:50-95)
    for st in (-1, 0):
        E.add("inv2_branch1_sv", st, [seg(0, 200, 1000, 1500), seg(250, 500, 1100, 1500 - (SV + st), st="-")])
        E.add("inv2_branch2_sv", st, [seg(0, 200, 1000, 1500), seg(250, 500, 1100, 1500 + (SV + st), st="-")])
        E.add("inv2_branch3_sv", st, [seg(0, 200, 1000, 1500, st="-"), seg(250, 500, 1000 + (SV + st), 1900)])
        E.add("inv2_branch4_sv", st, [seg(0, 200, 1000, 1500, st="-"), seg(250, 500, 1000 - (SV + st), 1900)])
    for st in (-1, 0, 1):                                                              # ele_2[0] + 0.5 * diff >= ele_1[1], diff even / odd
        E.add("inv2_half_even", st, [seg(0, 200, 1000, 1500), seg(175 + st, 500, 1100, 1450, st="-")])
        E.add("inv2_half_odd", st, [seg(0, 200, 1000, 1500), seg(175 + st, 500, 1100, 1451, st="-")])
        E.add("inv2_half_minus_odd", st, [seg(0, 200, 1000, 1500, st="-"), seg(175 + st, 500, 1049, 1900)])
    # ---- analysis_bnd (:97-188)
    for st in (0, 1):
        E.add("bnd_gap", st, [seg(0, 200, 1000, 1200, "10"), seg(300 + st, 500, 3000, 3200, "2")])
    k = 0
    for s1 in "+-":
        for s2 in "+-":
            for c1, c2 in (("10", "2"), ("2", "10")):
                E.add("bnd_shapes", k, [seg(0, 200, 1000, 1200, c1, s1), seg(250, 500, 3000, 3200, c2, s2)])
                k += 1
    # ---- two segments on one strand (:216-257)
    both = lambda fam, st, segs, L=600, **kw: (E.add(fam, st, segs, L=L, **kw), E.add(fam + "_minus", st, minus(segs, L), L=L, **kw))      # noqa: E731
    for st in (-1, 0):
        both("two_overlap_sv", st, [seg(0, 200, 1000, 1500), seg(300, 600, 1500 - (SV + st), 1900)])
    for st in (-1, 0, 1):
        both("two_ins_or_dup", st, [seg(0, 200, 1000, 1500), seg(300 + st, 600, 1400, 1900)])
    # ---- the INS / DEL pair of rules (sp_indel), on two segments: a2 = [rs2, L) at reference gap g behind a1 = [0, 200)
    pair = lambda rs2, g, L=600: [seg(0, 200, 1000, 1500), seg(rs2, L, 1500 + g, 1900 + g)]      # noqa: E731
    for st in (-1, 0):
        both("indel_ins_delta_sv", st, pair(230 + st, 0))
        both("indel_del_delta_sv", st, pair(200, SV + st))
    for st in range(-2, 5):                                                            # overlap 30 against max(30, delta / 5), delta = 148 .. 154
        E.add("indel_ins_overlap_fifth", st, pair(170 + 150 + st, -30))
        E.add("indel_del_overlap_fifth", st, pair(170 - (150 + st), -30))
    for st in range(-2, 3):                                                            # overlap 31, delta = 153 .. 157 (31 == 155 / 5)
        E.add("indel_ins_overlap_fifth_31", st, pair(169 + 155 + st, -31))
        E.add("indel_del_overlap_fifth_31", st, pair(169 - (155 + st), -31))
    for st in (0, 1):
        E.add("indel_ins_gap_100", st, pair(401, 100 + st))                             # ele_2[2] - ele_1[3] <= max(100, delta / 5), delta ~ 100
        E.add("indel_del_gap_100", st, pair(300 + st, 300))                             # ele_2[0] - ele_1[1] <= max(100, delta / 5), delta ~ 200
    for st in range(-2, 3):                                                            # ... against delta / 5 = 100.6 .. 101.4 at a gap of 101
        E.add("indel_ins_gap_fifth", st, pair(301 + 505 + st, 101, L=1200), L=1200)
        E.add("indel_del_gap_fifth", st, pair(301, 101 + 505 + st))
    for st in (0, 1):
        E.add("indel_ins_max", st, pair(240 + st, 0), case="edges_tight")
        E.add("indel_del_max", st, pair(200, 40 + st), case="edges_tight")
    E.add("indel_ins_max", 2, pair(241, 0), case="edges_no_limits")
    E.add("indel_del_max", 2, pair(200, 41), case="edges_no_limits")
    for st in (-1, 0, 1):
        both("indel_trunc_negative", st, pair(300, -32 + st))                           # int(x / 2) of -33, -32, -31
        both("indel_trunc_positive", st, pair(400, 32 + st))
        E.add("indel_half_position", st, pair(400, 1 + st))                             # (ele_2[2] + ele_1[3]) / 2: x.0 and x.5
    # ---- three segments + - + (:271-292) and - + - (:293-314)
    pmp = lambda a2rs=200, a2fs=1200, a2fe=1210, a3rs=400, a3fs=1210: [seg(0, 200, 1000, 1200), seg(a2rs, 400, a2fs, a2fe, st="-"), seg(a3rs, 600, a3fs, a3fs + 200)]      # noqa: E731
    mpm = lambda a2rs=200, a2fs=1250, a2fe=1295, a3rs=400, a3fe=1290: [seg(0, 200, 1300, 1500, st="-"), seg(a2rs, 400, a2fs, a2fe), seg(a3rs, 600, 1100, a3fe, st="-")]     # noqa: E731
    for st in (-1, 0, 1):
        E.add("tri_pmp_first_even", st, pmp(a2rs=195 + st))
        E.add("tri_pmp_first_odd", st, pmp(a2rs=195 + st, a2fe=1209, a3fs=1209))
        E.add("tri_pmp_second_even", st, pmp(a3rs=395 + st))
        E.add("tri_pmp_second_odd", st, pmp(a3rs=395 + st, a2fe=1209, a3fs=1209))
        E.add("tri_mpm_first_even", st, mpm(a2rs=195 + st))
        E.add("tri_mpm_first_odd", st, mpm(a2rs=195 + st, a3fe=1291))
        E.add("tri_mpm_second_even", st, mpm(a3rs=395 + st))
        E.add("tri_mpm_second_odd", st, mpm(a3rs=395 + st, a3fe=1291))
    for st in (-1, 0):
        E.add("tri_pmp_gate_first", st, pmp(a2fs=1200 + st))
        E.add("tri_pmp_gate_second", st, pmp(a2fe=1210 - st))
        E.add("tri_mpm_gate_first", st, mpm(a2fs=1240 + st))                             # ele_2[2] - ele_3[3] = -50, -51
        E.add("tri_mpm_gate_second", st, mpm(a2fe=1350 - st))                            # ele_1[2] - ele_2[3] = -50, -51
    # ---- the last window's analysis_inv (:316-331)
    ppm = [seg(0, 200, 1000, 1200), seg(200, 400, 1300, 1500), seg(400, 600, 1600, 1900, st="-")]
    E.add("lastwin_choice", 0, ppm, L=800)
    E.add("lastwin_choice", 1, [ppm[0], seg(200, 400, 1300, 1500, st="-"), ppm[2]], L=800)
    E.add("lastwin_fourth", 0, ppm, L=800)
    E.add("lastwin_fourth", 1, ppm + [seg(600, 800, 1800, 2000)], L=800)              # (+ + - +: neither window calls analysis_inv)
    # ---- all on one strand (:333-399)
    for st in (-1, 0):
        both("one_dup_sv", st, [seg(0, 200, 1000, 1200), seg(200, 400, 1300, 1500), seg(400, 600, 1500 - (SV + st), 1800)])
        E.add("one_dup_gate", st, [seg(0, 200, 500, 700), seg(200, 400, 1100 + st, 1300), seg(400, 600, 1000, 1100)])      # ele_2[2] < ele_3[3]
        both("one_gate_third", st, [seg(0, 200, 1000, 1200), seg(200, 400, 1300, 1500), seg(400, 600, 1500 + st, 1800)])      # ele_3[2] >= ele_2[3]
    four = [seg(0, 150, 200, 400), seg(150, 300, 1100, 1300), seg(300, 450, 1000, 1100), seg(450, 600, 1200, 1400)]
    E.add("one_dup_first_window", 0, four)                                             # the second window would qualify for the a == 0 DUP
    E.add("one_dup_first_window", 1, four[1:])
    three = [seg(0, 200, 1000, 1200), seg(200, 400, 1200, 1400), seg(400, 600, 1500, 1700)]
    E.add("one_last_extra", 0, three, L=800)
    E.add("one_last_extra", 1, three + [seg(600, 800, 1650, 1900)], L=800)              # not the last window any more, and its gate fails
    # ---- :401-428
    for st in (-1, 0):
        E.add("route_third_none_plus", st, [seg(0, 200, 3000, 3200, st="-"), seg(200, 400, 1000, 1200), seg(400, 600, 1200 + SV + st, 1500)])
        E.add("route_third_none_minus", st, [seg(0, 200, 1200 + SV + st, 1500), seg(200, 400, 1000, 1200, st="-"), seg(400, 600, 700, 900, st="-")])
        E.add("route_pair_then_other_plus", st, [seg(0, 200, 1000, 1200), seg(200, 400, 1200 + SV + st, 1500), seg(400, 600, 3000, 3300, st="-")])
        E.add("route_pair_then_other_minus", st, minus([seg(200, 400, 1000, 1200), seg(400, 600, 1200 + SV + st, 1500)], 600) + [seg(400, 600, 3000, 3300)])
    # ---- an insertion inside a translocation (:439-464)
    def instra(dis_ref, dis_read=100):
        return [seg(0, 200, 1000, 1200), seg(200, 200 + dis_read, 5000, 5000 + dis_read, "2"),
                seg(200 + dis_read, 400 + dis_read, 1200 + dis_ref, 1400 + dis_ref)], 400 + dis_read
    for st in (-1, 0, 1):
        s, L = instra(SV + st)
        both("instra_ref_distance", st, s, L=L)                                        # abs(dis_ref) < max(SV, .)
        s, L = instra(-SV + st)
        both("instra_ref_distance_negative", st, s, L=L)                               # ... and dis_ref <= -SV: the DUP
    for st in (-2, -1, 0, 1):
        s, L = instra(50 + st, 300)
        E.add("instra_ref_distance_fifth", st, s, L=L)                                 # 48 .. 51 against (300 - dis_ref) / 5
    for st in (-1, 0):
        s, L = instra(0, SV + st)
        E.add("instra_length_sv", st, s, L=L)
    for st in (0, 1):
        s, L = instra(0, 40 + st)
        E.add("instra_length_max", st, s, L=L, case="edges_tight")
    s, L = instra(0, 41)
    E.add("instra_length_max", 2, s, L=L, case="edges_no_limits")
    for k, dr in enumerate((10, -10)):
        s, L = instra(dr)
        E.add("instra_min_side", k, s, L=L)
    s, L = instra(10)
    E.add("instra_ends_differ", 0, s, L=L)
    E.add("instra_ends_differ", 1, s[:2] + [s[2][:4] + ["10", "+"]], L=L)
    E.add("instra_ends_differ", 2, s[:2] + [s[2][:4] + ["1", "-"]], L=L)
    # ---- slices that leave [0, L]: the moved quantity is the read length
    def forms(fam, st, a1, a2, L, physical=True, case="edges"):
        """the pair as a '+' read, as a '-' read (aux bit 0) and - where every segment lies inside the read - again behind / in front
        of a record of the other strand: flag 16 with aux bit 0 clear, flag 0 with it set"""
        p = 0 if 0 <= a1[0] < a1[1] <= L else 1
        E.add(fam + "_plus", st, [a1, a2], L=L, primary=p, case=case)
        E.add(fam + "_minus", st, minus([a1, a2], L), L=L, primary=1 - p, case=case)
        if physical:
            E.add(fam + "_reversed_record", st, [a1, a2, seg(L - 5, L, 3000, 3100, st="-")], L=L, primary=2, case=case)
            E.add(fam + "_forward_record", st, minus([a1, a2], L) + [seg(L - 5, L, 3000, 3100)], L=L, primary=2, case=case)
    for L in (600, 291, 290, 289, 285):                                                # c = -20, d = 290: empty, 19 bases, d == L, d > L
        forms("slice_negative_start", L - 290, seg(0, 10, 1000, 1200), seg(260, L, 1140, 1400), L)
    for L in (600, 360):                                                               # c = -40, d = 350 through the :231 form: empty, 30 bases
        E.add("slice_negative_start_two_segment_rule", L - 390, [seg(0, 10, 1000, 1200), seg(300, L, 1100, 1400)], L=L)
    for L in (400, 419, 420, 421):                                                     # c = 70, d = 420
        forms("slice_end_past_read", L - 420, seg(0, 100, 1000, 1200), seg(390, L, 1140, 1400), L)
    for L in (300, 314, 315, 316):                                                     # c = 315, d = 475: a leading clip longer than the read
        forms("slice_start_past_read", L - 315, seg(200, 290, 1000, 1100), seg(500, L, 1150, 1200), L, physical=False)
    for L in (300, 260, 150, 100):                                                     # c = -150, d = -40: a trailing clip longer than the read
        forms("slice_negative_end", L - 150, seg(0, -200, 1000, 1100), seg(10, L, 1200, 1400), L, physical=False)
    for st in (0, 1):                                                                  # --min_size 0: c == d
        forms("slice_empty", st, seg(0, 200, 1000, 1200), seg(200 + st, 600, 1200, 1500), 600, physical=False, case="edges_sv0")


def small_fuzz_reads(seed, n, first):
    """random reads with L in 150 .. 400 and reference coordinates below 1000: comparisons land on equality and slices leave [0, L]"""
    rng = np.random.default_rng(seed)
    chroms = ["1", "10", "2"]
    reads = []
    for it in range(n):
        L = int(rng.integers(150, 400)); k = int(rng.choice([2, 2, 3, 3, 4, 5]))
        ch = str(rng.choice(chroms)); st = str(rng.choice(["+", "-"])); ref = int(rng.integers(0, 600))
        segs = []
        for _ in range(k):
            rs = int(rng.integers(0, L - 1)); re = int(rng.integers(rs + 1, L + 1))
            if rng.random() < 0.15:
                ch = str(rng.choice(chroms))
            if rng.random() < 0.25:
                st = "-" if st == "+" else "+"
            fs = max(0, ref + int(rng.integers(-120, 160))); fe = fs + int(rng.integers(1, 200))
            segs.append([rs, re, fs, fe, ch, st]); ref = int(rng.choice([fs, fe]))
        mapq = [60] + [int(rng.choice([0, 20, 60, 60])) for _ in segs[1:]]
        primary = 0 if rng.random() < 0.85 else None
        sa = "".join(sa_entry(s, L, q) for j, (s, q) in enumerate(zip(segs, mapq)) if j != primary)
        reads.append(dict(name="f%05d" % (first + it), primary=list(segs[0]) if primary is not None else [], sa=sa, qlen=L, key=880000 + first + it,
                          family="small_fuzz", step=it))
    return reads


def run_reads(main, reads, params):
    """-> per read, the five lists organize_split_signal appended for it"""
    out = []
    for r in reads:
        cand = {t: [] for t in TYPES5}
        main.organize_split_signal(list(r["primary"]), r["sa"].split(";")[:-1], r["qlen"], params["sv"], params["min_mapq"], params["parts"], r["name"], cand,
                                   params["max_size"], synth.pseudo_sequence(r["qlen"], r["key"]))
        out.append({t: [list(x) for x in cand[t]] for t in TYPES5})
    return out


def negative_starts(case):
    """the INS candidates of a case whose slice starts below 0, counted with the package's own CPU restatement (the reference does
    not hand its slice bounds out)"""
    from cutesv_amd import extract
    from oracle import oracle
    p = case["params"]
    rank = {c: i for i, c in enumerate(sorted(CHROMS))}
    enc = extract.encode_split_reads([(r["primary"], r["sa"], r["qlen"]) for r in case["reads"]], rank)
    sig = oracle.split_signatures(enc, sv_size=p["sv"], min_mapq=p["min_mapq"], max_split_parts=p["parts"], max_size=p["max_size"])
    return int(((sig["kind"] == 1) & (sig["c"] < 0)).sum())


def split_edges(main):
    E = Edges()
    edge_families(E)
    cases, by_family = [], {}
    for name, params in EDGE_CASES.items():
        reads = E.reads[name]
        per_read = run_reads(main, reads, params)
        for r, o in zip(reads, per_read):
            by_family.setdefault(r["family"], []).append((r["step"], o))
        cases.append(dict(name=name, params=params, reads=reads, **{t: [x for o in per_read for x in o[t]] for t in TYPES5}))
    # self-checks, on the reference alone: a family whose output never changes between neighbouring steps crosses no threshold
    print("split_edges.json.gz: %d families, %d crafted reads" % (len(by_family), E.n))
    for fam, steps in by_family.items():
        outs = [o for _, o in steps]
        shapes = [tuple(len(o[t]) for t in TYPES5) for o in outs]
        assert any(x != y for x, y in zip(outs, outs[1:])), "family %s: the reference's output does not change across its steps" % fam
        print("  %-34s steps %-24s DEL/INS/DUP/INV/TRA per step: %s" % (fam, [s for s, _ in steps], " ".join("%d%d%d%d%d" % s for s in shapes)))
    crafted = {t: [x for c in cases for x in c[t]] for t in TYPES5}
    assert all(crafted[t] for t in TYPES5), "a kind does not occur"
    assert any(type(x[0]) is float for x in crafted["INS"]) and any(type(x[0]) is int for x in crafted["INS"])
    assert any(x[3] == "" for x in crafted["INS"])
    fuzz_sets = [dict(sv=1, max_size=-1, min_mapq=20, parts=-1), dict(sv=5, max_size=40, min_mapq=20, parts=3), dict(sv=30, max_size=100000, min_mapq=20, parts=7),
                 dict(sv=1, max_size=40, min_mapq=20, parts=7), dict(sv=5, max_size=100000, min_mapq=20, parts=-1), dict(sv=30, max_size=-1, min_mapq=20, parts=3)]
    for k, params in enumerate(fuzz_sets):
        reads = small_fuzz_reads(500 + k, 500, 500 * k)
        per_read = run_reads(main, reads, params)
        cases.append(dict(name="small_fuzz_%d" % k, params=params, reads=reads, **{t: [x for o in per_read for x in o[t]] for t in TYPES5}))
    neg = sum(negative_starts(c) for c in cases if c["name"].startswith("small_fuzz"))
    assert neg >= 5, "small_fuzz: only %d INS rows with a negative slice start" % neg
    path = os.path.join(HERE, "split_edges.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(cases).encode())
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "split_sigs.json.gz"))
    print("split_edges.json.gz: %d cases, %d bytes; small_fuzz INS rows with c < 0: %d (crafted: %d); candidates %s"
          % (len(cases), os.path.getsize(path), neg, sum(negative_starts(c) for c in cases if c["name"].startswith("edges")),
             {t: sum(len(c[t]) for c in cases) for t in TYPES5}))
