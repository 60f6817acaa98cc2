#!/usr/bin/env python3
"""Golden vectors of the reference's TASK CUT (main_ctrl, main script :1015-1045) and of load_bed on its float task lists, produced by
running the reference here.

    python tests/golden/make_golden_index_cut.py        # needs /root/reference (read-only mount)  ->  index_cut.json.gz

The main script is imported as make_golden_main.py imports it.  `pysam.AlignmentFile` is a stub that offers get_index_statistics /
get_reference_length over the case's numbers; `load_bed` in the module is replaced by a function that records Task_list, writes the
case's BED from it (regions that start exactly on floor(t0) and ceil(t0) and one that ends on ceil(t0) of fractional bounds, after
the reference's padding), calls the real load_bed, records its lists and leaves main_ctrl with a private exception.  Nothing of the
reference is copied: the file holds the numbers we chose and the lists its functions returned.

Per case: name, stats [[contig, mapped, unmapped, total]], lengths {contig: bases}, batch, threads, tasks [[contig, t0, t1]] (ints and
floats as the reference made them), bed {contig: [[start, end]]} as written (unpadded), regions [[[b0, b1], ...] per task].
"""
import gzip
import json
import math
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_main import load_main      # noqa: E402


class _Left(Exception):
    pass


def sliver_lengths(parts, lo, n_want=2):
    """lengths L >= lo for which the running sum of L / parts, taken `parts` times, stays below L: the reference appends a sliver task"""
    found, L = [], lo
    while len(found) < n_want and L < lo + 100_000:           # (some part counts - 3, 5, 6 - never leave one: the search is bounded)
        bs, pos = L / parts, 0
        if int(L / bs) == parts:
            for _ in range(parts):
                pos += bs
            if pos < L:
                found.append(L)
        L += 1
    assert len(found) == n_want, "no sliver length for %d parts" % parts
    return found


def run_case(main, case, tmp):
    stats, lengths = case["stats"], case["lengths"]
    seen = {}

    class AlignmentFile:
        def __init__(self, *a, **k):
            pass

        def get_index_statistics(self):
            return [tuple(s) for s in stats]

        def get_reference_length(self, name):
            return lengths[name]
    sys.modules["pysam"].AlignmentFile = AlignmentFile
    real = seen["real"] = getattr(main, "_real_load_bed", None) or main.load_bed
    main._real_load_bed = real

    def recording(bed_file, task_list):
        seen["tasks"] = [list(t) for t in task_list]
        bed = {}
        frac = [(t[0], x) for t in task_list for x in t[1:] if x != int(x)]
        for c, x in frac[:6] + frac[-2:]:
            f, ce = math.floor(x), math.ceil(x)
            bed.setdefault(c, []).extend([[f + 1000, f + 2000], [ce + 1000, ce + 2500], [ce - 2000, ce - 1000]])      # padded: [f, f + 3000) [ce, ce + 3500) [ce - 3000, ce)
        for k, t in enumerate(task_list[:: max(1, len(task_list) // 5)]):                                            # and plain ones, here and there
            mid = int((t[1] + t[2]) / 2)
            bed.setdefault(t[0], []).append([mid + 37 * k, mid + 37 * k + 400])
        bed.setdefault("not_in_the_header", []).append([100, 200])
        seen["bed"] = bed
        with open(bed_file, "w") as fh:
            for c, iv in bed.items():
                for s, e in iv:
                    fh.write("%s\t%d\t%d\n" % (c, s, e))
        seen["regions"] = [[list(r) for r in lst] for lst in real(bed_file, task_list)]
        raise _Left()
    main.load_bed = recording
    ref = os.path.join(tmp, "ref.fa")
    open(ref, "w").close()
    args = types.SimpleNamespace(work_dir=tmp, Ivcf=None, reference=ref, input="x.bam", threads=case["threads"], batches=case["batch"],
                                 include_bed=os.path.join(tmp, "case.bed"))
    try:
        main.main_ctrl(args, [])
    except _Left:
        pass
    else:
        raise AssertionError("main_ctrl did not reach load_bed")
    case.update(tasks=seen["tasks"], bed=seen["bed"], regions=seen["regions"])
    return case


def cases():
    def case(name, contigs, batch, threads):
        return dict(name=name, stats=[[c, m, u, m + u] for c, _, m, u in contigs], lengths={c: ln for c, ln, _, _ in contigs}, batch=batch, threads=threads)
    out = [case("no_mapped_read", [("a", 25_000_000, 0, 3), ("b", 9_999_999, 0, 0), ("c", 10_000_000, 0, 0)], 10_000_000, 16),
           case("every_contig_under_the_unit", [("c%d" % k, 3_000_000 + 1_234_567 * k, 100, 1) for k in range(10)], 2_000_000, 1)]
    sl11, sl7 = sliver_lengths(11, 10_000_001), sliver_lengths(7, 50_000_001)
    for threads in (1, 16, 64):
        unit = 10 * (k := 7)                                  # total = unit * threads * 10 reads: the unit is a whole number
        total = unit * threads * 10
        heavy = [("exactly_the_unit", 30_000_000, unit, 2), ("one_more", 30_000_000, unit + 1, 0), ("shorter_than_batch", 1_000_000, 5, 0),
                 ("thirds", 10_000_000, 2 * unit + k, 4), ("sevenths", 10_000_000, 6 * unit + 3, 0), ("divides", 12_000_000, 3 * unit + 1, 0),
                 ("sliver11", sl11[0], 10 * unit + 1, 0), ("sliver7", sl7[0], 6 * unit + 5, 1), ("sliver11b", sl11[1], 10 * unit + 9, 0)]
        # (with one thread the whole file holds ten units: the contigs are taken in this order while they fit, the threshold pair and a sliver first)
        order = ("exactly_the_unit", "one_more", "shorter_than_batch", "sliver7", "thirds", "sliver11", "sevenths", "divides", "sliver11b")
        contigs, left = [], total
        for name in order:
            c = next(h for h in heavy if h[0] == name)
            if c[2] < left:
                contigs.append(c); left -= c[2]
        contigs.append(("the_rest", 40_000_000, left, 0))
        assert sum(c[2] for c in contigs) == total and total / threads / 10 == unit and contigs[0][2] == unit and contigs[1][2] == unit + 1
        out.append(case("threads_%d" % threads, contigs, 10_000_000, threads))
    out.append(case("small_batch", [("x", 1_000_003, 5000, 0), ("y", 77_777, 20, 0), ("z", 999_983, 4000, 9)], 100_000, 16))
    return out


def main_():
    main = load_main()
    done = []
    with tempfile.TemporaryDirectory() as tmp:
        for c in cases():
            done.append(run_case(main, c, tmp))
    slivers = [(c["name"], t) for c in done for t in c["tasks"] if 0 < t[2] - t[1] < 1]
    assert slivers, "no case yields a sliver tail task"
    frac = sum(1 for c in done for t in c["tasks"] if t[1] != int(t[1]))
    assert frac > 10
    with gzip.GzipFile(os.path.join(HERE, "index_cut.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(done).encode())
    print("index_cut.json.gz: %d cases, %d tasks, %d fractional starts, slivers: %s" % (len(done), sum(len(c["tasks"]) for c in done), frac, slivers[:4]))


if __name__ == "__main__":
    main_()
