"""--include_bed: "only call where these regions are" (cuteSV main script :1045, :715-723; load_bed, cuteSV_genotype.py:704-726;
DESIGN.md section 19).

    regions = load_bed("panel.bed")
    regions.for_task("chr20", 10_000_000, 20_000_000)        # the (k, 2) list single_pipe_bam / task_to_pool take as bed_regions

The reference pads every region by 1000 bases on both sides, sorts a chromosome's regions by (start, end) and hands a task
[chrom, t0, t1] the regions with `t0 <= b0 < t1 or b0 <= t0 < b1`, in that order.  A record passes when it starts in the task and
some region OF THAT LIST has `end > b0 and start < b1`.  So a read that starts in task k and reaches only a region that begins
at or after task k's end is dropped: with a BED the calls depend on the cut (call_bam's `batch`).  That is the reference's
behaviour and it is kept.  Regions are not merged (a zero-span record on the seam of two touching regions lies in neither) and
may overlap, nest, start below 0 or end past the contig."""
import os

import numpy as np

_SKIP = ("#", "track", "browser")


class Regions:
    """the padded regions of a BED per chromosome: {chrom: int64 (n, 2) array sorted by (start, end)}"""

    def __init__(self, by_chrom):
        self.by_chrom = by_chrom

    @classmethod
    def from_intervals(cls, intervals, pad=1000):
        """{chrom: [(start, end), ...]} as the BED has them -> Regions (each padded to (start - pad, end + pad))"""
        by_chrom = {}
        for chrom, iv in intervals.items():
            a = np.asarray(sorted((int(s) - pad, int(e) + pad) for s, e in iv), np.int64).reshape(-1, 2)
            by_chrom[chrom] = a
        return cls(by_chrom)

    def for_task(self, chrom, t0, t1):
        """the regions of task [chrom, t0, t1), in order: `t0 <= b0 < t1 or b0 <= t0 < b1` (load_bed :719-724) -> int64 (k, 2), k may
        be 0 - also for a chromosome the BED does not name: with a BED a task without regions passes no read.  t0 / t1 may be the
        fractional bounds of call.cut_tasks_index: the comparison is Python's of an int with a float (exact below 2^53, where every
        coordinate lies), as the reference applies it to its float task list"""
        t0, t1 = (float(t) if isinstance(t, float) else int(t) for t in (t0, t1))
        a = self.by_chrom.get(chrom)
        if a is None or len(a) == 0:
            return np.zeros((0, 2), np.int64)
        b0, b1 = a[:, 0], a[:, 1]
        return a[((t0 <= b0) & (b0 < t1)) | ((b0 <= t0) & (t0 < b1))]

    def __len__(self):
        return sum(len(a) for a in self.by_chrom.values())


def load_bed(path, pad=1000):
    """a BED file -> Regions.  Fields are split on tabs, as in the reference; blank lines and lines that start with '#', 'track'
    or 'browser' are skipped; any other line with fewer than three fields or a coordinate that is no integer raises ValueError
    naming file and line (the reference dies with an IndexError there)."""
    intervals = {}
    with open(os.fspath(path)) as f:
        for ln, line in enumerate(f, 1):
            s = line.strip()
            if not s or s.startswith(_SKIP):
                continue
            fields = s.split("\t")
            if len(fields) < 3:
                raise ValueError("%s:%d: a BED line needs three tab-separated fields (chrom, start, end), found %d" % (path, ln, len(fields)))
            try:
                beg, end = int(fields[1]), int(fields[2])
            except ValueError:
                raise ValueError("%s:%d: start / end are not integers: %r, %r" % (path, ln, fields[1], fields[2])) from None
            intervals.setdefault(fields[0], []).append((beg, end))
    return Regions.from_intervals(intervals, pad=pad)
