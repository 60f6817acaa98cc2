#!/usr/bin/env python3
"""Record tests/golden/cover_edges.json.gz by RUNNING THE REFERENCE's overlap_cover (cuteSV_genotype.py:95-159) on the seam,
tie and edge tables of tests/cover_helpers.py.

    python tests/golden/make_golden_cover.py      # needs the reference checkout make_golden.py names; CPU only

The reference is imported exactly as make_golden.py imports it (same stub `pysam` module).  Nothing of it is copied: the file
holds the tables' rows as integers, the windows of the calls in doubled coordinates and the cover sets the reference returns.
One case per chromosome that has a genotyped call."""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg                                   # noqa: E402  (stubs pysam, imports the reference, puts the repository on the path)
import cover_helpers as ch                                 # noqa: E402

TABLES = ("seam", "tie", "edge")


def cover_cases():
    out = []
    for name in TABLES:
        st, _ = ch.table(name)
        hb, want, brute = ch.expected(name)
        calls = ch.genotyped_calls(ch.PARAMS, hb.segments, want)
        for chrom in sorted(set(c[1] for c in calls)):
            lo, hi = int(st.reads_off[chrom]), int(st.reads_off[chrom + 1])
            cols = [st.r_start[lo:hi].tolist(), st.r_end[lo:hi].tolist(), st.r_primary[lo:hi].tolist(), st.r_id[lo:hi].tolist()]
            wins = [w for c in calls if c[1] == chrom for w in c[2]]
            svs = [(l // 2 if l % 2 == 0 else l / 2, r // 2 if r % 2 == 0 else r / 2) for l, r in wins]
            _, _, cover, _ = mg.R_GT.overlap_cover(svs, list(zip(*cols)))
            out.append(dict(table=name, chrom=st.chroms[chrom], start=cols[0], end=cols[1], primary=cols[2], id=cols[3],
                            windows2=[list(w) for w in wins], cover=[sorted(int(x) for x in cover[i]) for i in range(len(wins))]))
    return out


if __name__ == "__main__":
    cases = cover_cases()
    path = os.path.join(HERE, "cover_edges.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(cases, separators=(",", ":")).encode())
    print("%s: %d cases, %d reads, %d windows, %d bytes" % (path, len(cases), sum(len(c["start"]) for c in cases),
                                                            sum(len(c["windows2"]) for c in cases), os.path.getsize(path)))
