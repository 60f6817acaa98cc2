#!/usr/bin/env python3
"""Record tests/golden/tra_edges.json.gz by RUNNING THE REFERENCE's call_gt (cuteSV_resolveTRA.py:258-309, with count_coverage of
cuteSV_genotype.py:72-93) on the step, name and edge tables of tests/tra_table_helpers.py.

    python tests/golden/make_golden_tra_edges.py      # needs the reference checkout make_golden.py names; CPU only

The reference is imported exactly as make_golden.py imports it, and its call_gt reads the tables through make_golden.py's stub
AlignmentFile.  Nothing of it is copied: the file holds the tables' rows as integers, the calls (chromosomes, positions, support
read ids) and what call_gt returns for each.  A read id i is given to the reference as the name "n%08d" % i.  A call whose first
window is inverted by the clamp (start > stop) makes fetch raise, in pysam as in the stub: it is recorded as "raises"."""
import gzip
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg                                   # noqa: E402  (stubs pysam, imports the reference, puts the repository on the path)
import tra_table_helpers as th                             # noqa: E402


class _Names:
    def __getitem__(self, i):
        return "n%08d" % int(i)


def tra_cases():
    out = []
    for name in th.RECORDED:
        st, T, G = th.table(name)
        hb, want, _ = th.expected(name)
        mg._BAM["store"] = types.SimpleNamespace(chroms=st.chroms, contig_len=st.contig_len, reads_off=st.reads_off, r_start=st.r_start, r_end=st.r_end,
                                                 r_primary=st.r_primary, r_id=st.r_id, names=_Names())
        calls, answers = [], []
        for k in th.tra_calls(st, hb.segments, want):
            if not k["genotyped"]:
                continue
            calls.append([k["chr1"], k["bp1"], k["chr2"], k["bp2"], k["sup"]])
            try:
                r = mg.R_TRA.call_gt("bam", k["bp1"], k["bp2"], st.chroms[k["chr1"]], st.chroms[k["chr2"]], set("n%08d" % i for i in k["sup"]), th.BIAS, G)
                answers.append([str(x) for x in r])
            except ValueError:
                answers.append("raises")
        out.append(dict(table=name, gt_round=G, bias=th.BIAS, chroms=st.chroms, contig_len=st.contig_len.tolist(), reads_off=st.reads_off.tolist(),
                        start=st.r_start.tolist(), end=st.r_end.tolist(), primary=st.r_primary.tolist(), id=st.r_id.tolist(), calls=calls, answers=answers))
    return out


if __name__ == "__main__":
    cases = tra_cases()
    path = os.path.join(HERE, "tra_edges.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(cases, separators=(",", ":")).encode())
    print("%s: %d tables, %d reads, %d calls, %d bytes" % (path, len(cases), sum(len(c["start"]) for c in cases), sum(len(c["calls"]) for c in cases),
                                                           os.path.getsize(path)))
