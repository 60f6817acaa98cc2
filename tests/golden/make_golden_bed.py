#!/usr/bin/env python3
"""include_bed.json.gz: the reference's --include_bed, recorded by running it here (data only: BED texts and records we
synthesise, and what the reference's load_bed / single_pipe return for them).

    python tests/golden/make_golden_bed.py        # needs the reference checkout make_golden_main.py names

load_bed     cuteSV_genotype.py:704-726 on BED texts and the task lists call.cut_tasks makes: unsorted lines, nested and
             overlapping regions after the padding, a region whose padded start equals a task's end, a region that spans two
             task boundaries, a start below 1000 (negative after the padding), a chromosome no task names and a task chromosome
             without a region.
multi_task   the reference's single_pipe (main script :697-743) on ONE contig cut into three tasks, each with its load_bed list,
             over a stub alignment file whose fetch() yields - in start order - the records that overlap the region, as a real
             fetch does.  Beside random records the case holds planted ones: each starts in one task and overlaps only a region
             that begins in the next.  The reference drops them (that region is not in their task's list) although they overlap
             the chromosome's full list: the rule DESIGN.md section 19 keeps."""
import gzip
import json
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden_main import load_main                        # noqa: E402
from make_golden_parse import random_record, _Read            # noqa: E402
from make_golden_split import CHROMS                          # noqa: E402
from cutesv_amd import call                                   # noqa: E402

REF_SPAN_OPS = (0, 2, 3, 7, 8)


def task_list(contigs, batch):
    return [[c, s, e] for c, n in contigs for s, e in call.cut_tasks(n, batch)]


def bed_text(lines):
    return "".join("%s\t%d\t%d\n" % tuple(x) for x in lines)


def run_load_bed(main, text, tasks):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "regions.bed")
        with open(path, "w") as f:
            f.write(text)
        return [[list(r) for r in lst] for lst in main.load_bed(path, tasks)]


def load_bed_cases(main):
    rng = np.random.default_rng(71)
    spec = [
        # unsorted lines; (20000, 23000) begins where task 1 ends; (7500, 22500) spans two boundaries; (-500, 1700) starts below 0;
        # (4000, 7000) and (4000, 10000) share a start; (4200, 6300) is nested; chrUn is in no task; c2 has no region
        ("edges", [("c1", 35000), ("c2", 12000)], 10000,
         [("c1", 21000, 22000), ("c1", 5000, 6000), ("chrUn", 100, 200), ("c1", 5200, 5300), ("c1", 4500, 8000), ("c1", 500, 700), ("c1", 8500, 21500),
          ("c1", 5000, 9000), ("c1", 33000, 36000)]),
        # the example of the issue: the padded region (4000, 7000) is not in the list of task [0, 4000)
        ("seam", [("c1", 8000)], 4000, [("c1", 5000, 6000)]),
        ("one_task", [("c1", 9000), ("c2", 500)], 10000, [("c2", 100, 200), ("c1", 8000, 20000), ("c1", 0, 10)]),
        ("random", [("a", 95000), ("b", 40000), ("c", 7000)], 20000,
         [(str(rng.choice(["a", "a", "b", "c", "d"])), int(s), int(s + rng.integers(1, 30000))) for s in rng.integers(0, 90000, 40)]),
    ]
    cases = []
    for name, contigs, batch, lines in spec:
        tasks = task_list(contigs, batch)
        text = bed_text(lines)
        cases.append(dict(name=name, contigs=[list(c) for c in contigs], batch=batch, bed=text, tasks=tasks, regions=run_load_bed(main, text, tasks)))
    return cases


class _Sam:
    """fetch() as a real alignment file answers it: the records that overlap [s, e), in start order"""

    def __init__(self, reads):
        self.reads = sorted(reads, key=lambda r: r.reference_start)

    def fetch(self, chrom, s, e):
        return iter([r for r in self.reads if r.reference_end > s and r.reference_start < e])


def overlaps(start, end, regions):
    return any(not (end <= b0 or start >= b1) for b0, b1 in regions)


def multi_task_case(main):
    chrom, length, batch = "7", 3_000_000, 1_000_000
    params = dict(sv=30, min_mapq=20, parts=7, min_read_len=500, min_siglength=10, md=0, mi=100, max_size=100000)
    # padded: A (299000, 501000) in task 0; B (1000000, 1051000) begins where task 0 ends; C (1399000, 1451000) with a nested
    # (1409000, 1421000); D (2003000, 2050000) begins in task 2; E (2499000, 2701000)
    lines = [(chrom, 2004000, 2049000), (chrom, 300000, 500000), (chrom, 1410000, 1420000), (chrom, 1001000, 1050000), (chrom, 1400000, 1450000),
             (chrom, 2500000, 2700000)]
    text = bed_text(lines)
    tasks = task_list([(chrom, length)], batch)
    assert len(tasks) == 3
    regions = run_load_bed(main, text, tasks)
    full = sorted((s - 1000, e + 1000) for _, s, e in lines)
    rng = np.random.default_rng(72)
    recs = [random_record(rng, "mt%05d" % i, 7200000 + i) for i in range(260)]
    planted = []
    for k, b0 in enumerate([1_000_000] * 4 + [2_003_000] * 4):              # primary, MAPQ 60, ending 1 .. 2000 bases inside the next task's region
        span = 0
        while span < 6000:                                                   # (long enough to start in front of the task's end)
            d = random_record(rng, "plant%02d" % k, 7300000 + k)
            span = sum(ln for op, ln in d["cigar"] if op in REF_SPAN_OPS)
        d.update(flag=0 if k % 2 == 0 else 16, mapq=60, start=b0 - span + int(rng.integers(1, 2000)))
        assert d["start"] < (b0 // batch) * batch
        planted.append(d["name"])
        recs.append(d)
    recs.sort(key=lambda d: d["start"])
    reads = [_Read(d) for d in recs]
    main.samfile = _Sam(reads)
    per_task = []
    for task, bed in zip(tasks, regions):
        with tempfile.TemporaryDirectory() as tmp:
            tmp += "/"
            os.mkdir(tmp + "signatures")
            main.single_pipe("stub.bam", params["sv"], params["min_mapq"], params["parts"], params["min_read_len"], tmp, task, params["min_siglength"],
                             params["md"], params["mi"], params["max_size"], [tuple(r) for r in bed])
            out = {}
            for fn in os.listdir(tmp + "signatures"):
                for t in ("DEL", "INS", "DUP", "INV", "TRA", "reads"):
                    if fn.endswith(t + ".pickle"):
                        with open(tmp + "signatures/" + fn, "rb") as f:
                            out["reads_table" if t == "reads" else t] = [list(x) for x in pickle.load(f)]
        per_task.append(out)
    main.samfile = None
    # the fixture must show the rule: planted records the reference drops although they overlap the chromosome's full list
    in_table = {row[3] for out in per_task for row in out["reads_table"]}
    by_name = {r.query_name: r for r in reads}
    shown = [n for n in planted if n not in in_table and overlaps(by_name[n].reference_start, by_name[n].reference_end, full)]
    assert len(shown) >= 3, shown
    assert all(len(out["reads_table"]) > 5 for out in per_task)
    return dict(name="multi_task", params=params, chrom=chrom, contig_len=length, batch=batch, bed=text, tasks=tasks, regions=regions, full=[list(r) for r in full],
                chroms=sorted(set(CHROMS) | {chrom}), reads=recs, planted=planted, dropped=shown, out=per_task)


def main_():
    main = load_main()
    data = dict(load_bed=load_bed_cases(main), multi_task=multi_task_case(main))
    path = os.path.join(HERE, "include_bed.json.gz")
    with gzip.open(path, "wt") as f:
        json.dump(data, f)
    mt = data["multi_task"]
    print("include_bed.json.gz: %d bytes; %d load_bed cases; multi_task: %d records, reads rows %s, candidates %s, %d of %d planted records dropped" % (
        os.path.getsize(path), len(data["load_bed"]), len(mt["reads"]), [len(o["reads_table"]) for o in mt["out"]],
        {t: sum(len(o[t]) for o in mt["out"]) for t in ("DEL", "INS", "DUP", "INV", "TRA")}, len(mt["dropped"]), len(mt["planted"])))


if __name__ == "__main__":
    main_()
