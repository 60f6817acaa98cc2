#!/usr/bin/env python3
"""Record tests/golden/refine_edges.json.gz by RUNNING THE REFERENCE's resolvers (run_del / run_ins / run_dup / run_inv / run_tra, as
make_golden.run_reference drives them) on the threshold tables of tests/refine_helpers.py, every table and variant.

    python tests/golden/make_golden_refine.py      # needs the reference checkout make_golden.py names; CPU only

The reference is imported exactly as make_golden.py imports it (same stub `pysam` module).  Nothing of it is copied: the file holds,
per case, the parameters, a sha256 of the input columns (the inputs themselves come from the builders) and per (type, chromosome)
helpers.digest of the reference's rows next to the rows themselves, a read list of more than 64 names as the sha256 of its sorted
names.  An exception of the reference (a zero-width genotype window, say) ends the run: nothing is swallowed."""
import gzip
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg                                   # noqa: E402  (stubs pysam, imports the reference, puts the repository on the path)
import helpers                                             # noqa: E402
import refine_helpers as rh                                # noqa: E402


def refine_cases():
    out = []
    for case in rh.cases():
        t0 = time.time()
        st = rh.store_of(case)
        rows = mg.run_reference(st, case["params"])
        rec = dict(name=case["name"], params=mg.params_to_json(case["params"]), n_sig=st.n_sig, n_reads=st.n_reads, input_sha256=rh.input_digest(st),
                   rows=[[t, c, helpers.digest(t, r), [rh.slim_row(t, x) for x in r]] for (t, c), r in rows.items()])
        rh.check_landing(case, {t: r for t, c, _, r in rec["rows"]})
        out.append(rec)
        print("%-14s sigs=%-7d reads=%-6d rows=%-5d reference %.1f s" % (case["name"], st.n_sig, st.n_reads, sum(len(r) for r in rows.values()), time.time() - t0))
    return out


if __name__ == "__main__":
    cases = refine_cases()
    path = os.path.join(HERE, "refine_edges.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(cases, separators=(",", ":"), sort_keys=True).encode())
    print("%s: %d cases, %d signatures, %d rows, %d bytes" % (path, len(cases), sum(c["n_sig"] for c in cases),
                                                             sum(len(r[3]) for c in cases for r in c["rows"]), os.path.getsize(path)))
