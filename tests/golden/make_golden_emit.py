#!/usr/bin/env python3
"""Record tests/golden/emit_edges.json.gz by RUNNING THE REFERENCE's resolvers (run_del / run_ins / run_dup / run_inv / run_tra, as
make_golden.run_reference drives them) on the small tables of tests/emit_helpers.py (A, B, C1, C7, C8, D, F).

    python tests/golden/make_golden_emit.py        # needs the reference checkout make_golden.py names; CPU only

The reference is imported exactly as make_golden.py imports it (same stub `pysam` module).  Nothing of it is copied: the file holds,
per table, the parameters, a sha256 of the input columns (the inputs themselves come from the builders) and per (type, chromosome)
helpers.digest of the reference's rows next to the rows themselves - a read list of more than 64 names and an INS sequence of more
than 64 bases as their sha256 (emit_helpers.slim_row).  The output is the same bytes on every run (no time stamp, sorted keys)."""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg                                   # noqa: E402  (stubs pysam, imports the reference, puts the repository on the path)
import helpers                                             # noqa: E402
import emit_helpers as eh                                  # noqa: E402


def emit_cases():
    out = []
    for name in eh.SMALL_TABLES:
        case = eh.case(name)
        rows = mg.run_reference(case.store, case.params)
        out.append(dict(name=name, params=mg.params_to_json(case.params), n_sig=case.n_sig, n_reads=case.store.n_reads, input_sha256=eh.input_digest(case),
                        rows=[[t, c, helpers.digest(t, r), [eh.slim_row(t, x) for x in r]] for (t, c), r in rows.items()]))
        print("%-4s sigs=%-6d reads=%-6d rows=%d" % (name, case.n_sig, case.store.n_reads, sum(len(r) for r in rows.values())))
    return out


if __name__ == "__main__":
    cases = emit_cases()
    path = os.path.join(HERE, "emit_edges.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(cases, separators=(",", ":"), sort_keys=True).encode())
    print("%s: %d tables, %d rows, %d bytes" % (path, len(cases), sum(len(r[3]) for c in cases for r in c["rows"]), os.path.getsize(path)))
