"""What call.call_bam costs, stage by stage, against the route the same file took before it, on the input
of scripts/bam_stage.py (one synthetic contig of long reads).

    python scripts/call_stage.py [--reads N] [--reps R] [--warmup W] [--bam PATH] [--gates host|device] [--out profiles/call_bam.json]

Per pass, in one process and on one context: call_bam (wall, and its stages: tasks, rebuild, cluster, the two gathers, emit) with
report_readid, and the earlier route - single_pipe_bam per task, store_from_unsorted with sequences, x.5 flags and names,
cluster_batch, emit_records (tests/call_helpers.parent_route).  The two texts must be equal.  Medians over --reps passes after
--warmup passes, with min and max.  min_support is 1: the contig is covered about once, so every signature is a call and the
gathers have something to do."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

from cutesv_amd import bam, call, engine, synth             # noqa: E402
from cutesv_amd.columns import Params                       # noqa: E402
from bam_stage import CHROMS, make_records, spread          # noqa: E402
import call_helpers                                         # noqa: E402

CONTIG_LEN = 250_000_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bam", default=None, help="reuse / write the input here (default: a temporary file)")
    ap.add_argument("--gates", default=None, choices=["host", "device"], help="where call_bam evaluates the task gates (default: call_bam's own choice)")
    ap.add_argument("--sigs", action="store_true", help="also write the <TYPE>.sigs files (call_bam(sigs_dir=...), DESIGN.md section 24) and report ms_sigs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bam_writer
    path = a.bam or os.path.join(__import__("tempfile").mkdtemp(), "stage.bam")
    if not os.path.exists(path):
        recs = make_records(a.reads, a.seed)
        bam_writer.write_bam(path, [(c, CONTIG_LEN) for c in CHROMS],
                             [dict(d, seq=synth.pseudo_sequence(d["seq_len"], d["seq_key"]), refid=3, tags=[tuple(t) for t in d["tags"]]) for d in recs], level=1)
    # the REF bases: every record lies on "7", below 150 Mb plus its length
    rng = np.random.default_rng(a.seed)
    reference = {"7": np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 160_000_000, dtype=np.uint8)].tobytes()}
    os.environ["CUTESV_AMD_TRA_GT"] = "off"
    cp = call.CallParams(Params.ont(min_support=1))
    keys = ("ms_call_bam_wall", "ms_tasks", "ms_rebuild", "ms_cluster", "ms_alt_gather", "ms_support_join", "ms_emit", "ms_parent_wall", "ms_parent_tasks",
            "ms_parent_rebuild", "ms_parent_cluster", "ms_parent_emit")
    sigs_dir = __import__("tempfile").mkdtemp() if a.sigs else None
    if a.sigs:
        keys += ("ms_sigs",)
    runs = {k: [] for k in keys}
    info = {}
    with engine.Context(0) as ctx, bam.BamFile(path) as bf:
        for it in range(a.warmup + a.reps):
            t, tp = {}, {}
            t0 = time.perf_counter()
            text, svid = call.call_bam(bf, reference, cp, ctx=ctx, batch=CONTIG_LEN, report_readid=True, timings=t, gates=a.gates, sigs_dir=sigs_dir)
            t["ms_call_bam_wall"] = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            want = call_helpers.parent_route(ctx, bf, reference, cp, batch=CONTIG_LEN, report_readid=True, timings=tp)
            t["ms_parent_wall"] = (time.perf_counter() - t0) * 1e3
            assert text == want, "call_bam and the route through the store disagree"
            t.update({"ms_parent_" + k[3:]: v for k, v in tp.items()})
            if it >= a.warmup:
                for k in keys:
                    runs[k].append(t[k])
            info = dict(n_records_text=text.count("\n"), text_bytes=len(text), svid=svid.tolist())
    out = dict(input=dict(reads=a.reads, seed=a.seed, reps=a.reps, warmup=a.warmup, min_support=1, report_readid=True, gates=a.gates or call.DEFAULT_GATES), **info, **{k: spread(v) for k, v in runs.items()})
    out["call_bam_over_parent"] = out["ms_call_bam_wall"]["median"] / out["ms_parent_wall"]["median"]
    out["gathers_share_of_call_bam"] = (out["ms_alt_gather"]["median"] + out["ms_support_join"]["median"]) / out["ms_call_bam_wall"]["median"]
    if a.sigs:
        out["sigs_share_of_call_bam"] = out["ms_sigs"]["median"] / out["ms_call_bam_wall"]["median"]
        out["sigs_bytes"] = sum(os.path.getsize(os.path.join(sigs_dir, f)) for f in os.listdir(sigs_dir))
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
