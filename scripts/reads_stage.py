"""What the genotyping reads table costs on the host against the device.

    python scripts/reads_stage.py [--reads N] [--records M] [--reps R] [--warmup W] [--bam PATH] [--bam-chunk PATH] [--out profiles/reads_table.json]

The two inputs of scripts/gates_stage.py, both on contig "7": the contig of scripts/bam_stage.py (N long
reads with ONT-like CIGARs) and a chunk of M short synthetic records - the size of a dense 10 Mb task.  Per input, call.call_bam
with genotype=True, min_support 1 and TRA genotyping from the reads table, reads_table="host" and "device" alternating in one
process on one context; the texts of the two must be equal in every pass.  Recorded per mode: the wall time, the per-stage
`timings` of call_bam and - device mode - the HIP-event times of the append kernels and of the rank gather (csv_reads_timing).
Medians over --reps passes after --warmup passes, with min and max.

On a checkout whose call_bam has no reads_table option (the parent of the commit that added it) the same passes run on its one
path and are recorded as "parent": the figure the host mode of this commit is compared with."""
import argparse
import inspect
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

from cutesv_amd import bam, call, engine, synth                        # noqa: E402
from cutesv_amd.columns import Params                                  # noqa: E402
from bam_stage import CHROMS, make_records, spread                     # noqa: E402
from gates_stage import CONTIG_LEN, chunk_records                      # noqa: E402

HAVE_OPTION = "reads_table" in inspect.signature(call.call_bam).parameters


def measure(ctx, bf, reference, reps, warmup):
    modes = ("host", "device") if HAVE_OPTION else ("parent",)
    cp = call.CallParams(Params.ont(min_support=1, genotype=True))
    walls = {m: [] for m in modes}
    stages = {m: {} for m in modes}
    events = dict(ms_append_kernels=[], ms_rank_gather=[])
    texts, rows = {}, 0
    for it in range(warmup + reps):
        for m in modes:
            t = {}
            kw = dict(reads_table=m) if HAVE_OPTION else {}
            t0 = time.perf_counter()
            texts[m], _ = call.call_bam(bf, reference, cp, ctx=ctx, batch=CONTIG_LEN, timings=t, tra_gt="reads_table", **kw)
            wall = (time.perf_counter() - t0) * 1e3
            if m == "device":
                from cutesv_amd import reads
                ev, rows = reads.timing(ctx), reads.rows(ctx)
            if it >= warmup:
                walls[m].append(wall)
                for k, v in t.items():
                    stages[m].setdefault(k, []).append(v)
                if m == "device":
                    events["ms_append_kernels"].append(ev[0]); events["ms_rank_gather"].append(ev[1])
        assert all(texts[m] == texts[modes[0]] for m in modes) and texts[modes[0]]
    out = dict(records=int(texts[modes[0]].count("\n")), genotyped=int(sum(1 for ln in texts[modes[0]].splitlines() if ln.split("\t")[9].split(":")[0] != "./.")))
    for m in modes:
        out[m] = dict(ms_wall=spread(walls[m]), **{k: spread(v) for k, v in stages[m].items()})
    if HAVE_OPTION:
        out["reads_rows"] = rows
        out["device"].update({k: spread(v) for k, v in events.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--records", type=int, default=50_000)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bam", default=None, help="reuse / write the contig of bam_stage.py here (default: a temporary file)")
    ap.add_argument("--bam-chunk", default=None, help="reuse / write the chunk of short records here")
    ap.add_argument("--write-only", action="store_true", help="write the two inputs and stop (no GPU needed)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bam_writer
    tmp = __import__("tempfile").mkdtemp()
    path, path_chunk = a.bam or os.path.join(tmp, "stage.bam"), a.bam_chunk or os.path.join(tmp, "chunk.bam")
    refs = [(c, CONTIG_LEN) for c in CHROMS]
    if not os.path.exists(path):
        bam_writer.write_bam(path, refs, [dict(d, seq=synth.pseudo_sequence(d["seq_len"], d["seq_key"]), refid=3, tags=[tuple(t) for t in d["tags"]])
                                          for d in make_records(a.reads, a.seed)], level=1)
    if not os.path.exists(path_chunk):
        bam_writer.write_bam(path_chunk, refs, chunk_records(a.records, a.seed), level=1)
    if a.write_only:
        return
    rng = np.random.default_rng(a.seed)
    reference = {"7": np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 160_000_000, dtype=np.uint8)].tobytes()}
    out = dict(input=dict(reads=a.reads, records=a.records, seed=a.seed, reps=a.reps, warmup=a.warmup), reads_table_option=HAVE_OPTION)
    with engine.Context(0) as ctx:
        for name, p in (("contig", path), ("chunk", path_chunk)):
            with bam.BamFile(p) as bf:
                out[name] = measure(ctx, bf, reference, a.reps, a.warmup)
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
