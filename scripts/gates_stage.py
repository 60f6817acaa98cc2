"""What the task gates cost on the device against the host.

    python scripts/gates_stage.py [--reads N] [--records M] [--reps R] [--warmup W] [--bam PATH] [--bam-chunk PATH] [--out profiles/task_gates.json]

Two inputs, both on contig "7": the contig of scripts/bam_stage.py (N long reads with ONT-like CIGARs)
and a chunk of M short synthetic records (one match, a clip, an SA tag on four in ten) - the size of a dense 10 Mb task.
Per input and per region table (none, 100 and 10 000 regions spread over the records):
  ms_gates_kernel     the kernel of csv_bam_task_gates alone (HIP events)
  ms_gates_device     the wall time of extract.task_gates: table upload, kernel, the bytes back
  ms_gates_host       the wall time of extract._gates on the same columns, plus the `want` and reads-row masks task_to_pool makes of them
and, without a BED and with the 100-region table, the wall time of extract.task_to_pool with gates="host" and gates="device"
(name pool and sequence pool on, as call_bam runs it; the 10 000-region table is timed for the gates alone).  On the first input
also call.call_bam without a BED, gates="host" against gates="device", same process, same context.  The bits of the two sides must be equal.  Medians over --reps passes after
--warmup passes, with min and max."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

from cutesv_amd import bam, call, engine, extract, rebuild, synth      # noqa: E402
from cutesv_amd.columns import Params                                  # noqa: E402
from bam_stage import CHROMS, PARAMS, make_records, spread             # noqa: E402

CONTIG_LEN = 250_000_000


def chunk_records(n, seed):
    """n short records over 10 Mb of contig "7", in coordinate order"""
    rng = np.random.default_rng(seed)
    start = np.sort(rng.integers(0, 10_000_000, n))
    span = rng.integers(300, 3000, n)
    clip = rng.integers(0, 400, n)
    flag = rng.choice([0, 16, 256, 2048, 2064], n, p=[0.45, 0.40, 0.05, 0.05, 0.05])
    mapq = rng.integers(0, 61, n)
    sa = rng.random(n) < 0.4
    return [dict(name="g%06d" % i, flag=int(flag[i]), mapq=int(mapq[i]), start=int(start[i]), cigar=[(0, int(span[i]))] + ([(4, int(clip[i]))] if clip[i] else []),
                 seq="A" * int(span[i] + clip[i]), tags=[("SA", "7,%d,+,%dS%dM,60,0;" % (int(start[i]) + 5000, int(span[i]), int(clip[i]) + 1))] if sa[i] else [], refid=3)
            for i in range(n)]


def tables(cols, seed):
    """region tables spread over the chunk's records: name -> None or a sorted (k, 2) array (about half of the records lie in one)"""
    rng = np.random.default_rng(seed)
    lo, hi = int(cols["ref_start"].min()), int(cols["ref_end"].max()) + 1
    out = {"no_bed": None}
    for k in (100, 10_000):
        beg = np.sort(rng.integers(lo, hi, k))
        out["%d_regions" % k] = np.stack([beg, beg + max(1, (hi - lo) // (2 * k))], 1).astype(np.int64)
    return out


def measure(ctx, bf, rank, reps, warmup):
    pv = tuple(PARAMS.values())
    chunk = bf.records("7", 0, 1 << 40)
    cols = bam.decode(ctx, chunk, host_outputs=False)
    n = chunk.n
    res = dict(records=n)
    for name, regions in tables(cols, 5).items():
        runs = dict(ms_gates_kernel=[], ms_gates_device=[], ms_gates_host=[])
        for it in range(warmup + reps):
            tm = {}
            t0 = time.perf_counter()
            bits = extract.task_gates(ctx, n, 0, PARAMS["min_read_len"], PARAMS["min_mapq"], regions, timing=tm)
            t1 = time.perf_counter()
            gate, _, use, sel = extract._gates(cols, 0, regions, PARAMS["min_read_len"], PARAMS["min_mapq"])
            want, rows = (use != 0) | sel, gate & (cols["mapq"] >= PARAMS["min_mapq"])
            t2 = time.perf_counter()
            assert np.array_equal(bits, extract.gate_bits_host(cols, 0, regions, PARAMS["min_read_len"], PARAMS["min_mapq"])), name
            assert len(want) == len(rows) == n
            if it >= warmup:
                runs["ms_gates_kernel"].append(tm["ms_device"]); runs["ms_gates_device"].append((t1 - t0) * 1e3); runs["ms_gates_host"].append((t2 - t1) * 1e3)
        res[name] = dict(n_regions=0 if regions is None else len(regions), records_passing=int((bits & 1).sum()), **{k: spread(v) for k, v in runs.items()})
        if name == "10000_regions":
            continue
        for gates in ("host", "device"):
            walls = []
            for it in range(warmup + reps):
                rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)
                t0 = time.perf_counter()
                extract.task_to_pool(ctx, bf, "7", 0, 1 << 40, rank, *pv, 5 + rank["7"], rank["7"], [0, 5, 10, 15, 20], None, bed_regions=regions, name_pool=True,
                                     seq_pool=True, gates=gates)
                if it >= warmup:
                    walls.append((time.perf_counter() - t0) * 1e3)
            res[name]["ms_task_to_pool_gates_" + gates] = spread(walls)
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)
    return res


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
    rank = {c: i for i, c in enumerate(CHROMS)}
    out = dict(input=dict(reads=a.reads, records=a.records, seed=a.seed, reps=a.reps, warmup=a.warmup))
    with engine.Context(0) as ctx:
        with bam.BamFile(path) as bf:
            out["contig"] = measure(ctx, bf, rank, a.reps, a.warmup)
            # call_bam without a BED: the two sides of the gates in one process (min_support 1, as scripts/call_stage.py)
            rng = np.random.default_rng(a.seed)
            reference = {"7": np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 160_000_000, dtype=np.uint8)].tobytes()}
            os.environ["CUTESV_AMD_TRA_GT"] = "off"
            cp = call.CallParams(Params.ont(min_support=1))
            walls, tasks, texts = {"host": [], "device": []}, {"host": [], "device": []}, {}
            for it in range(a.warmup + a.reps):
                for gates in ("host", "device"):
                    t = {}
                    t0 = time.perf_counter()
                    texts[gates], _ = call.call_bam(bf, reference, cp, ctx=ctx, batch=CONTIG_LEN, report_readid=True, timings=t, gates=gates)
                    if it >= a.warmup:
                        walls[gates].append((time.perf_counter() - t0) * 1e3); tasks[gates].append(t["ms_tasks"])
            assert texts["host"] == texts["device"] and texts["host"]
            out["call_bam_no_bed"] = {"ms_wall_gates_" + g: spread(walls[g]) for g in walls}
            out["call_bam_no_bed"].update({"ms_tasks_gates_" + g: spread(tasks[g]) for g in tasks})
        with bam.BamFile(path_chunk) as bf:
            out["chunk"] = measure(ctx, bf, rank, a.reps, a.warmup)
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
