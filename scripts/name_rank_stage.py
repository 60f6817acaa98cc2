"""Stage times of the read-name ranking on the GPU.

    python scripts/name_rank_stage.py [--names N] [--inputs contig,uuid,hifi] [--reps R] [--warmup W] [--out profiles/name_ranks.json]

Inputs: the 4 000 names of the synthetic contig of scripts/bam_stage.py ("st%07d", section 13), and N (default 2.3 M: the HiFi 30x
genome's count) synthetic names of two shapes - 36-byte random UUIDs (ONT) and
m64011_190830_220126/<zmw>/ccs (HiFi) - of which --repeat (default 10 %) repeat an earlier name, as supplementary records do.
Per input and pass: the upload (name_pool_reset + name_pool_append: host compaction and the copy, wall), the kernels of
csv_name_ranks (HIP events), the number of radix passes, the wall time of name_ranks(host=True) (kernels + download of rank and
first), and the wall time of rebuild_pool_by_name over a pool with one row per name, next to rebuild_pool fed with host ranks.
Baselines, the parent commit's only options, on the same names in the same process: (a) Python's sorted(set(names)) plus a dict
look-up per record (the names as str objects already built: not timed), (b) rebuild.name_ranks_host in numpy.  All three must
agree on every rank.  Medians over --reps passes after --warmup passes, [min, max] as the spread.  One process; run it under a
time limit."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from cutesv_amd import engine, rebuild          # noqa: E402

HBM_COPY_PEAK = 6.29e12                          # bytes/s: the measured device-to-device copy rate of an MI355X (spec: 8.0e12)


def contig_names(n=4000):
    return [b"st%07d" % i for i in range(n)]


def with_repeats(distinct, n, repeat, rng):
    """n names: the distinct ones, then repeats of random earlier ones, shuffled"""
    names = distinct + [distinct[i] for i in rng.integers(0, len(distinct), n - len(distinct)).tolist()]
    return [names[i] for i in rng.permutation(n).tolist()]


def uuid_names(n, repeat, rng):
    k = n - int(n * repeat)
    hexd = np.frombuffer(b"0123456789abcdef", np.uint8)
    raw = rng.integers(0, 16, (k, 32), dtype=np.uint8)
    m = np.full((k, 36), ord("-"), np.uint8)
    cols = [c for c in range(36) if c not in (8, 13, 18, 23)]
    m[:, cols] = hexd[raw]
    blob = m.tobytes()
    return with_repeats([blob[36 * i:36 * i + 36] for i in range(k)], n, repeat, rng)


def hifi_names(n, repeat, rng):
    k = n - int(n * repeat)
    zmw = rng.choice(180_000_000, k, replace=False)
    return with_repeats([b"m64011_190830_220126/%d/ccs" % z for z in zmw.tolist()], n, repeat, rng)


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def measure(ctx, label, names, reps, warmup):
    clock = time.perf_counter
    n = len(names)
    ln = np.fromiter((len(s) for s in names), np.int32, n)
    off = (np.cumsum(ln, dtype=np.int64) - ln).astype(np.int64)
    data = np.frombuffer(b"".join(names), np.uint8)
    strs = [s.decode() for s in names]                      # (what chunk.name(i) per record would have built: not timed)
    rng = np.random.default_rng(5)
    n_seg = 10
    zeros = np.zeros(n_seg, np.uint8)
    rebuild.pool_reset(ctx)
    rebuild.pool_append(ctx, rng.integers(0, n_seg, n), rng.integers(0, 150_000_000, n), rng.integers(30, 5000, n), np.arange(n, dtype=np.int32), np.zeros(n, np.int32))
    keys = ("ms_upload_wall", "ms_kernels", "ms_name_ranks_wall", "ms_rebuild_pool_by_name_wall", "ms_rebuild_pool_host_rank_wall", "ms_baseline_sorted_set_dict",
            "ms_baseline_name_ranks_host")
    runs = {k: [] for k in keys}
    got = None
    for it in range(warmup + reps):
        t = {}
        t0 = clock()
        rebuild.name_pool_reset(ctx)
        rebuild.name_pool_append(ctx, data, off, ln)
        t["ms_upload_wall"] = (clock() - t0) * 1e3
        t0 = clock()
        got = rebuild.name_ranks(ctx, host=True)
        t["ms_name_ranks_wall"] = (clock() - t0) * 1e3
        t["ms_kernels"] = got["ms_device"]
        t0 = clock()
        by_name = rebuild.rebuild_pool_by_name(ctx, zeros, keep_on_device=True)         # (the ranks are fresh: the rebuild alone)
        t["ms_rebuild_pool_by_name_wall"] = (clock() - t0) * 1e3
        t0 = clock()
        uniq = sorted(set(strs))
        at = {s: r for r, s in enumerate(uniq)}
        rank_a = [at[s] for s in strs]
        t["ms_baseline_sorted_set_dict"] = (clock() - t0) * 1e3
        t0 = clock()
        rank_b, first_b = rebuild.name_ranks_host(data, off, ln)
        t["ms_baseline_name_ranks_host"] = (clock() - t0) * 1e3
        t0 = clock()
        by_host = rebuild.rebuild_pool(ctx, rank_b, zeros, keep_on_device=True)
        t["ms_rebuild_pool_host_rank_wall"] = (clock() - t0) * 1e3
        assert np.array_equal(got["rank"], rank_b) and np.array_equal(got["first"], first_b) and got["rank"].tolist() == rank_a, "the three rankings differ"
        assert by_name["n_out"] == by_host["n_out"] and np.array_equal(by_name["src_row"], by_host["src_row"]), "rebuild by name differs from rebuild by host ranks"
        if it >= warmup:
            for k in keys:
                runs[k].append(t[k])
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)
    res = dict(input=label, names=n, distinct=got["n_distinct"], max_len=got["max_len"], name_bytes=int(ln.sum()), n_passes=got["n_passes"],
               **{k: spread(v) for k, v in runs.items()})
    # what one radix pass moves: the histogram kernel reads the permutation and gathers the word (4 + 8 bytes per name), the scatter
    # reads both again and writes the permutation (4 + 8 + 4).  The kernel time also holds the pack and rank kernels, so the rate is
    # a lower bound of the passes' own.
    res["bytes_per_pass"] = 28 * n
    if got["n_passes"]:
        per_pass_s = res["ms_kernels"]["median"] * 1e-3 / got["n_passes"]
        res["pass_fraction_of_hbm_copy_peak"] = 28 * n / per_pass_s / HBM_COPY_PEAK
    res["speedup_kernels_plus_upload_vs_numpy"] = res["ms_baseline_name_ranks_host"]["median"] / (res["ms_upload_wall"]["median"] + res["ms_name_ranks_wall"]["median"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", type=int, default=2_300_000)
    ap.add_argument("--repeat", type=float, default=0.10)
    ap.add_argument("--inputs", default="contig,uuid,hifi")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    make = dict(contig=lambda: contig_names(), uuid=lambda: uuid_names(a.names, a.repeat, np.random.default_rng(11)),
                hifi=lambda: hifi_names(a.names, a.repeat, np.random.default_rng(12)))
    rows = []
    with engine.Context(0) as ctx:
        for label in a.inputs.split(","):
            rows.append(measure(ctx, label, make[label](), a.reps, a.warmup))
            print(json.dumps(rows[-1]), flush=True)
    res = dict(metric="name_rank_stage", device="gfx950", compute_units=engine.device_info(0)[1], sort="permutation sort of sort.hip.h over the word columns (the only form tried)",
               reps=a.reps, warmup=a.warmup, hbm_copy_peak_bytes_per_s=HBM_COPY_PEAK, rows=rows)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
