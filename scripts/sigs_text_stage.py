"""What the text signature files cost on the device and on the host.

    python scripts/sigs_text_stage.py [--sizes 100000,1000000] [--reps 7] [--warmup 2] [--out profiles/sigs_text.json]

Per size: synthetic signature rows of all five types (INS lengths log-uniform in [30, 2000], read names in synth's 'r%09d' scheme,
coordinates of a human-sized contig set) go into a context's pool, name pool and sequence pool and are rebuilt by name with the
columns kept on the device.  Then, per pass: rebuild.write_sigs into a temporary directory (wall, and the kernels' HIP-event
time) against rebuild.sigs_text_host of the downloaded rebuild plus the same five file writes (wall).  Median of --reps passes
after --warmup, with [min, max]; both routes' files are compared byte for byte once."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from cutesv_amd import engine, rebuild                         # noqa: E402
from cutesv_amd.columns import TYPES                           # noqa: E402
import sigs_helpers                                            # noqa: E402

CHROMS = sorted(["chr%d" % k for k in range(1, 23)] + ["chrX", "chrY"])
SHARE = dict(DEL=0.35, INS=0.45, INV=0.05, DUP=0.05, TRA=0.10)


def synth_rows(n, seed):
    rng = np.random.default_rng(seed)
    nc = len(CHROMS)
    ti = rng.choice(len(TYPES), n, p=[SHARE[t] for t in TYPES])
    ch = rng.integers(0, nc, n)
    a = rng.integers(10_000, 240_000_000, n)
    b = np.where(ti == TYPES.index("DUP"), a + rng.integers(50, 100_000, n), np.exp(rng.uniform(np.log(30), np.log(2000), n)).astype(np.int64))
    b = np.where((ti == TYPES.index("INV")) | (ti == TYPES.index("TRA")), rng.integers(10_000, 240_000_000, n), b)
    aux = np.zeros(n, np.int64)
    ins = ti == TYPES.index("INS")
    aux[ins] = b[ins]
    inv = ti == TYPES.index("INV")
    aux[inv] = rng.integers(0, 2, int(inv.sum()))
    tra = ti == TYPES.index("TRA")
    aux[tra] = rng.integers(0, nc, int(tra.sum())) * 8 + rng.integers(0, 4, int(tra.sum()))
    reads = rng.integers(0, max(1, n // 8), n)
    base = "ACGT" * 501
    rows = dict(seg=(ti * nc + ch).tolist(), a=a.tolist(), b=b.tolist(), aux=aux.tolist(), names=[b"r%09d" % r for r in reads.tolist()],
                seqs={int(k): base[int(k) % 4:int(k) % 4 + int(aux[k])] for k in np.flatnonzero(ins).tolist()}, halves={})
    return rows


def write_host(host, rows, first, out_dir):
    ranges = rebuild.type_row_ranges(np.bincount(host["seg_id"], minlength=len(TYPES) * len(CHROMS)), len(CHROMS))
    for t, (r0, r1) in ranges.items():
        with open(os.path.join(out_dir, t + ".sigs"), "wb") as f:
            f.write(rebuild.sigs_text_host(host, rows["names"], first, rows["seqs"], CHROMS, r0, r1))


def stat(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=21)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = dict(reps=a.reps, warmup=a.warmup, sizes=[])
    with engine.Context(0) as ctx:
        for n in [int(x) for x in a.sizes.split(",")]:
            rows = synth_rows(n, a.seed)
            sigs_helpers.fill_pools(ctx, rows)
            host, first = sigs_helpers.host_rebuild(ctx, len(CHROMS))
            rb = sigs_helpers.kept_rebuild(ctx, len(CHROMS))
            dev, hst, kern = [], [], []
            with tempfile.TemporaryDirectory() as d_dev, tempfile.TemporaryDirectory() as d_host:
                for it in range(a.warmup + a.reps):
                    timing = {}
                    t0 = time.perf_counter()
                    written = rebuild.write_sigs(ctx, rb, CHROMS, d_dev, timing=timing)
                    t1 = time.perf_counter()
                    write_host(host, rows, first, d_host)
                    t2 = time.perf_counter()
                    if it >= a.warmup:
                        dev.append((t1 - t0) * 1e3); hst.append((t2 - t1) * 1e3); kern.append(timing["ms_kernels"])
                for t in TYPES:
                    with open(os.path.join(d_dev, t + ".sigs"), "rb") as f, open(os.path.join(d_host, t + ".sigs"), "rb") as g:
                        assert f.read() == g.read(), t
            entry = dict(n_rows_in=n, n_rows_out=int(rb["n_out"]), bytes=int(sum(written.values())), ms_write_sigs_wall=stat(dev), ms_kernels=stat(kern),
                         ms_host_twin_wall=stat(hst))
            result["sizes"].append(entry)
            print(json.dumps(entry))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
