"""What sorting a BAM file by coordinate costs on the device and on the host.

    python scripts/sort_stage.py [--reads N] [--reps 5] [--warmup 1] [--threads 16] [--out profiles/bam_sort.json]

One timeout-guarded GPU process.  Two inputs, made once: section 13's contig (scripts/bam_stage.py) with its records shuffled, and the
same records with random bases and qualities - the two inputs of section 27 (scripts/inflate_stage.py writes them).  Per input:
bam.sort_bam on the device route with the reader on its framing route - wall, and the device time of the key kernel, the radix passes
with the prefix sums, the gather and the compressor - median [min, max] of --reps passes after --warmup; against the host route in the
same job on --threads threads: the file inflated by the reader, a numpy stable argsort of the keys, a gather through it and
csv_bgzf_deflate_host.  The gather kernel's rate - it reads and writes every byte once - stands next to csv_measure_copy_bandwidth's
device-to-device figure of the same job, the roof for such a kernel.  The first pass of each route is checked against the judge of
tests/sort_helpers.py."""
import argparse
import json
import os
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

from cutesv_amd import bam, bgzf, engine                    # noqa: E402
import sort_helpers as sh                                   # noqa: E402
from inflate_stage import write_input                       # noqa: E402


def stat(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def shuffled_input(d, kind, reads, seed):
    """-> (path of the shuffled file, the inflated stream of it)"""
    src = os.path.join(d, kind + ".sorted.bam")
    write_input(src, kind, reads, seed)
    head, recs = sh.split_stream(sh.inflate_file(src))
    rng = np.random.default_rng(seed + 5)
    l_text = struct.unpack_from("<i", head, 4)[0]
    text = head[8 : 8 + l_text].replace(b"SO:coordinate", b"SO:unsorted")
    stream = b"BAM\1" + struct.pack("<i", len(text)) + text + head[8 + l_text :] + b"".join(recs[i] for i in rng.permutation(len(recs)))
    path = os.path.join(d, kind + ".bam")
    sh.write_stream(path, stream)
    return path, stream


def host_baseline(path, stream, threads):
    """the host route a numpy user would write: reader inflate (threads), keys, stable argsort, gather, csv_bgzf_deflate_host on one
    thread per call spread over a pool -> (ms, the inflated result)"""
    from concurrent.futures import ThreadPoolExecutor
    t0 = time.perf_counter()
    data = np.frombuffer(sh.inflate_file(path), np.uint8)
    l_text = struct.unpack_from("<i", stream, 4)[0]
    o = 12 + l_text
    for _ in range(struct.unpack_from("<i", stream, 8 + l_text)[0]):
        o += 8 + struct.unpack_from("<i", stream, o)[0]
    head, starts = stream[:o], []
    while o < len(data):
        starts.append(o)
        o += 4 + int(data[o : o + 4].view("<i4")[0])
    starts = np.asarray(starts, np.int64)
    w = lambda off, dt: np.ascontiguousarray(data[(starts + off)[:, None] + np.arange(np.dtype(dt).itemsize)]).view(dt).ravel()      # noqa: E731
    refid, pos, flag, ln = w(4, "<i4").astype(np.int64), w(8, "<i4").astype(np.int64), w(18, "<u2").astype(np.int64), w(0, "<i4").astype(np.int64) + 4
    n_ref = struct.unpack_from("<i", head, 8 + struct.unpack_from("<i", head, 4)[0])[0]
    key = (np.where(refid < 0, n_ref, refid) << 33) | ((pos + 1) << 1) | ((flag >> 4) & 1)
    order = np.argsort(key, kind="stable")
    dst = np.zeros(len(order) + 1, np.int64)
    dst[1:] = np.cumsum(ln[order])
    src = np.repeat(starts[order] - dst[:-1], ln[order]) + np.arange(dst[-1])
    out = np.concatenate([np.frombuffer(sh.judge_header(head), np.uint8), data[src]])
    cuts = list(zip(*bgzf._cuts(len(out))))
    share = [cuts[k::threads] for k in range(threads)]
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(lambda part: [bgzf.deflate_blocks(None, out, [int(o)], [int(k)], route="core") for o, k in part], share))
    return (time.perf_counter() - t0) * 1e3, out.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = dict(reps=a.reps, warmup=a.warmup, host_threads=a.threads, inputs=[])
    d = tempfile.mkdtemp()
    with engine.Context(0) as ctx:
        result["copy_gb_per_s"] = ctx.copy_bandwidth()
        for kind in ("constant", "random"):
            path, stream = shuffled_input(d, kind, a.reads, a.seed)
            want = sh.judge(stream)[0]
            runs = {k: [] for k in ("ms", "ms_keys", "ms_sort", "ms_gather", "ms_deflate", "ms_host_twin", "ms_host_numpy")}
            st = None
            for it in range(a.warmup + a.reps):
                out = os.path.join(d, "out.bam")
                st = bam.sort_bam(path, out, ctx=ctx, route="device", inflate=ctx, frame="device", overwrite=True)
                if it == 0:
                    assert sh.inflate_file(out) == want, kind
                t0 = time.perf_counter()
                bam.sort_bam(path, out, route="host", threads=a.threads, overwrite=True)
                ms_twin = (time.perf_counter() - t0) * 1e3
                ms_np, got = host_baseline(path, stream, a.threads)
                if it == 0:
                    assert got == want, kind
                if it >= a.warmup:
                    for k in ("ms", "ms_keys", "ms_sort", "ms_gather", "ms_deflate"):
                        runs[k].append(st[k])
                    runs["ms_host_twin"].append(ms_twin); runs["ms_host_numpy"].append(ms_np)
            entry = dict(input=kind, records=st["records"], inversions=st["inversions"], inflated_bytes=st["inflated_bytes"], out_bytes=st["out_bytes"], blocks=st["blocks"],
                         slices=st["slices"], passes=st["passes"], bytes_up=st["bytes_up"], bytes_down=st["bytes_down"], **{k: stat(v) for k, v in runs.items()})
            entry["gather_gb_per_s"] = 2.0 * st["stream_bytes"] / (entry["ms_gather"]["median"] * 1e-3) / 1e9 if entry["ms_gather"]["median"] > 0 else None
            print(json.dumps(entry), flush=True)
            result["inputs"].append(entry)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
