"""What the REF bases of a BGZF-compressed reference cost on the device and on the host.

    python scripts/ref_stage.py [--mb 256] [--ranges 25000] [--reads N] [--reps 7] [--warmup 2] [--threads 16] [--out profiles/ref_gather.json]

One process per run.  The input, made once: a synthetic FASTA of --mb megabases in 8 contigs of 60-base lines, BGZF-compressed by
bgzf.compress (host route), with its .fai and .gzi beside it.  The ranges are shaped like a call set: --ranges of them over the
contigs, half of them single bases, half with lengths log-uniform in [30, 100 000], in random order.  Per pass:
BgzfReference.gather on the device route (wall: the blocks read from the mapping, upload, kernels, download; and the two kernel
times) against the host route (zlib on --threads threads, then ref_core.h's host form) on the same ranges; the bytes are compared
once.  Then the .fai build of the same file on both routes (k_fai_events' rows against zlib and the byte walk), and call.call_bam on the contig of
scripts/bam_stage.py with the plain reference and with its bgzipped twin on both ref_routes.  Median of --reps
passes after --warmup, with [min, max]."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

from cutesv_amd import bam, bgzf, call, engine, fasta, synth               # noqa: E402
from cutesv_amd.columns import Params                                      # noqa: E402


def stat(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def write_fasta(path, contigs, rng, width=60):
    """contigs [(name, bases)] of random ACGT in lines of `width` -> the file; returns nothing: the file is the product"""
    with open(path, "wb") as f:
        for name, n in contigs:
            f.write(b">%s synthetic\n" % name.encode())
            seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n, dtype=np.uint8)]
            full = n // width * width
            lines = np.empty((n // width, width + 1), np.uint8)
            lines[:, :width] = seq[:full].reshape(-1, width)
            lines[:, width] = 10
            f.write(lines.tobytes())
            if n > full:
                f.write(seq[full:].tobytes() + b"\n")


def bgzip(path, threads):
    with open(path, "rb") as f:
        text = f.read()
    image, _ = bgzf.compress(text, route="host", level=6, threads=threads)
    with open(path + ".gz", "wb") as f:
        f.write(image)
    return len(text), len(image)


def call_shaped_ranges(ref, n, rng):
    ci = rng.integers(0, len(ref.names), n)
    length = np.ones(n, np.int64)
    long = rng.permutation(n)[: n // 2]
    length[long] = np.exp(rng.uniform(np.log(30), np.log(100_000), len(long))).astype(np.int64)
    clen = np.asarray(ref.length, np.int64)[ci]
    beg = (rng.random(n) * np.maximum(clen - length, 1)).astype(np.int64)
    return ci, beg, np.minimum(beg + length, clen)


def measure_gather(ctx, gz, n_ranges, reps, warmup, threads, seed):
    ref = fasta.BgzfReference(gz, threads=threads)
    ci, beg, end = call_shaped_ranges(ref, n_ranges, np.random.default_rng(seed))
    runs = dict(ms_device_wall=[], ms_device_inflate_kernel=[], ms_device_gather_kernel=[], ms_host_wall=[])
    for it in range(warmup + reps):
        tm = {}
        t0 = time.perf_counter()
        dev, off = ref.gather(ci, beg, end, ctx=ctx, route="device", timings=tm)
        t1 = time.perf_counter()
        host, _ = ref.gather(ci, beg, end, route="host")
        t2 = time.perf_counter()
        if it == 0:
            assert np.array_equal(dev, host) and int(off[-1]) == int((end - beg).sum())
        if it >= warmup:
            runs["ms_device_wall"].append((t1 - t0) * 1e3); runs["ms_host_wall"].append((t2 - t1) * 1e3)
            runs["ms_device_inflate_kernel"].append(tm["ms_inflate"]); runs["ms_device_gather_kernel"].append(tm["ms_gather"])
    passes = warmup + reps
    entry = dict(ranges=n_ranges, bases=int((end - beg).sum()), blocks_per_pass=ref.stats["blocks"] // (2 * passes), windows_per_pass=ref.stats["windows_device"] // passes,
                 windows_host_after_device=ref.stats["windows_host_after_device"], host_threads=threads, **{k: stat(v) for k, v in runs.items()})
    # DESIGN.md section 27's spread-overlap rule, first half: the device route's median wall lies below the host route's minimum in the same job
    entry["device_median_below_host_min"] = entry["ms_device_wall"]["median"] < entry["ms_host_wall"]["min"]
    ref.close()
    return entry


def measure_fai(ctx, gz, reps, warmup, threads):
    """the .fai of the file when none is there, both routes in turn in every pass (the .gzi beside the file is read)"""
    none = os.path.join(os.path.dirname(gz), ".no-such-index")
    runs, kern, texts, stats = dict(host=[], device=[]), dict(inflate=[], events=[]), {}, {}
    for it in range(warmup + reps):
        for route in ("host", "device"):
            t0 = time.perf_counter()
            ref = fasta.BgzfReference(gz, fai=none, threads=threads, ctx=ctx, route=route)
            t1 = time.perf_counter()
            assert ref.fai_built
            texts[route], stats[route] = ref.fai_text(), ref.stats
            ref.close()
            if it >= warmup:
                runs[route].append((t1 - t0) * 1e3)
                if route == "device":
                    kern["inflate"].append(ref.stats["ms_fai_inflate"]); kern["events"].append(ref.stats["ms_fai_events"])
    assert texts["host"] == texts["device"]
    st = stats["device"]
    assert st["fai_windows_host"] == 0, st
    entry = dict(host_threads=threads, ms_host_wall=stat(runs["host"]), ms_device_wall=stat(runs["device"]), ms_inflate_kernel=stat(kern["inflate"]),
                 ms_events_kernels=stat(kern["events"]), windows_device=st["fai_windows_device"], windows_overflow=st["fai_windows_overflow"], rows=st["fai_rows"])
    entry["device_median_below_host_min"] = entry["ms_device_wall"]["median"] < entry["ms_host_wall"]["min"]
    return entry


def measure_call(ctx, n_reads, reps, warmup, threads, seed, work):
    import bam_writer
    from bam_stage import CHROMS, make_records
    contig_len = 250_000_000
    path = os.path.join(work, "stage.bam")
    recs = make_records(n_reads, seed)
    bam_writer.write_bam(path, [(c, contig_len) for c in CHROMS],
                         [dict(d, seq=synth.pseudo_sequence(d["seq_len"], d["seq_key"]), refid=3, tags=[tuple(t) for t in d["tags"]]) for d in recs], level=1)
    fa = os.path.join(work, "call_ref.fa")
    write_fasta(fa, [("7", 160_000_000)], np.random.default_rng(seed))
    bgzip(fa, threads)
    fasta.Reference(fa, write_fai=True).close()
    ref = fasta.BgzfReference(fa + ".gz", write_fai=True, write_gzi=True, threads=threads)
    ref.close()
    os.environ["CUTESV_AMD_TRA_GT"] = "off"
    cp = call.CallParams(Params.ont(min_support=1))
    runs, texts = dict(ms_plain=[], ms_bgzf_host=[], ms_bgzf_device=[]), {}
    for it in range(warmup + reps):
        for key, open_ref, route in (("ms_plain", lambda: fasta.Reference(fa), None), ("ms_bgzf_host", lambda: fasta.open_reference(fa + ".gz", threads=threads), "host"),
                                     ("ms_bgzf_device", lambda: fasta.open_reference(fa + ".gz", threads=threads), "device")):
            t0 = time.perf_counter()
            r = open_ref()
            with bam.BamFile(path) as bf:
                body, _ = call.call_bam(bf, r, cp, ctx=ctx, batch=contig_len, as_bytes=True, ref_route=route)
            t1 = time.perf_counter()
            r.close()
            texts.setdefault(key, body)
            if it >= warmup:
                runs[key].append((t1 - t0) * 1e3)
    assert texts["ms_plain"] == texts["ms_bgzf_host"] == texts["ms_bgzf_device"]
    return dict(reads=n_reads, records=texts["ms_plain"].count(b"\n"), **{k: stat(v) for k, v in runs.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256, help="megabases of the synthetic FASTA")
    ap.add_argument("--ranges", type=int, default=25_000)
    ap.add_argument("--reads", type=int, default=4000, help="reads of the call_bam input; 0: skip that part")
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = dict(reps=a.reps, warmup=a.warmup)
    with tempfile.TemporaryDirectory() as work, engine.Context(0) as ctx:
        fa = os.path.join(work, "ref.fa")
        t0 = time.perf_counter()
        write_fasta(fa, [("c%d" % i, a.mb * 1_000_000 // 8 + 17 * i) for i in range(8)], np.random.default_rng(a.seed))
        n_text, n_image = bgzip(fa, a.threads)
        ref = fasta.BgzfReference(fa + ".gz", write_fai=True, write_gzi=True, threads=a.threads)
        result["input"] = dict(text_bytes=n_text, compressed_bytes=n_image, blocks=ref.n_blocks, contigs=len(ref.names))
        ref.close()
        print("input: %d bytes -> %d in %.1f s" % (n_text, n_image, time.perf_counter() - t0), file=sys.stderr, flush=True)
        result["gather"] = measure_gather(ctx, fa + ".gz", a.ranges, a.reps, a.warmup, a.threads, a.seed + 1)
        print(json.dumps(result["gather"]), flush=True)
        result["fai_build"] = measure_fai(ctx, fa + ".gz", a.reps, a.warmup, a.threads)
        print(json.dumps(result["fai_build"]), flush=True)
        if a.reads > 0:
            result["call_bam"] = measure_call(ctx, a.reads, a.reps, a.warmup, a.threads, a.seed, work)
            print(json.dumps(result["call_bam"]), flush=True)
    result["default_ref_route"] = fasta.DEFAULT_REF_ROUTE
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
