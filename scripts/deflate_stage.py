"""What BGZF compression costs on the device and on the host.

    python scripts/deflate_stage.py [--reads N] [--sigs_rows N] [--reps 7] [--warmup 2] [--threads 16] [--out profiles/bgzf_deflate.json]

Two inputs, made once in this process: (a) the VCF text call.call_bam gives with report_readid on the contig of scripts/bam_stage.py
(DESIGN.md section 13), under vcf.header_text; (b) the <TYPE>.sigs text of --sigs_rows synthetic signatures from
scripts/sigs_text_stage.py's generator, the five files back to back.  Per input and pass: bgzf.compress on the
device route (wall: upload + kernels + download + the end-of-file block and the table; and the kernels' HIP-event time) against the
host route on --threads threads at zlib level 6 and at level 1 (wall).  Median of --reps passes after --warmup, with [min, max];
every image is inflated once and compared with the input; the compressed sizes are reported side by side."""
import argparse
import gzip
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

from cutesv_amd import bam, bgzf, call, engine, rebuild, synth, vcf        # noqa: E402
from cutesv_amd.columns import Params, TYPES                               # noqa: E402


def stat(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def vcf_input(ctx, n_reads, seed):
    import bam_writer
    from bam_stage import CHROMS, make_records
    contig_len = 250_000_000
    path = os.path.join(tempfile.mkdtemp(), "stage.bam")
    recs = make_records(n_reads, seed)
    bam_writer.write_bam(path, [(c, contig_len) for c in CHROMS],
                         [dict(d, seq=synth.pseudo_sequence(d["seq_len"], d["seq_key"]), refid=3, tags=[tuple(t) for t in d["tags"]]) for d in recs], level=1)
    rng = np.random.default_rng(seed)
    reference = {"7": np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 160_000_000, dtype=np.uint8)].tobytes()}
    os.environ["CUTESV_AMD_TRA_GT"] = "off"
    with bam.BamFile(path) as bf:
        body, _ = call.call_bam(bf, reference, call.CallParams(Params.ont(min_support=1)), ctx=ctx, batch=contig_len, report_readid=True, as_bytes=True)
    return vcf.header_text([(c, contig_len) for c in CHROMS], "NULL", ["stage.bam", "ref.fa", "out.vcf.gz", "work", "--report_readid"]).encode() + body


def sigs_input(ctx, n_rows, seed):
    import sigs_helpers
    from sigs_text_stage import CHROMS, synth_rows
    rows = synth_rows(n_rows, seed)
    sigs_helpers.fill_pools(ctx, rows)
    rb = sigs_helpers.kept_rebuild(ctx, len(CHROMS))
    parts = []
    with tempfile.TemporaryDirectory() as d:
        rebuild.write_sigs(ctx, rb, CHROMS, d)
        for t in TYPES:
            with open(os.path.join(d, t + ".sigs"), "rb") as f:
                parts.append(f.read())
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)
    return b"".join(parts)


def measure(ctx, name, data, reps, warmup, threads):
    runs = dict(ms_device_wall=[], ms_device_kernels=[], ms_host_level6_wall=[], ms_host_level1_wall=[])
    size = {}
    for it in range(warmup + reps):
        t, tm = time.perf_counter(), {}
        dev, _ = bgzf.compress(data, ctx=ctx, route="device", timings=tm)
        t1 = time.perf_counter()
        h6, _ = bgzf.compress(data, route="host", level=6, threads=threads)
        t2 = time.perf_counter()
        h1, _ = bgzf.compress(data, route="host", level=1, threads=threads)
        t3 = time.perf_counter()
        if it == 0:
            for img in (dev, h6, h1):
                assert gzip.decompress(img) == data, name
            size = dict(bytes_device=len(dev), bytes_host_level6=len(h6), bytes_host_level1=len(h1))
        if it >= warmup:
            runs["ms_device_wall"].append((t1 - t) * 1e3); runs["ms_device_kernels"].append(tm["ms_bgzf_kernels"])
            runs["ms_host_level6_wall"].append((t2 - t1) * 1e3); runs["ms_host_level1_wall"].append((t3 - t2) * 1e3)
    entry = dict(input=name, bytes=len(data), blocks=-(-len(data) // bgzf.BLOCK), host_threads=threads, **size, **{k: stat(v) for k, v in runs.items()})
    entry["device_below_host_level6"] = entry["ms_device_wall"]["median"] < entry["ms_host_level6_wall"]["median"]
    entry["device_below_host_level1"] = entry["ms_device_wall"]["median"] < entry["ms_host_level1_wall"]["median"]
    print(json.dumps(entry), flush=True)
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--sigs_rows", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = dict(reps=a.reps, warmup=a.warmup, inputs=[])
    with engine.Context(0) as ctx:
        for name, make in (("vcf_report_readid", lambda: vcf_input(ctx, a.reads, a.seed)), ("sigs_text", lambda: sigs_input(ctx, a.sigs_rows, 21))):
            t0 = time.perf_counter()
            data = make()
            print("%s: %d bytes made in %.1f s" % (name, len(data), time.perf_counter() - t0), file=sys.stderr, flush=True)
            result["inputs"].append(measure(ctx, name, data, a.reps, a.warmup, a.threads))
    # the rule of DESIGN.md section 34: the device route is the default only if its wall is below the host route's on both inputs, at both levels
    result["device_is_default"] = all(e["device_below_host_level6"] and e["device_below_host_level1"] for e in result["inputs"])
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
