"""BGZF inflate on the device against the host threads, by the method of section 13: one MI355X, one process,
medians of --reps passes after --warmup, with [min, max].

    python scripts/inflate_stage.py [--reads N] [--reps R] [--warmup W] [--dir DIR] [--write-only] [--skip-call] [--out profiles/bgzf_inflate.json]

Inputs, written outside every clock with the test-side writer (an existing file in --dir is reused):
  constant   section 13's contig (scripts/bam_stage.py): pseudo-random bases, every quality 0xff - it compresses about 22:1
  random     the same records with random bases and random qualities (0 .. 41): a ratio closer to a real file's
Per input, alternating in one process so that no route runs on a machine state the other did not see:
  * the whole-file counting pass (csv_bam_read with CSV_BAM_COUNT_ONLY over the contig) on the host route and on the device route
    at window_blocks 256, 1024, 4096 and 16384.  ms_inflate is the reader's wall time in its inflate step: on the device route
    staging, upload, kernels, download and fallback; ms_inflate_kernels the kernel time (HIP events); bytes in and out;
    fallback_blocks, which must be 0.
  * call_bam of scripts/call_stage.py (report_readid, min_support 1, one task) with inflate="host" and inflate="device".
The reference point of every comparison is the host route in the same job on the same file: the parent commit's code path.

The rule (section 27): window_blocks takes the size with the lowest median ms_inflate; call.DEFAULT_INFLATE becomes "device" only
if on BOTH inputs the device route's median ms_inflate lies below the host route's minimum AND call_bam's median wall with it does
not lie above the host route's maximum.  The script prints the verdict; it changes nothing."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

from cutesv_amd import _abi, bam, call, engine, synth       # noqa: E402
from cutesv_amd.columns import Params                       # noqa: E402
from bam_stage import CHROMS, make_records, spread          # noqa: E402

CONTIG_LEN = 250_000_000
WINDOWS = (256, 1024, 4096, 16384)


def write_input(path, kind, reads, seed):
    import bam_writer
    recs = make_records(reads, seed)
    refs = [(c, CONTIG_LEN) for c in CHROMS]
    if kind == "constant":
        full = [dict(d, seq=synth.pseudo_sequence(d["seq_len"], d["seq_key"]), refid=3, tags=[tuple(t) for t in d["tags"]]) for d in recs]
        bam_writer.write_bam(path, refs, full, level=1)
        return
    rng = np.random.default_rng(seed + 2)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    full = [dict(d, seq=acgt[rng.integers(0, 4, d["seq_len"], dtype=np.uint8)].tobytes().decode(), refid=3, tags=[tuple(t) for t in d["tags"]]) for d in recs]
    orig = bam_writer.record_bytes

    def with_qualities(r, cg=False):                        # the writer fills the qualities with 0xff: random ones are put in their place
        blob, offs = orig(r, cg=cg)
        n = len(r["seq"])
        q = rng.integers(0, 42, n, dtype=np.uint8).tobytes()
        return blob[: offs["qual"]] + q + blob[offs["qual"] + n :], offs
    try:
        bam_writer.record_bytes = with_qualities
        bam_writer.write_bam(path, refs, full, level=1)
    finally:
        bam_writer.record_bytes = orig


def counting_pass(bf):
    """every record of the contig, counted: -> (records, sums of the reader's figures over its reads)"""
    tot = dict(ms_inflate=0.0, ms_frame=0.0, ms_inflate_kernels=0.0, inflated_bytes=0, compressed_bytes=0, device_blocks=0, fallback_blocks=0)
    n, flags = 0, _abi.BAM_RESTART | _abi.BAM_COUNT_ONLY
    t0 = time.perf_counter()
    while True:
        k, more = bf._read("7", -bam.ALL, bam.ALL, 1 << 30, flags)
        n += k
        for key in tot:
            tot[key] += bf.last_stats[key]
        if not more:
            break
        flags = _abi.BAM_COUNT_ONLY
    tot["ms_pass_wall"] = (time.perf_counter() - t0) * 1e3
    return n, tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default=None, help="reuse / write the inputs here (default: a temporary directory)")
    ap.add_argument("--write-only", action="store_true", help="write the inputs and stop (no GPU needed)")
    ap.add_argument("--skip-call", action="store_true", help="only the counting passes")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d = a.dir or __import__("tempfile").mkdtemp()
    os.makedirs(d, exist_ok=True)
    paths = {}
    for kind in ("constant", "random"):
        paths[kind] = os.path.join(d, "inflate_stage_%s_%d_%d.bam" % (kind, a.reads, a.seed))
        if not os.path.exists(paths[kind]):
            write_input(paths[kind], kind, a.reads, a.seed)
    if a.write_only:
        print({k: os.path.getsize(p) for k, p in paths.items()})
        return
    rng = np.random.default_rng(a.seed)
    reference = {"7": np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 160_000_000, dtype=np.uint8)].tobytes()}
    os.environ["CUTESV_AMD_TRA_GT"] = "off"
    cp = call.CallParams(Params.ont(min_support=1))
    out = dict(metric="bgzf_inflate_stage", input=dict(reads=a.reads, seed=a.seed, reps=a.reps, warmup=a.warmup), windows=list(WINDOWS))
    verdict = True
    with engine.Context(0) as ctx:
        for kind, path in paths.items():
            routes = [("host", None, 0)] + [("device_%d" % w, ctx, w) for w in WINDOWS]
            runs = {name: {} for name, _, _ in routes}
            res = dict(file_bytes=os.path.getsize(path))
            with bam.BamFile(path) as bf:
                res["threads"] = bf.threads
                want = None
                for it in range(a.warmup + a.reps):
                    for name, where, w in routes:
                        bf.set_inflate(where, window_blocks=w)
                        n, tot = counting_pass(bf)
                        want = n if want is None else want
                        assert n == want, "the routes count different records"
                        assert tot["fallback_blocks"] == 0, "%s: %d blocks fell back to the host" % (name, tot["fallback_blocks"])
                        assert (tot["device_blocks"] > 0) == (where is not None)
                        if it >= a.warmup:
                            for key, v in tot.items():
                                runs[name].setdefault(key, []).append(v)
                bf.set_inflate(None)
                res["records"] = want
            for name in runs:
                r = runs[name]
                res[name] = dict(ms_inflate=spread(r["ms_inflate"]), ms_inflate_kernels=spread(r["ms_inflate_kernels"]), ms_frame=spread(r["ms_frame"]),
                                 ms_pass_wall=spread(r["ms_pass_wall"]), inflated_bytes=r["inflated_bytes"][0], compressed_bytes=r["compressed_bytes"][0],
                                 device_blocks=r["device_blocks"][0], fallback_blocks=max(r["fallback_blocks"]))
                res[name]["inflated_gb_per_s"] = res[name]["inflated_bytes"] / res[name]["ms_inflate"]["median"] / 1e6
            best = min(WINDOWS, key=lambda w: res["device_%d" % w]["ms_inflate"]["median"])
            res["best_window_blocks"] = best
            dev, host = res["device_%d" % best], res["host"]
            res["inflate_device_below_host_min"] = dev["ms_inflate"]["median"] < host["ms_inflate"]["min"]
            verdict = verdict and res["inflate_device_below_host_min"]
            if not a.skip_call:
                walls = {"host": [], "device": []}
                infl = {"host": [], "device": []}
                texts = {}
                with bam.BamFile(path) as bf:
                    bf.set_inflate(None, window_blocks=best)             # (call_bam sets the context; the window size stays the reader's)
                    for it in range(a.warmup + a.reps):
                        for route in ("host", "device"):
                            t = {}
                            t0 = time.perf_counter()
                            text, _ = call.call_bam(bf, reference, cp, ctx=ctx, batch=CONTIG_LEN, report_readid=True, timings=t, inflate=route)
                            wall = (time.perf_counter() - t0) * 1e3
                            texts[route] = text
                            if it >= a.warmup:
                                walls[route].append(wall); infl[route].append(t["ms_inflate"])
                assert texts["host"] == texts["device"], "call_bam gives different texts on the two routes"
                res["call_bam"] = {r: dict(ms_wall=spread(walls[r]), ms_inflate=spread(infl[r])) for r in walls}
                res["call_bam"]["records_text"] = texts["host"].count("\n")
                res["call_bam_device_not_above_host_max"] = res["call_bam"]["device"]["ms_wall"]["median"] <= res["call_bam"]["host"]["ms_wall"]["max"]
                verdict = verdict and res["call_bam_device_not_above_host_max"]
            out[kind] = res
    out["default_inflate_by_the_rule"] = "device" if (verdict and not a.skip_call) else "host"
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
