"""What SAM text -> BAM costs on the device and on the host.

    python scripts/sam_stage.py [--reads N] [--reps 5] [--warmup 1] [--threads 16] [--out profiles/sam_to_bam.json]

One timeout-guarded GPU process.  Two inputs, made once: section 13's contig (scripts/inflate_stage.py's records) written as SAM text by
the test suite's writer (tests/sam_helpers.py), and the same records with random bases and qualities.  Per input: sam.sam_to_bam on the
device route - wall, and the device time of the marks, the plan, the scan and write kernels, the compressor - median [min, max] of
--reps passes after --warmup; against csv_sam_to_bam_host on --threads threads in the same job.  The write pass reads the text and
writes the stream once: its bytes per second stand next to csv_measure_copy_bandwidth's device-to-device figure of the same job.  The
first pass of each route is checked against the judge of tests/sam_helpers.py."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

from cutesv_amd import engine, sam, synth                   # noqa: E402
import sam_helpers as sh                                    # noqa: E402
from inflate_stage import CHROMS, CONTIG_LEN, make_records  # noqa: E402


def stat(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def write_sam(path, kind, reads, seed):
    recs = make_records(reads, seed)
    refs = [(c, CONTIG_LEN) for c in CHROMS]
    rng = np.random.default_rng(seed + 2)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    full = []
    for d in recs:
        r = dict(d, refid=3, tags=[tuple(t) for t in d["tags"]])
        if kind == "constant":
            r["seq"] = synth.pseudo_sequence(d["seq_len"], d["seq_key"])
        else:
            r["seq"] = acgt[rng.integers(0, 4, d["seq_len"], dtype=np.uint8)].tobytes().decode()
            r["qual"] = (rng.integers(0, 42, d["seq_len"], dtype=np.uint8) + 33).tobytes().decode()
        full.append(r)
    text = sh.sam_text(refs, full)
    with open(path, "wb") as f:
        f.write(text)
    return text


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
            path = os.path.join(d, kind + ".sam")
            want = sh.judge_stream(write_sam(path, kind, a.reads, a.seed))
            runs = {k: [] for k in ("ms", "ms_lines", "ms_plan", "ms_write", "ms_deflate", "ms_host")}
            st = None
            for it in range(a.warmup + a.reps):
                out = os.path.join(d, "out.bam")
                st = sam.sam_to_bam(path, out, ctx=ctx, route="device", overwrite=True)
                if it == 0:
                    assert sh.inflate_file(out) == want, kind
                    with open(out, "rb") as f:
                        dev = f.read()
                hs = sam.sam_to_bam(path, out, route="host", threads=a.threads, overwrite=True)
                if it == 0:
                    with open(out, "rb") as f:
                        assert f.read() == dev, kind
                if it >= a.warmup:
                    for k in ("ms", "ms_lines", "ms_plan", "ms_write", "ms_deflate"):
                        runs[k].append(st[k])
                    runs["ms_host"].append(hs["ms"])
            entry = dict(input=kind, **{k: st[k] for k in ("lines", "records", "text_bytes", "stream_bytes", "out_bytes", "blocks", "windows", "float_patches", "cg_records", "bytes_up", "bytes_down")},
                         **{k: stat(v) for k, v in runs.items()})
            entry["write_gb_per_s"] = (st["text_bytes"] + st["stream_bytes"]) / (entry["ms_write"]["median"] * 1e-3) / 1e9 if entry["ms_write"]["median"] > 0 else None
            print(json.dumps(entry), flush=True)
            result["inputs"].append(entry)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
