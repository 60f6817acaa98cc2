"""The CSI build against the BAI build on section 30's inputs, by the method of scripts/index_build_stage.py: one
MI355X, one process per run, medians of --reps passes after --warmup, with [min, max].

    python scripts/csi_stage.py [--reads N] [--reps R] [--warmup W] [--dir DIR] [--write-only] [--out profiles/csi_index.json]

Inputs: the two of scripts/inflate_stage.py, `constant` and `random` bases, written outside every clock (an existing file in --dir is
reused).  A run is one (input, format) pair in a process of its own (a fresh child of this script, which itself never opens the GPU),
on the device route - device inflate, device framing, the index kernels over the rows of every window:
  bai    BamFile.build_index(): the linear arrays come down at the end
  csi    BamFile.build_index(format="csi"): htslib's scheme for the file; k_index_loff gathers one loffset per bin, the arrays stay
Per pass, with the reader's window dropped before each: wall, the kernels' device time, bytes down - and for csi the device time of
k_index_loff alone and the bins it served.  No gate and no default depend on these numbers.  The script reports; it changes nothing."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ("bai", "csi")


def run_child(a):
    """one run: this process opens the GPU, measures one format on one input and prints one JSON line"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
    from cutesv_amd import bam, engine
    from bam_stage import spread
    ctx = engine.Context(0)
    runs, sha, st = {}, None, None
    try:
        with bam.BamFile(a.run_path, index=False) as bf:
            for it in range(a.warmup + a.reps):
                bf.set_inflate(ctx)                             # (setting the route again drops the window: every pass inflates the whole file)
                bf.set_frame("device")
                st = bf.build_index(format=a.run_format)
                sha = hashlib.sha1(bf.index_payload() if a.run_format == "csi" else bf.index_bytes()).hexdigest()
                bf.drop_index()
                if it >= a.warmup:
                    for k in ("ms", "ms_kernels") + (("ms_loff",) if a.run_format == "csi" else ()):
                        runs.setdefault(k, []).append(st[k])
    finally:
        ctx.close()
    out = {k: spread(v) for k, v in runs.items()}
    out.update(records=st["records"], runs=st["runs"], index_bytes=st["index_bytes"], bytes_down=st["bytes_down"], bytes_up=st["bytes_up"], index_windows=st["index_windows"],
               fallback_blocks=st["fallback_blocks"], frame_fallback_blocks=st["frame_fallback_blocks"], bins=st.get("bins"), sha1=sha)
    print("CSI_STAGE " + json.dumps(out))


def _child_json(cmd, tag, timeout=900):
    print("run: " + " ".join(cmd[2:8]), file=sys.stderr, flush=True)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:                                      # (a run that failed ends the job: nothing more is started on the device)
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        return None
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith(tag)]
    return json.loads(lines[-1][len(tag):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default=None, help="reuse / write the inputs here (default: a temporary directory)")
    ap.add_argument("--write-only", action="store_true", help="write the inputs and stop (no GPU needed)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--run-format", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--run-path", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.run_format:
        return run_child(a)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
    from inflate_stage import write_input
    d = a.dir or __import__("tempfile").mkdtemp()
    os.makedirs(d, exist_ok=True)
    paths = {}
    for kind in ("constant", "random"):
        paths[kind] = os.path.join(d, "inflate_stage_%s_%d_%d.bam" % (kind, a.reads, a.seed))
        if not os.path.exists(paths[kind]):
            write_input(paths[kind], kind, a.reads, a.seed)
    if a.write_only:
        print({k: os.path.getsize(p) for k, p in paths.items()})
        return 0
    me = os.path.abspath(__file__)
    out = dict(metric="csi_stage", route="device inflate, device frame", input=dict(reads=a.reads, seed=a.seed, reps=a.reps, warmup=a.warmup), formats=list(FORMATS))
    for kind, path in paths.items():
        res = dict(file_bytes=os.path.getsize(path))
        for fmt in FORMATS:
            res[fmt] = _child_json([sys.executable, me, "--run-format", fmt, "--run-path", path, "--reps", str(a.reps), "--warmup", str(a.warmup)], "CSI_STAGE ")
            if res[fmt] is None:
                return 1
        res["csi_bytes_down_minus_bai"] = res["csi"]["bytes_down"] - res["bai"]["bytes_down"]
        out[kind] = res
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
