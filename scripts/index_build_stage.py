"""Building the BAM index on the three reader routes, by the method of sections 13, 27 and 29: one MI355X, one
process per run, medians of --reps passes after --warmup, with [min, max].

    python scripts/index_build_stage.py [--reads N] [--reps R] [--warmup W] [--dir DIR] [--write-only] [--parent DIR] [--bench-runs K]
                                        [--out profiles/index_build.json]

Inputs: the two of scripts/inflate_stage.py, `constant` and `random` bases, written outside every clock (an existing file in --dir is
reused); --reads makes a larger file.  A run is one (input, route) pair in a process of its own (a fresh child of this script, which
itself never opens the GPU):
  host_host      host inflate, host frame: the host loop over the records
  device_host    device inflate, host frame: the same loop out of the page-locked window
  device_device  device inflate, device frame: the index kernels over the rows of every window
Per pass, with the reader's window dropped before each: BamFile.build_index (wall, the kernels' device time, bytes up and down, runs
and records), then the whole-file counting pass bf.count(None) on the same route - the pass that has to happen anyway; what the build
costs above it is the index work.  For the device route the host_host build of the same job is the second reference; the route's own
earlier run never is.  The built bytes of the three routes must be the same: the script asserts it.

With --parent DIR (a checkout of the parent commit with its library built) the default path is measured against it in the same job:
call_bam through scripts/frame_stage.py's host_host / parent runs, and `bench.py --gpus 1 --steps 20 --warmup 5` --bench-runs times each,
alternating.  Section 27's rule: the default path has not moved when the two [min, max] spreads overlap.  The script reports; it
changes nothing."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = {"host_host": ("host", "host"), "device_host": ("device", "host"), "device_device": ("device", "device")}


def run_child(a):
    """one run: this process opens the GPU (for the device routes), measures one route on one input and prints one JSON line"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
    from cutesv_amd import bam
    from bam_stage import spread
    inflate, frame = ROUTES[a.run_route]
    ctx = None
    if inflate == "device":
        from cutesv_amd import engine
        ctx = engine.Context(0)
    runs, sha, st = {}, None, None
    try:
        with bam.BamFile(a.run_path, index=False) as bf:
            def routes():                                      # (setting the route again drops the window: every pass inflates the whole file)
                bf.set_inflate(ctx)
                bf.set_frame(frame)
            for it in range(a.warmup + a.reps):
                routes()
                st = bf.build_index()
                sha = hashlib.sha1(bf.index_bytes()).hexdigest()
                bf.drop_index()
                routes()
                t0 = time.perf_counter()
                n = bf.count(None)
                ms_count = (time.perf_counter() - t0) * 1e3
                if it >= a.warmup:
                    for k, v in (("ms_build", st["ms"]), ("ms_build_kernels", st["ms_kernels"]), ("ms_count", ms_count), ("ms_build_minus_count", st["ms"] - ms_count)):
                        runs.setdefault(k, []).append(v)
    finally:
        if ctx is not None:
            ctx.close()
    out = {k: spread(v) for k, v in runs.items()}
    out.update(records=st["records"], runs=st["runs"], runs_per_record=st["runs"] / max(st["records"], 1), index_bytes=st["index_bytes"], bytes_down=st["bytes_down"],
               bytes_up=st["bytes_up"], frame_runs=st["frame_runs"], index_windows=st["index_windows"], fallback_blocks=st["fallback_blocks"],
               frame_fallback_blocks=st["frame_fallback_blocks"], tail_records=n, index_sha1=sha)
    print("INDEX_BUILD_STAGE " + json.dumps(out))


def _child_json(cmd, tag, cwd=None, timeout=900):
    print("run: " + " ".join(cmd[2:8]), file=sys.stderr, flush=True)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=cwd)
    if p.returncode != 0:                                      # (a run that failed ends the job: nothing more is started on the device)
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        return None
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith(tag)]
    return json.loads(lines[-1][len(tag):])


def overlap(a, b):
    return a["min"] <= b["max"] and b["min"] <= a["max"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default=None, help="reuse / write the inputs here (default: a temporary directory)")
    ap.add_argument("--write-only", action="store_true", help="write the inputs and stop (no GPU needed)")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: adds the default-path comparison")
    ap.add_argument("--bench-runs", type=int, default=3, help="bench.py runs per side of the default-path comparison")
    ap.add_argument("--out", default=None)
    ap.add_argument("--run-route", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--run-path", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.run_route:
        return run_child(a)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
    from inflate_stage import write_input
    from bam_stage import spread
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
    out = dict(metric="index_build_stage", input=dict(reads=a.reads, seed=a.seed, reps=a.reps, warmup=a.warmup), routes=list(ROUTES))
    for kind, path in paths.items():
        res = dict(file_bytes=os.path.getsize(path))
        for route in ROUTES:
            res[route] = _child_json([sys.executable, me, "--run-route", route, "--run-path", path, "--reps", str(a.reps), "--warmup", str(a.warmup)], "INDEX_BUILD_STAGE ")
            if res[route] is None:
                return 1
        assert len({res[r]["index_sha1"] for r in ROUTES}) == 1, "the routes build different bytes"
        dev, host = res["device_device"], res["host_host"]
        res["device_build_below_host_build_min"] = dev["ms_build"]["median"] < host["ms_build"]["min"]
        out[kind] = res
    if a.parent:
        parent = os.path.abspath(a.parent)
        frame_stage = os.path.join(ROOT, "scripts", "frame_stage.py")
        call = {}
        for kind, path in paths.items():
            call[kind] = {}
            for route in ("host_host", "parent"):
                r = _child_json([sys.executable, frame_stage, "--run-route", route, "--run-path", path, "--seed", str(a.seed), "--reps", str(a.reps), "--warmup", str(a.warmup),
                                 "--parent", parent], "FRAME_STAGE ")
                if r is None:
                    return 1
                call[kind][route] = dict(ms_wall=r["ms_wall"], ms_tasks=r["ms_tasks"], text_sha1=r["text_sha1"])
            call[kind]["same_text"] = call[kind]["host_host"]["text_sha1"] == call[kind]["parent"]["text_sha1"]
            call[kind]["wall_spreads_overlap"] = overlap(call[kind]["host_host"]["ms_wall"], call[kind]["parent"]["ms_wall"])
        out["call_bam_default_path"] = call
        bench = {"this": [], "parent": []}
        for _ in range(a.bench_runs):
            for side, cwd in (("this", ROOT), ("parent", parent)):
                print("run: bench.py (%s)" % side, file=sys.stderr, flush=True)
                p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], capture_output=True, text=True, timeout=900, cwd=cwd)
                if p.returncode != 0:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    return 1
                line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
                bench[side].append(line)
        key = next((k for k in ("step_ms", "ms_per_step", "value", "median_ms") if k in bench["this"][0]), None)
        out["bench"] = dict(key=key, runs=a.bench_runs, lines={s: [{k: v for k, v in ln.items() if isinstance(v, (int, float, str))} for ln in lines] for s, lines in bench.items()})
        if key is not None:
            sp = {s: spread([float(ln[key]) for ln in lines]) for s, lines in bench.items()}
            out["bench"].update(spreads=sp, spreads_overlap=overlap(sp["this"], sp["parent"]))
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
