"""Record framing on the device against host framing, by the method of sections 13 and 27: one MI355X, one
process per run, medians of --reps passes after --warmup, with [min, max].

    python scripts/frame_stage.py [--reads N] [--reps R] [--warmup W] [--dir DIR] [--write-only] [--parent DIR] [--out profiles/bam_frame.json]

Inputs: the two of scripts/inflate_stage.py, `constant` and `random`, written outside every clock (an existing file in --dir is reused).
A run is one (input, route) pair in a process of its own (a fresh child of this script, which itself never opens the GPU):
  host_host      host inflate, host frame       - the default path
  device_host    device inflate, host frame     - the reference point of the route
  device_device  device inflate, device frame   - the route
  parent         --parent DIR: the default path of a checkout of the parent commit built in DIR - the reference point of "the default
                 path did not move" (compared with host_host)
Per pass one call_bam of scripts/call_stage.py (report_readid, min_support 1, one task).  Recorded per run: the wall time, ms_tasks,
ms_inflate, ms_frame (the reader's host wall time outside the inflate), the framing and pack kernels (HIP events), the upload
milliseconds of decode (HIP events), names (wall) and sequences (wall), the bytes over PCIe in each direction per task - the window,
the images, the framing route's own copies - and the fallback blocks.  On the device route no image may be fetched and what the
consumers upload must be their tables alone: the script asserts both.

The rule (section 27's): call.DEFAULT_FRAME becomes "device" only if on BOTH inputs the device route's median ms_tasks lies below
the host-frame route's (device_host) minimum AND call_bam's median wall does not lie above that route's maximum.  The route's own
earlier run is never a reference.  The script prints the verdict; it changes nothing."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = {"host_host": ("host", "host"), "device_host": ("device", "host"), "device_device": ("device", "device"), "parent": ("host", None)}
CONTIG_LEN = 250_000_000


def run_child(a):
    """one run: this process opens the GPU, measures one route on one input and prints one JSON line"""
    root = a.parent if a.run_route == "parent" else ROOT
    sys.path[:0] = [root, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
    import numpy as np
    from cutesv_amd import bam, call, engine, extract, rebuild
    from cutesv_amd.columns import Params
    from bam_stage import spread
    inflate, frame = ROUTES[a.run_route]
    rng = np.random.default_rng(a.seed)
    reference = {"7": np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 160_000_000, dtype=np.uint8)].tobytes()}
    os.environ["CUTESV_AMD_TRA_GT"] = "off"
    cp = call.CallParams(Params.ont(min_support=1))
    acc = {}

    def add(key, v):
        acc[key] = acc.get(key, 0) + v
    # the consumers, wrapped: their upload times and what they send
    dec, names_fn, seqs_fn = bam.decode, rebuild.name_pool_append_chunk, extract.upload_read_sequences

    def decode(ctx, chunk, *args, **kw):
        cols = dec(ctx, chunk, *args, **kw)
        add("ms_upload_decode", cols["ms_upload"]); add("decode_bytes_up", cols["bytes_uploaded"])
        return cols

    def names(ctx, chunk):
        t0 = time.perf_counter()
        r = names_fn(ctx, chunk)
        add("ms_upload_names", (time.perf_counter() - t0) * 1e3)
        framed = getattr(chunk, "framed", False) and not chunk.fetched
        add("names_bytes_up", 20 * chunk.n + 8 if framed else int(chunk.name_columns()[1].sum()) + 8 * (chunk.n + 1))
        return r

    def seqs(ctx, *args, **kw):
        seqs_fn(ctx, *args, **kw)
        info = extract.seq_info(ctx)
        framed = bool(args) and getattr(args[0], "framed", False)                # (its gather tables: 12 bytes a read more)
        add("ms_upload_seqs", float(info["ms_upload"])); add("seqs_bytes_up", int(info["bytes_uploaded"]) + (12 * args[0].n if framed else 0))
    bam.decode, rebuild.name_pool_append_chunk, extract.upload_read_sequences = decode, names, seqs
    runs, text, fetched = {}, None, 0
    with engine.Context(0) as ctx, bam.BamFile(a.run_path) as bf:
        read = bf._read
        chunks = []

        def _read(*args, **kw):
            r = read(*args, **kw)
            st = bf.last_stats
            add("n_tasks", 1); add("compressed_bytes", st["compressed_bytes"]); add("inflated_bytes", st["inflated_bytes"])
            add("slim_bytes", st["slim_bytes"]); add("n_records", st["n_records"])
            for k in ("ms_frame_kernels", "frame_bytes_down", "frame_bytes_up", "frame_fallback_blocks", "right_blocks", "fallback_blocks"):
                add(k, st.get(k, 0))
            chunks.append(r)
            return r
        bf._read = _read
        for it in range(a.warmup + a.reps):
            acc.clear(); chunks.clear()
            t = {}
            kw = dict(inflate=inflate) if frame is None else dict(inflate=inflate, frame=frame)
            t0 = time.perf_counter()
            text, _ = call.call_bam(bf, reference, cp, ctx=ctx, batch=CONTIG_LEN, report_readid=True, timings=t, **kw)
            acc["ms_wall"] = (time.perf_counter() - t0) * 1e3
            for k in ("ms_tasks", "ms_inflate", "ms_frame"):
                acc[k] = t.get(k, 0.0)
            fetched += sum(1 for c in chunks if getattr(c, "fetched", False))
            # bytes over PCIe per task.  down: the inflated window (device inflate with host framing) or the framing route's rows and
            # verdicts; up: the compressed payloads and tables (device inflate), the images or the tables of the three consumers
            n_tasks = max(acc.get("n_tasks", 1), 1)
            consumers_up = acc.get("decode_bytes_up", 0) + acc.get("names_bytes_up", 0) + acc.get("seqs_bytes_up", 0)
            if frame == "device":
                down, up = acc["frame_bytes_down"], acc["frame_bytes_up"] + consumers_up
                assert acc.get("decode_bytes_up", 0) == 12 * acc["n_records"], "the decode uploaded more than its offset tables"
            elif inflate == "device":
                down, up = acc["inflated_bytes"] + acc.get("n_tasks", 0), acc["compressed_bytes"] + consumers_up
            else:
                down, up = 0, consumers_up
            acc["pcie_down_per_task"], acc["pcie_up_per_task"], acc["consumers_up_per_task"] = down / n_tasks, up / n_tasks, consumers_up / n_tasks
            if it >= a.warmup:
                for k, v in acc.items():
                    runs.setdefault(k, []).append(v)
    assert frame != "device" or fetched == 0, "an image was fetched on the device route"
    out = {k: spread(v) if k.startswith("ms_") else v[0] for k, v in runs.items()}
    out["frame_fallback_blocks"] = max(runs.get("frame_fallback_blocks", [0]))
    out["images_fetched"] = fetched
    out["text_lines"] = text.count("\n")
    import hashlib
    out["text_sha1"] = hashlib.sha1(text.encode()).hexdigest()
    print("FRAME_STAGE " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default=None, help="reuse / write the inputs here (default: a temporary directory)")
    ap.add_argument("--write-only", action="store_true", help="write the inputs and stop (no GPU needed)")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: adds the `parent` run")
    ap.add_argument("--out", default=None)
    ap.add_argument("--run-route", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--run-path", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.run_route:
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
    routes = [r for r in ROUTES if r != "parent" or a.parent]
    out = dict(metric="bam_frame_stage", input=dict(reads=a.reads, seed=a.seed, reps=a.reps, warmup=a.warmup), routes=routes)
    verdict = True
    for kind, path in paths.items():
        res = dict(file_bytes=os.path.getsize(path))
        for route in routes:
            cmd = [sys.executable, os.path.abspath(__file__), "--run-route", route, "--run-path", path, "--seed", str(a.seed), "--reps", str(a.reps), "--warmup", str(a.warmup)]
            if a.parent:
                cmd += ["--parent", os.path.abspath(a.parent)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:                              # (a run that failed ends the job: nothing more is started on the device)
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                return 1
            res[route] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("FRAME_STAGE ")][-1][len("FRAME_STAGE "):])
        assert len({res[r]["text_sha1"] for r in routes}) == 1, "the routes give different texts"
        ref, dev = res["device_host"], res["device_device"]
        res["tasks_device_below_host_frame_min"] = dev["ms_tasks"]["median"] < ref["ms_tasks"]["min"]
        res["wall_device_not_above_host_frame_max"] = dev["ms_wall"]["median"] <= ref["ms_wall"]["max"]
        verdict = verdict and res["tasks_device_below_host_frame_min"] and res["wall_device_not_above_host_frame_max"]
        out[kind] = res
    out["default_frame_by_the_rule"] = "device" if verdict else "host"
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
