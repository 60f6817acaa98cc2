"""resolve.phase3 on a work directory of the reference's pickles (written before the clock starts): one JSON line.

    python scripts/phase3_stage.py --cfg cfg3|cfg4 [--scale 1.0] [--reps 5] [--threads N] [--oracle] [--ref-T 1,8,16]

walk_ms   SigStore.from_reference_workdir_native alone (the pickles walked, names interned, narrow forms)
gpu_ms    csv_cluster_batch inside phase3 (host to host; --oracle: the C oracle on the CPU instead of the device)
wall_ms   the whole resolve.phase3 call with lazy rows, on a context made before the clock (ctx_ms: what making it took)
crit_ms   the largest single block walked alone on one thread (the walk cannot be shorter than it)
digest    sha256 of the rows' per-(type, chromosome) digests
ref_T     --ref-T: main_ctrl_phase3 with the reference model's five callables (oracle/py_restatement) under a forked
          Pool(T) on the same files, seconds per T - and whether its rows equal phase3's.
Medians over --reps runs after one warm-up run."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cutesv_amd import resolve, synth, _cols_native as cn     # noqa: E402
from cutesv_amd.columns import Params, SigStore, default_threads, _WALK, _map_file     # noqa: E402
from cutesv_amd.phase3 import digests                  # noqa: E402


class _Timed:
    def __init__(self, eng):
        self.eng, self.s = eng, 0.0

    def cluster_batch(self, hb, **kw):
        t = time.perf_counter()
        r = self.eng.cluster_batch(hb, **kw)
        self.s += time.perf_counter() - t
        return r

    def __getattr__(self, k):
        return getattr(self.eng, k)


class _OracleCtx:
    def cluster_batch(self, hb, reuse=False, **kw):
        from oracle import oracle
        return oracle.cluster_batch(hb, per_sig=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg3", choices=["cfg3", "cfg4"])
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=None)
    ap.add_argument("--oracle", action="store_true", help="the C oracle instead of the GPU (no device needed)")
    ap.add_argument("--ref-T", default="", help="comma-separated pool sizes for the reference model's main_ctrl_phase3")
    ap.add_argument("--work", default=None)
    a = ap.parse_args()
    os.environ.setdefault("CUTESV_AMD_TRA_GT", "off")
    if a.cfg == "cfg3":
        st, p = synth.ont30(scale=a.scale), Params.ont()
    else:
        st, p = synth.hifi30_gt(scale=a.scale), Params.hifi(genotype=True)
    wd = tempfile.mkdtemp(prefix="phase3_", dir=a.work) + "/"
    idx = st.write_reference_workdir(wd)
    n_sig, n_reads = st.n_sig, st.n_reads
    del st
    threads = a.threads or default_threads()
    t = time.perf_counter()
    if a.oracle:
        eng = _OracleCtx()
    else:
        from cutesv_amd import engine
        eng = engine.Context(resolve.device_index())
    ctx_ms = (time.perf_counter() - t) * 1e3
    walk, wall, gpu = [], [], []
    res = None
    for k in range(a.reps + 1):
        res = None                                     # (both timings start from the same heap: the previous run's store freed)
        t = time.perf_counter()
        st = SigStore.from_reference_workdir_native(wd, idx, threads=threads, reads=p.genotype)
        w = time.perf_counter() - t
        del st
        te = _Timed(eng)
        t = time.perf_counter()
        res = resolve.phase3(wd, idx, p, threads=threads, ctx=te, lazy=True)
        tot = time.perf_counter() - t
        if k:
            walk.append(w * 1e3); wall.append(tot * 1e3); gpu.append(te.s * 1e3)
    dg = digests(res)
    # the critical-path block: the largest one, walked alone on one thread
    kinds = ["DEL", "INS", "INV", "DUP", "TRA"] + (["reads"] if p.genotype else [])
    big = max(((k, c, o) for k in kinds for c, o in idx.get(k, {}).items()),
              key=lambda x: _block_size(wd, idx, x[0], x[2]))
    mm = _map_file(wd + big[0] + ".pickle")
    width, fi, fs, chk, key = _WALK[big[0]]
    crit = []
    for _ in range(3):
        t = time.perf_counter()
        cn.walk_workdir(((mm, int(big[2]), -1, width, fi, fs, chk, big[1].encode(), key),), 1)
        crit.append((time.perf_counter() - t) * 1e3)
    out = dict(cfg=a.cfg, scale=a.scale, engine="oracle" if a.oracle else "libcutesv_hip.so", n_sig=n_sig, n_reads=n_reads,
               threads=threads, walk_ms=round(statistics.median(walk), 3), gpu_ms=round(statistics.median(gpu), 3),
               wall_ms=round(statistics.median(wall), 3), ctx_ms=round(ctx_ms, 1), crit_block="%s:%s" % big[:2],
               crit_ms=round(min(crit), 3), rows=sum(len(v) for v in res.values()),
               digest=hashlib.sha256(json.dumps(dg, sort_keys=True).encode()).hexdigest())
    if a.ref_T:
        from oracle import py_restatement as pr
        out["ref_T"] = {}
        for T in [int(x) for x in a.ref_T.split(",")]:
            t = time.perf_counter()
            ref = resolve.main_ctrl_phase3(wd, idx, p, T, fns=pr.REF_FNS)
            out["ref_T"][str(T)] = round(time.perf_counter() - t, 3)
            out["ref_rows_equal"] = digests(ref) == dg
    print(json.dumps(out), flush=True)


def _block_size(wd, idx, kind, off):
    offs = sorted(int(o) for o in idx[kind].values())
    nxt = [o for o in offs if o > int(off)]
    return (nxt[0] if nxt else os.path.getsize(wd + kind + ".pickle")) - int(off)


if __name__ == "__main__":
    main()
