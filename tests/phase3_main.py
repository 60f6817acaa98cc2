"""Run in a FRESH interpreter by tests/test_phase3_workdir.py (`-m gpu`): resolve.phase3 on a work directory of the reference's
pickles, on device 0.

    python tests/phase3_main.py --cfg cfg3_s025|cfg4_s002|cfg5_s002|cfg3 [--oracle] --out result.json --work DIR

Writes the rows' per-(type, chromosome) digests, whether the process mapped libcutesv_hip.so, the cutesv_amd broker sockets
it could see and its child processes; --oracle: the digests of the same store through the C oracle as well.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from cutesv_amd import resolve, synth                 # noqa: E402
from cutesv_amd.columns import Params, SigStore       # noqa: E402
from cutesv_amd.phase3 import digests                  # noqa: E402


def workload(cfg):
    import helpers
    d = helpers.load_json("digests.json")
    st = {"cfg3_s025": lambda: synth.ont30(scale=0.25), "cfg4_s002": lambda: synth.hifi30_gt(scale=0.02),
          "cfg5_s002": lambda: synth.ont90_all(scale=0.02), "cfg3": lambda: synth.ont30(scale=1.0)}[cfg]()
    return st, Params(**d["cfg3_s025" if cfg == "cfg3" else cfg]["params"])


def children():
    me, out = str(os.getpid()), []
    for pid in os.listdir("/proc"):
        if pid.isdigit():
            try:
                with open("/proc/%s/stat" % pid) as f:
                    if f.read().rsplit(")", 1)[1].split()[1] == me:
                        out.append(int(pid))
            except OSError:
                pass
    return out


def sockets():
    try:
        with open("/proc/net/unix") as f:
            return sorted({ln.split()[-1] for ln in f if "cutesv_amd-" in ln and str(os.getpid()) in ln})
    except OSError:
        return []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg3_s025")
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--out", required=True)
    ap.add_argument("--work", required=True)
    a = ap.parse_args()
    st, p = workload(a.cfg)
    wd = os.path.join(a.work, "wd_%s" % a.cfg) + "/"
    os.makedirs(wd, exist_ok=True)
    idx = st.write_reference_workdir(wd)
    del st
    results = resolve.phase3(wd, idx, p, lazy=False)
    with open("/proc/self/maps") as f:
        mapped = "libcutesv_hip" in f.read()
    out = dict(cfg=a.cfg, digests=digests(results), mapped_hip_library=mapped, sockets=sockets(), children=children())
    if a.oracle:
        class OracleCtx:
            def cluster_batch(self, hb, reuse=False, **kw):
                from oracle import oracle
                return oracle.cluster_batch(hb, per_sig=False)
        want = resolve.cluster_stage(SigStore.from_reference_workdir_native(wd, idx, reads=p.genotype), p, ctx=OracleCtx())
        out["oracle_digests"] = digests(want)
    with open(a.out, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
