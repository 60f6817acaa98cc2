"""What the BAM index saves, by the method of section 13: one MI355X, one process per run, the median of
--reps passes after --warmup, with [min, max].

    python scripts/index_stage.py [--reads N] [--reps R] [--warmup W] [--dir DIR] [--write-only] [--parent TREE] [--out profiles/bam_index.json]

Input, written outside every clock with the test-side writers (an existing file in --dir is reused): section 13's contig
(scripts/bam_stage.py) written three times into one file as the contigs c1, c2, c3, and its index (tests/bai_writer.py).
Measured, each in a process of its own:
  (a) last    call_bam(chroms=["c3"])
  (b) bed     call_bam(include_bed=ten regions of 1 kb on c2 and c3, tra_gt="off")
each with the index, with index=False, and - with --parent TREE, a built checkout of the parent commit - on the parent's code, which
knows no index.  The parent is the reference point, not this commit's own unindexed route.  Every variant must give the same text
(its CRC32 is compared).  Also reported, for the record: bench.py --gpus 1 --steps 20 --warmup 5.

Nothing's default depends on these numbers: the claim that is tested is the deterministic one (tests/test_bam_index.py,
tests/test_index_calls.py) - never more compressed bytes read, same bytes out."""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTIGS = ("c1", "c2", "c3")
CONTIG_LEN = 250_000_000
REF_LEN = 160_000_000                                        # every record lies below 150 Mb plus its length


def write_input(path, reads, seed):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
    import bai_writer
    import bam_writer
    from bam_stage import make_records
    from cutesv_amd import synth
    recs = make_records(reads, seed)
    full = [dict(d, name="%s_%s" % (c, d["name"]), seq=synth.pseudo_sequence(d["seq_len"], d["seq_key"]), refid=k, tags=[t for t in map(tuple, d["tags"]) if t[0] != "SA"])
            for k, c in enumerate(CONTIGS) for d in recs]
    bam_writer.write_bam(path, [(c, CONTIG_LEN) for c in CONTIGS], full, level=1)
    bai_writer.write_bai(path)
    with open(path + ".bed", "w") as f:
        for k in range(10):
            f.write("%s\t%d\t%d\n" % (CONTIGS[1 + k % 2], 10_000_000 + 13_000_000 * k, 10_000_000 + 13_000_000 * k + 1000))


def worker(a):
    """one run: --what last|bed, --variant index|noindex|parent, the package taken from --tree -> one JSON line"""
    sys.path.insert(0, a.tree)
    import numpy as np
    from cutesv_amd import call, engine
    from cutesv_amd.columns import Params
    rng = np.random.default_rng(a.seed)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, REF_LEN, dtype=np.uint8)].tobytes()
    reference = {c: bases for c in CONTIGS}
    cp = call.CallParams(Params.ont(min_support=1))
    kw = dict(chroms=[CONTIGS[-1]]) if a.what == "last" else dict(include_bed=a.bam + ".bed")
    stats = {}
    if a.variant != "parent":
        kw.update(index=None if a.variant == "index" else False, read_stats=stats)
    walls, crc = [], None
    with engine.Context(0) as ctx:
        for _ in range(a.warmup + a.reps):
            stats.clear()
            t0 = time.perf_counter()
            text, _ = call.call_bam(a.bam, reference, cp, ctx=ctx, batch=10_000_000, tra_gt="off", as_bytes=True, **kw)
            walls.append((time.perf_counter() - t0) * 1e3)
            crc = zlib.crc32(text)
    w = sorted(walls[a.warmup:])
    print(json.dumps(dict(what=a.what, variant=a.variant, ms_wall=dict(median=w[len(w) // 2], min=w[0], max=w[-1]), records_out=text.count(b"\n"), crc32=crc,
                          compressed_bytes=stats.get("compressed_bytes"), records_read=stats.get("n_records"))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000, help="records per contig")
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default=None, help="reuse / write the input here (default: a temporary directory)")
    ap.add_argument("--write-only", action="store_true", help="write the input and stop (no GPU needed)")
    ap.add_argument("--parent", default=None, metavar="TREE", help="a built checkout of the parent commit: its call_bam is measured in the same job")
    ap.add_argument("--skip-bench", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--what", default=None, choices=["last", "bed"], help=argparse.SUPPRESS)
    ap.add_argument("--variant", default=None, choices=["index", "noindex", "parent"], help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--bam", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.what:
        return worker(a)
    d = os.path.abspath(a.dir or __import__("tempfile").mkdtemp())
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "index_stage_%d.bam" % a.reads)
    if not (os.path.exists(path) and os.path.exists(path + ".bai") and os.path.exists(path + ".bed")):
        write_input(path, a.reads, a.seed)
    if a.write_only:
        print("wrote", path)
        return 0
    res = dict(method="one process per run; median of %d passes after %d, [min, max]; wall milliseconds of call_bam" % (a.reps, a.warmup),
               input=dict(contigs=len(CONTIGS), records_per_contig=a.reads, bam_bytes=os.path.getsize(path)), runs=[])
    for what in ("last", "bed"):
        for variant, tree in (("index", ROOT), ("noindex", ROOT), ("parent", a.parent)):
            if tree is None:
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--what", what, "--variant", variant, "--tree", os.path.abspath(tree), "--bam", path,
                   "--reps", str(a.reps), "--warmup", str(a.warmup), "--seed", str(a.seed)]
            p = subprocess.run(cmd, capture_output=True, text=True, cwd=os.path.abspath(tree))
            if p.returncode:
                raise SystemExit("%s / %s failed:\n%s" % (what, variant, p.stderr[-3000:]))
            res["runs"].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(res["runs"][-1], flush=True)
        same = {r["crc32"] for r in res["runs"] if r["what"] == what}
        assert len(same) == 1, "the variants of %r disagree on the text" % what
    if not a.skip_bench:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], capture_output=True, text=True, cwd=ROOT)
        line = json.loads(p.stdout.strip().splitlines()[-1]) if p.returncode == 0 else None
        res["bench"] = None if line is None else {k: line[k] for k in ("value", "unit", "ms_per_step", "steps", "warmup")}
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
