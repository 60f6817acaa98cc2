"""Stage times of the native BAM reader on one synthetic contig of long reads.

    python scripts/bam_stage.py [--reads N] [--chunk-records K] [--reps R] [--bam PATH] [--out profiles/bam_reader.json]

Input: N reads with the ONT-like CIGAR statistics of synth.cigar_reads (the shape the extraction benchmark uses: ~180
operations per read, clips at both ends), sorted by position, written once with the test-side writer (tests/bam_writer.py)
outside every clock; an existing --bam file of the same N and seed is reused.
Per pass over the contig, summed over its chunks: host inflate ms, framing + packing ms, upload bytes and ms, csv_bam_decode
kernel ms, the CIGAR scan on the device columns (ms_device of csv_cigar_signatures with CSV_CG_FROM_BAM), and the wall time
of the whole pass.  Next to it the path the reader replaces, for the same records: StubRecord objects already built (not
timed), then extract.single_pipe with the context's kernels - the time from objects to candidates.  There is no reference
side: the reference reads BAM through pysam, which the build environment does not have.
Medians over --reps passes after --warmup passes, with min and max as the spread.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from cutesv_amd import bam, engine, extract, synth          # noqa: E402

CHROMS = ["1", "10", "2", "7", "X"]
PARAMS = dict(sv_size=30, min_mapq=20, max_split_parts=7, min_read_len=500, min_siglength=10, merge_del_threshold=0, merge_ins_threshold=100, max_size=100000)


def make_records(n, seed):
    off, cigar, start, _ = synth.cigar_reads(n, seed=seed)
    rng = np.random.default_rng(seed + 1)
    start = np.sort(start % 150_000_000)
    flags = rng.choice([0, 16, 256, 2048, 2064], n, p=[0.45, 0.40, 0.05, 0.05, 0.05])
    mapq = rng.integers(0, 61, n)
    recs = []
    for i in range(n):
        w = cigar[off[i] : off[i + 1]]
        ops = list(zip((w & 15).tolist(), (w >> 4).tolist()))
        qlen = int((w >> 4)[np.isin(w & 15, (0, 1, 4, 7, 8))].sum())
        tags = [["NM", int(rng.integers(0, 900))]]
        if rng.random() < 0.2:
            tags.append(["SA", "%s,%d,%s,%dS%dM%dS,%d,3;" % (CHROMS[int(rng.integers(0, 5))], int(rng.integers(1, 100_000_000)), "+-"[int(rng.integers(0, 2))],
                                                            int(rng.integers(0, 4000)), int(rng.integers(100, 6000)), int(rng.integers(0, 4000)), int(rng.integers(0, 61)))])
        recs.append(dict(name="st%07d" % i, flag=int(flags[i]), mapq=int(mapq[i]), start=int(start[i]), cigar=ops, seq_len=qlen, seq_key=seed * 1000003 + i, tags=tags))
    return recs


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--chunk-records", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=None)
    ap.add_argument("--bam", default=None, help="reuse / write the input here (default: a temporary file)")
    ap.add_argument("--write-only", action="store_true", help="write --bam and stop (no GPU needed)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 5
    import bam_writer
    from helpers import StubRecord
    recs = make_records(a.reads, a.seed)
    path = a.bam or os.path.join(__import__("tempfile").mkdtemp(), "stage.bam")
    if not os.path.exists(path):
        refs = [(c, 250_000_000) for c in CHROMS]
        bam_writer.write_bam(path, refs, [dict(d, seq=synth.pseudo_sequence(d["seq_len"], d["seq_key"]), refid=3, tags=[tuple(t) for t in d["tags"]]) for d in recs], level=1)
    if a.write_only:
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
        return
    rank = {c: i for i, c in enumerate(CHROMS)}
    pv = tuple(PARAMS.values())
    stubs = [StubRecord(d) for d in recs]                    # (not timed: the parent path starts from objects)
    keys = ("ms_inflate", "ms_frame", "ms_upload", "ms_decode_kernels", "ms_cigar_scan", "ms_pass_wall", "ms_single_pipe_bam_wall", "ms_objects_single_pipe_wall")
    runs = {k: [] for k in keys}
    info = {}
    with engine.Context(0) as ctx, bam.BamFile(path, threads=a.threads) as bf:
        cig = lambda *x, **k: extract.cigar_signatures(ctx, *x, **k)          # noqa: E731
        spl = lambda enc, **k: extract.split_signatures(ctx, enc, **k)        # noqa: E731
        want = None
        for it in range(a.warmup + a.reps):
            t = dict.fromkeys(keys, 0.0)
            t0 = time.perf_counter()
            n = up = infl = rec_b = n_ops = 0
            for ch in bf.chunks("7", chunk_records=a.chunk_records):
                cols = bam.decode(ctx, ch, host_outputs=False)
                sig = extract.cigar_signatures(ctx, None, None, None, (cols["mapq"] >= 20).astype(np.uint8), from_bam=cols)
                t["ms_inflate"] += ch.stats["ms_inflate"]; t["ms_frame"] += ch.stats["ms_frame"]
                t["ms_upload"] += cols["ms_upload"]; t["ms_decode_kernels"] += cols["ms_device"]; t["ms_cigar_scan"] += sig["ms_device"]
                n += ch.n; up += cols["bytes_uploaded"]; infl += ch.stats["inflated_bytes"]; rec_b += ch.stats["record_bytes"]; n_ops += cols["n_ops"]
            t["ms_pass_wall"] = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            got = extract.single_pipe_bam(ctx, bf, "7", 0, 1 << 40, rank, *pv)
            t["ms_single_pipe_bam_wall"] = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            obj = extract.single_pipe(stubs, "7", 0, rank, *pv, cig, spl)
            t["ms_objects_single_pipe_wall"] = (time.perf_counter() - t0) * 1e3
            assert got == obj, "single_pipe_bam differs from single_pipe on the same records"
            want = obj
            if it >= a.warmup:
                for k in keys:
                    runs[k].append(t[k])
            info = dict(records=n, cigar_ops=n_ops, upload_bytes_per_record=up / n, inflated_bytes_per_record=rec_b / n, inflated_bytes=infl,
                        file_bytes=os.path.getsize(path), candidates=sum(len(v) for v in want[0].values()), reads_rows=len(want[1]))
    res = dict(metric="bam_reader_stage", device=engine.device_name(0) if hasattr(engine, "device_name") else "gfx950", threads=bf.threads, chunk_records=a.chunk_records,
               reps=a.reps, warmup=a.warmup, **info, **{k: spread(v) for k, v in runs.items()})
    up_ms, dec_ms = res["ms_upload"]["median"], res["ms_decode_kernels"]["median"]
    res["decode_vs_upload"] = "decode kernels %.3f ms vs upload %.3f ms per pass" % (dec_ms, up_ms)
    res["note"] = ("no reference side: the reference reads BAM through pysam, absent here; ms_objects_single_pipe_wall starts from StubRecord objects "
                   "already built and is the parent commit's objects-to-candidates path on the same records")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
