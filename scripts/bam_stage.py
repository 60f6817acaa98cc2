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

The split-read rows (--out-split profiles/bam_split.json), same input and same process: encode_split_reads
on the host for the task's calls (reads already sliced out of the chunk), csv_bam_split_inputs kernels (HIP events) and the wall
time of split_inputs_bam (kernels + the download of the columns), single_pipe_bam with sa="host" and sa="device", task_to_pool,
and single_pipe_bam(sa="host") taken apart: records + decode + CIGAR scan, the SA path (slicing the values, primary_info,
encode_split_reads), the split-read kernel call, names, sequences, tuple assembly.
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


def host_breakdown(ctx, bf, rank, t):
    """single_pipe_bam(sa="host") step by step, with a clock between the steps (same calls, same results)"""
    P = PARAMS
    clock = time.perf_counter
    t0 = clock()
    chunk = bf.records("7", 0, 1 << 40)
    cols = bam.decode(ctx, chunk, host_outputs=False)
    start, end, flag, mapq, qlen = cols["ref_start"], cols["ref_end"], cols["flag"], cols["mapq"], cols["query_len"]
    gate = (cols["cls"] != 0) & (start >= 0)
    parsed = gate & (qlen >= P["min_read_len"])
    use = (parsed & (mapq >= P["min_mapq"])).astype(np.uint8)
    sig = extract.cigar_signatures(ctx, None, None, None, use, from_bam=cols, min_siglength=P["min_siglength"], merge_ins_threshold=P["merge_ins_threshold"],
                                   merge_del_threshold=P["merge_del_threshold"])
    t1 = clock()
    sel = parsed & (cols["cls"] == 1) & (cols["sa_off"][1:] > cols["sa_off"][:-1])
    reads, sp_idx, sp_query = [], [], []
    for i in np.flatnonzero(sel).tolist():
        primary = extract._primary_info(int(flag[i]), mapq[i] >= P["min_mapq"], int(cols["clip_left"][i]), int(cols["clip_right"][i]), int(qlen[i]), int(start[i]), int(end[i]), "7")
        for v in chunk.sa_values(cols, i):
            reads.append((primary, v, int(qlen[i]))); sp_idx.append(i); sp_query.append(int(flag[i]) == 16)
    t2 = clock()
    enc = extract.encode_split_reads(reads, rank)
    t3 = clock()
    ssig = extract.split_signatures(ctx, enc, sv_size=P["sv_size"], min_mapq=P["min_mapq"], max_split_parts=P["max_split_parts"], max_size=P["max_size"])
    t4 = clock()
    rows = np.flatnonzero(gate & (mapq >= P["min_mapq"])).tolist()
    need = set(rows) | set(sig["ins_read"].tolist()) | set(sig["del_read"].tolist()) | set(sp_idx)                     # (_merge names every call's read)
    names = {i: chunk.name(i) for i in need}
    t5 = clock()
    need_seq = set(sig["ins_read"].tolist()) | {sp_idx[r] for r, k in zip(ssig["read"].tolist(), ssig["kind"].tolist()) if k == 1}
    seqs = {i: chunk.sequence(i) for i in need_seq}
    t6 = clock()
    c_ins, c_del = extract.candidates(sig, names, seqs, "7")
    cand = extract._merge(sig, names, seqs, c_ins, c_del, ssig, sp_idx, sp_query, rank)
    reads_info = [(int(start[i]), int(end[i]), 1 if cols["cls"][i] == 1 else 0, names[i], "7") for i in rows]
    t7 = clock()
    for k, v in (("ms_bd_records_decode_scan", t1 - t0), ("ms_bd_sa_slice_primary", t2 - t1), ("ms_bd_sa_encode_split_reads", t3 - t2), ("ms_bd_split_kernel_call", t4 - t3),
                 ("ms_bd_names", t5 - t4), ("ms_bd_sequences", t6 - t5), ("ms_bd_tuple_assembly", t7 - t6)):
        t[k] = v * 1e3
    return (cand, reads_info), chunk, cols, sel, reads


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
    ap.add_argument("--out-split", default=None, help="write the split-read rows (DESIGN.md section 14) here")
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
    split_keys = ("ms_encode_split_reads_host", "ms_split_inputs_kernels", "ms_split_inputs_wall", "ms_single_pipe_bam_sa_host_wall", "ms_single_pipe_bam_sa_device_wall",
                  "ms_task_to_pool_wall", "ms_bd_records_decode_scan", "ms_bd_sa_slice_primary", "ms_bd_sa_encode_split_reads", "ms_bd_split_kernel_call", "ms_bd_names",
                  "ms_bd_sequences", "ms_bd_tuple_assembly")
    keys = keys + split_keys
    sinfo, first_task_to_pool = {}, None
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
            # ---- the split-read rows
            t["ms_single_pipe_bam_sa_host_wall"] = t["ms_single_pipe_bam_wall"]
            t0 = time.perf_counter()
            dev = extract.single_pipe_bam(ctx, bf, "7", 0, 1 << 40, rank, *pv, sa="device")
            t["ms_single_pipe_bam_sa_device_wall"] = (time.perf_counter() - t0) * 1e3
            assert dev == got, "single_pipe_bam(sa='device') differs from sa='host'"
            from cutesv_amd import rebuild
            rebuild.pool_reset(ctx)
            t0 = time.perf_counter()
            tp = extract.task_to_pool(ctx, bf, "7", 0, 1 << 40, rank, *pv, 5 + rank["7"], rank["7"], [0, 5, 10, 15, 20], 0)
            t["ms_task_to_pool_wall"] = (time.perf_counter() - t0) * 1e3
            if it == 0:
                first_task_to_pool = t["ms_task_to_pool_wall"]          # the process's first call: its arenas and the pool are allocated in it
            pool_rows = rebuild.pool_rows(ctx)
            rebuild.pool_reset(ctx)
            bd, chunk, cols, sel, reads = host_breakdown(ctx, bf, rank, t)
            assert bd == got, "the step-by-step run differs from single_pipe_bam"
            t0 = time.perf_counter()
            enc = extract.encode_split_reads(reads, rank)
            t["ms_encode_split_reads_host"] = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            si = extract.split_inputs_bam(ctx, chunk, cols, sel, rank, "7", PARAMS["min_mapq"])
            t["ms_split_inputs_wall"] = (time.perf_counter() - t0) * 1e3
            t["ms_split_inputs_kernels"] = si["ms_device"]
            assert si["n_flagged"] == 0 and all(np.array_equal(si[k], enc[k]) for k in enc), "the device's split inputs differ from encode_split_reads"
            sinfo = dict(sa_calls=si["n_calls"], sa_entries=si["n_entries"], sa_flagged=si["n_flagged"], pool_rows=pool_rows, split_candidates=tp["n_split"])
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
    split = {k: res.pop(k) for k in split_keys}
    line = json.dumps(res)
    print(line)
    sres = dict(metric="bam_split_stage", device=res["device"], reps=a.reps, warmup=a.warmup, records=res["records"], **sinfo, **split,
                ms_task_to_pool_first_call=first_task_to_pool,
                ms_single_pipe_bam_parent_wall=res["ms_single_pipe_bam_wall"],
                note="ms_single_pipe_bam_parent_wall is single_pipe_bam without the keyword: the parent commit's code path on the same file, in the same process")
    sline = json.dumps(sres)
    print(sline)
    if a.out_split:
        os.makedirs(os.path.dirname(os.path.abspath(a.out_split)), exist_ok=True)
        with open(a.out_split, "w") as f:
            f.write(sline + "\n")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
