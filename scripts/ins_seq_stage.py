"""What the INS sequence pool costs and what it replaces, on the input of scripts/bam_stage.py
(one synthetic contig of long reads).

    python scripts/ins_seq_stage.py [--reads N] [--reps R] [--warmup W] [--bam PATH] [--out profiles/ins_seq_pool.json]

Per pass, in one process: task_to_pool without and with seq_pool=True (wall); the sequence upload in bytes and ms, packed (the
default) and with the image sent whole (extract.seq_option); the gather kernels of both calls (HIP events, csv_seq_info);
the numpy sequence step of single_pipe_bam - Chunk.sequence of every read with an INS candidate - which the feature replaces;
seq_pool_get of all INS rows; and, on the cases of tests/golden/rebuild_order.json.gz, rebuild_pool with ties="seqs" against
tie_order=tie_callback(...).  Medians over --reps passes after --warmup passes, with min and max."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

from cutesv_amd import bam, engine, extract, rebuild, synth          # noqa: E402
from bam_stage import CHROMS, PARAMS, make_records, spread           # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bam", default=None, help="reuse / write the input here (default: a temporary file)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bam_writer
    path = a.bam or os.path.join(__import__("tempfile").mkdtemp(), "stage.bam")
    if not os.path.exists(path):
        recs = make_records(a.reads, a.seed)
        bam_writer.write_bam(path, [(c, 250_000_000) for c in CHROMS],
                             [dict(d, seq=synth.pseudo_sequence(d["seq_len"], d["seq_key"]), refid=3, tags=[tuple(t) for t in d["tags"]]) for d in recs], level=1)
    rank = {c: i for i, c in enumerate(CHROMS)}
    pv = tuple(PARAMS.values())
    seg = (5 + 3, 3, [0, 5, 10, 15, 20], 0)                  # seg_ins, seg_del, seg_base, read_base
    keys = ("ms_task_to_pool_wall", "ms_task_to_pool_seq_wall", "ms_upload_packed", "ms_upload_whole", "ms_gather_cigar", "ms_gather_split", "ms_numpy_sequences",
            "ms_seq_pool_get_wall", "ms_rebuild_ties_seqs_wall", "ms_rebuild_ties_callback_wall")
    runs = {k: [] for k in keys}
    info = {}
    with engine.Context(0) as ctx, bam.BamFile(path) as bf:
        chunk = bf.records("7", 0, 1 << 40)
        s_off, l_seq = chunk.sequence_columns()
        for it in range(a.warmup + a.reps):
            t = {}
            rebuild.pool_reset(ctx)
            _, t["ms_task_to_pool_wall"] = timed(lambda: extract.task_to_pool(ctx, bf, "7", 0, 1 << 40, rank, *pv, *seg))
            n_rows = rebuild.pool_rows(ctx)
            rebuild.pool_reset(ctx)
            res, t["ms_task_to_pool_seq_wall"] = timed(lambda: extract.task_to_pool(ctx, bf, "7", 0, 1 << 40, rank, *pv, *seg, seq_pool=True))
            assert rebuild.pool_rows(ctx) == n_rows
            t["ms_gather_split"] = extract.seq_info(ctx)["ms_gather"]            # (the split call is the task's last)
            # the pool's INS rows are the CIGAR scan's first n_sig_ins rows and the kind-1 candidates behind the DEL rows
            cols = bam.decode(ctx, chunk, host_outputs=False)
            _, _, use, sel = extract._gates(cols, 0, None, PARAMS["min_read_len"], PARAMS["min_mapq"])
            want = (use != 0) | sel
            extract.seq_option(ctx, whole_image=True)
            extract.upload_read_sequences(ctx, chunk.host, s_off, l_seq, want=want)
            whole = extract.seq_info(ctx)
            extract.seq_option(ctx, whole_image=False)
            extract.upload_read_sequences(ctx, chunk.host, s_off, l_seq, want=want)
            packed = extract.seq_info(ctx)
            t["ms_upload_whole"], t["ms_upload_packed"] = whole["ms_upload"], packed["ms_upload"]
            rebuild.pool_reset(ctx)
            sig = extract.cigar_signatures(ctx, None, None, None, use, min_siglength=PARAMS["min_siglength"], merge_ins_threshold=PARAMS["merge_ins_threshold"],
                                           merge_del_threshold=PARAMS["merge_del_threshold"], from_bam=cols,
                                           pool=dict(seg_ins=seg[0], seg_del=seg[1], read_base=0, query_len=cols["query_len"], seqs=True))
            gi = extract.seq_info(ctx)
            t["ms_gather_cigar"] = gi["ms_gather"]
            _, t["ms_numpy_sequences"] = timed(lambda: [chunk.sequence(i) for i in sorted(set(sig["ins_read"].tolist()))])
            rows = np.arange(sig["n_sig_ins"])
            got, t["ms_seq_pool_get_wall"] = timed(lambda: rebuild.seq_pool_get(ctx, rows, raw=True))
            t["ms_rebuild_ties_seqs_wall"], t["ms_rebuild_ties_callback_wall"] = rebuild_cases(ctx)
            if it >= a.warmup:
                for k in keys:
                    runs[k].append(t[k])
            info = dict(n_records=chunk.n, host_image_bytes=int(len(chunk.host)), reads_wanted=packed["reads_uploaded"], bytes_upload_packed=packed["bytes_uploaded"],
                        bytes_upload_whole=whole["bytes_uploaded"], n_ins_rows_cigar=int(sig["n_sig_ins"]), bytes_ins_cigar=gi["bytes_gathered"],
                        n_seq_rows_task=res["n_seq_rows"], n_seq_bytes_task=res["n_seq_bytes"], bytes_seq_pool_get=sum(len(x) for x in got))
        rebuild.pool_reset(ctx)
    out = dict(input=dict(reads=a.reads, seed=a.seed, reps=a.reps, warmup=a.warmup), **info, **{k: spread(v) for k, v in runs.items()})
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def rebuild_cases(ctx):
    """the rebuild_order cases as pool rows with their INS sequences put beside them: (ms ties='seqs', ms tie_callback), summed over the cases"""
    from helpers import load_json
    from seq_pool_helpers import rebuild_case_pool
    ms_seqs = ms_cb = 0.0
    for case in load_json("rebuild_order.json.gz"):
        _, ident, major, nodedup, seqs, halves = rebuild_case_pool(ctx, case)
        _, ms = timed(lambda: rebuild.rebuild_pool(ctx, ident, major, nodedup, ties="seqs"))
        ms_seqs += ms
        cb = rebuild.tie_callback(seqs.__getitem__, halves.__getitem__)
        _, ms = timed(lambda: rebuild.rebuild_pool(ctx, ident, major, nodedup, tie_order=cb))
        ms_cb += ms
    return ms_seqs, ms_cb


if __name__ == "__main__":
    main()
