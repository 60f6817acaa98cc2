"""What TRA genotyping from every alignment costs, on the input of scripts/bam_stage.py (DESIGN.md section
13: one synthetic contig of long reads) with planted TRA calls: at each of --loci breakpoints on "7" six split reads whose SA tag
points to "2", and around the breakpoint what the reads table never sees - secondary and supplementary records and MAPQ-0
primaries that span it.

    python scripts/tra_aln_stage.py [--reads N] [--loci K] [--reps R] [--warmup W] [--out profiles/tra_alignments.json]

Per pass, in one process and on one context:
  append      aln.append_decoded of the contig's one task after its decode: HIP events (aln.timing) and wall
  genotype    aln.tra_genotype of the planted calls in plain-id mode over the table the task made: HIP events and wall
  ms_tra_gt   the same step inside call.call_bam(tra_gt="alignments") (rank mode, on the calls the engine found), and the call's wall
  host twin   aln.tra_genotype_host over the same table and calls: what the kernel replaces (tra_bam.window_status per window)
The kernel's answer must equal the twin's.  Medians over --reps passes after --warmup passes, with min and max."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

from cutesv_amd import aln, bam, call, engine, rebuild, synth      # noqa: E402
from cutesv_amd.columns import Params                               # noqa: E402
from bam_stage import CHROMS, make_records, spread                  # noqa: E402

CONTIG_LEN = 250_000_000
BIAS, GT_ROUND = 50, 500                                            # Params.ont: max_cluster_bias_TRA, gt_round


def planted(n_loci, seed):
    """-> (records, [(pos on "7", pos on "2", names of the six supports)])"""
    rng = np.random.default_rng(seed)
    recs, loci = [], []
    k = 0

    def add(name, start, cigar, flag, mapq, tags=()):
        nonlocal k
        qlen = sum(n for op, n in cigar if op in (0, 1, 4))
        recs.append(dict(name=name, flag=flag, mapq=mapq, start=start, cigar=cigar, seq_len=qlen, seq_key=seed * 7000003 + k, tags=[list(t) for t in tags]))
        k += 1
    for j in range(n_loci):
        p, q = 1_000_000 + j * (140_000_000 // n_loci), 5_000_000 + 1000 * j
        names = []
        for i in range(6):
            m = 2100 + 100 * i
            names.append("tra%04d_%d" % (j, i))
            add(names[-1], p - m, [(0, m), (4, 2000)], 0, 60, [("SA", "2,%d,+,%dS2000M,60,0;" % (q + 1, m))])
        for i in range(12):
            add("mq0_%04d_%d" % (j, i), p - 3000 + 37 * i, [(0, 6000)], 0 if i % 2 else 16, 0)
        for i in range(24):
            add("sec%04d_%d" % (j, i), p - 1500 + 97 * i, [(0, 1800)], (256, 272, 2048, 2064)[i % 4], 60)
        loci.append((p, q, names))
    return recs, loci


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--loci", type=int, default=200)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bam_writer
    path = os.path.join(__import__("tempfile").mkdtemp(), "stage.bam")
    extra, loci = planted(a.loci, a.seed)
    recs = sorted(make_records(a.reads, a.seed) + extra, key=lambda d: d["start"])
    bam_writer.write_bam(path, [(c, CONTIG_LEN) for c in CHROMS],
                         [dict(d, seq=synth.pseudo_sequence(d["seq_len"], d["seq_key"]), refid=3, tags=[tuple(t) for t in d["tags"]]) for d in recs], level=1)
    rng = np.random.default_rng(a.seed)
    reference = {"7": np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 160_000_000, dtype=np.uint8)].tobytes()}
    cp = call.CallParams(Params.ont(min_support=3, genotype=True))
    assert (cp.resolve.max_cluster_bias_TRA, cp.resolve.gt_round) == (BIAS, GT_ROUND)
    crank = {c: i for i, c in enumerate(CHROMS)}
    lens = [CONTIG_LEN] * len(CHROMS)
    keys = ("ms_append_device", "ms_append_wall", "ms_genotype_device", "ms_genotype_wall", "ms_host_twin", "ms_call_bam_wall", "ms_tra_gt", "ms_call_bam_reads_table_wall")
    runs = {k: [] for k in keys}
    info = {}
    with engine.Context(0) as ctx, bam.BamFile(path) as bf:
        for it in range(a.warmup + a.reps):
            t = {}
            # call_bam in both modes (the pools and the table are reset inside)
            tm = {}
            t0 = time.perf_counter()
            text, svid = call.call_bam(bf, reference, cp, ctx=ctx, batch=CONTIG_LEN, tra_gt="alignments", timings=tm)
            t["ms_call_bam_wall"] = (time.perf_counter() - t0) * 1e3
            t["ms_tra_gt"] = tm["ms_tra_gt"]
            t0 = time.perf_counter()
            text_rt, _ = call.call_bam(bf, reference, cp, ctx=ctx, batch=CONTIG_LEN, tra_gt="reads_table")
            t["ms_call_bam_reads_table_wall"] = (time.perf_counter() - t0) * 1e3
            # the append alone: the contig's chunk decoded, its names appended, then the table
            rebuild.name_pool_reset(ctx); aln.reset(ctx, len(CHROMS))
            chunk = bf.records("7", 0, CONTIG_LEN)
            bam.decode(ctx, chunk, host_outputs=False)
            base = rebuild.name_pool_append_chunk(ctx, chunk)
            t0 = time.perf_counter()
            n_rows = aln.append_decoded(ctx, crank["7"], 0, CONTIG_LEN, base)
            t["ms_append_wall"] = (time.perf_counter() - t0) * 1e3
            t["ms_append_device"] = aln.timing(ctx)[0]
            # the planted calls in plain-id mode: supports = the table ids of the planted names
            rows = aln.get(ctx)
            id_of = {n: int(i) for n, i in zip(rebuild.name_pool_get(ctx, rows["id"]), rows["id"])}
            calls = dict(chrom1=[crank["7"]] * len(loci), pos1=[p for p, _, _ in loci], chrom2=[crank["2"]] * len(loci), pos2=[q for _, q, _ in loci],
                         support_off=np.arange(len(loci) + 1) * 6, support=np.array([id_of[n] for _, _, names in loci for n in names], np.int64))
            t0 = time.perf_counter()
            dr, status = aln.tra_genotype(ctx, contig_len=lens, bias=BIAS, gt_round=GT_ROUND, **calls)
            t["ms_genotype_wall"] = (time.perf_counter() - t0) * 1e3
            t["ms_genotype_device"] = aln.timing(ctx)[1]
            off, maxlen = aln.layout(ctx, len(CHROMS))
            table = aln.Table(off, rows["start"], rows["end"], rows["primary"], rows["id"])
            t0 = time.perf_counter()
            hdr, hstatus = aln.tra_genotype_host(table, contig_len=lens, bias=BIAS, gt_round=GT_ROUND, **calls)
            t["ms_host_twin"] = (time.perf_counter() - t0) * 1e3
            assert dr.tolist() == hdr.tolist() and status.tolist() == hstatus.tolist(), "the kernel and the host twin disagree"
            if it >= a.warmup:
                for k in keys:
                    runs[k].append(t[k])
            bnd = [ln.split("\t")[9] for ln in text.splitlines() if "SVTYPE=BND" in ln]
            bnd_rt = [ln.split("\t")[9] for ln in text_rt.splitlines() if "SVTYPE=BND" in ln]
            info = dict(n_table_rows=n_rows, maxlen=int(maxlen[crank["7"]]), n_calls_planted=len(loci), n_bnd_records=len(bnd),
                        n_bnd_genotypes_that_differ_from_reads_table=sum(x != y for x, y in zip(bnd, bnd_rt)), dr_median=float(np.median(dr)),
                        status_counts={str(s): int((status == s).sum()) for s in (0, 1, -1)}, n_records_text=text.count("\n"))
    out = dict(input=dict(reads=a.reads, loci=a.loci, seed=a.seed, reps=a.reps, warmup=a.warmup, bias=BIAS, gt_round=GT_ROUND), **info, **{k: spread(v) for k, v in runs.items()})
    out["host_twin_over_genotype_wall"] = out["ms_host_twin"]["median"] / out["ms_genotype_wall"]["median"]
    out["tra_gt_share_of_call_bam"] = out["ms_tra_gt"]["median"] / out["ms_call_bam_wall"]["median"]
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
