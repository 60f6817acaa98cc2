"""What the record text costs on the device and on the host, alone and as the chain to out.vcf.gz.

    python scripts/emit_stage.py [--reads 4000] [--scale 1.0] [--reps 7] [--warmup 2] [--threads 16] [--no-genome] [--out profiles/vcf_emit_device.json]

One process per run, one context.  Two inputs:
  contig   the contig of scripts/bam_stage.py through call.call_bam with report_readid: the strings come from the
           kept rebuild.  Baseline, per pass: the route as it was before the device emitter - the two gathers (csv_seq_alt_gather,
           csv_name_support_join: blobs down), the host emitter, then bgzf.compress(route="device") + tabix_vcf, and the same with
           route="host" at level 6 on --threads threads.  Device chain: emit_records(route="device", from_pool, keep=header) +
           bgzf.compress_kept + bgzf.tabix_rows.  Also call_bam's wall with emit="host" and emit="device".
  genome   bench.py's cfg3 (synth.ont30 at --scale) clustered once: its call count, DEL REF from a synthetic reference of the contigs'
           lengths (a 1 MiB block of random bases, tiled), INS ALT as the store gives it.  The same two chains, the strings as host blobs.
Per stage: wall milliseconds and the kernels' event time; the bytes that cross the link each way; the text rate of k_vcf_write's phase.
Median of --reps passes after --warmup, with [min, max].  The texts, the images after inflation and the indexes are compared once."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

from cutesv_amd import bam, bgzf, call, engine, rebuild, synth, vcf             # noqa: E402
from cutesv_amd.columns import Params                                           # noqa: E402

CONTIG_LEN = 250_000_000


def stat(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def chains(ctx, header, host_emit, device_emit, reps, warmup, threads):
    """host_emit() -> body bytes (the route as it was); device_emit(tm) -> KeptText.  -> the entry of one input"""
    keys = ("ms_host_emit", "ms_host_compress_device", "ms_host_tabix", "ms_host_chain_device", "ms_host_compress_zlib", "ms_host_chain_zlib",
            "ms_device_emit", "ms_device_emit_kernels", "ms_device_compress", "ms_device_compress_kernels", "ms_device_tabix", "ms_device_chain")
    runs = {k: [] for k in keys}
    info = {}
    for it in range(warmup + reps):
        t = {}
        c0 = time.perf_counter()
        body = host_emit(t)
        c1 = time.perf_counter()
        text = header + body
        image, table = bgzf.compress(text, ctx=ctx, route="device")
        c2 = time.perf_counter()
        tbi = bgzf.tabix_vcf(text, table)
        c3 = time.perf_counter()
        zimage, ztable = bgzf.compress(text, route="host", level=6, threads=threads)
        c4 = time.perf_counter()
        t.update(ms_host_emit=(c1 - c0) * 1e3, ms_host_compress_device=(c2 - c1) * 1e3, ms_host_tabix=(c3 - c2) * 1e3, ms_host_chain_device=(c3 - c0) * 1e3,
                 ms_host_compress_zlib=(c4 - c3) * 1e3, ms_host_chain_zlib=(c4 - c3 + c1 - c0 + c3 - c2) * 1e3)
        tm = {}
        d0 = time.perf_counter()
        kept = device_emit(tm)
        d1 = time.perf_counter()
        dimage, dtable = bgzf.compress_kept(ctx, kept, timings=tm)
        d2 = time.perf_counter()
        dtbi = bgzf.tabix_rows(kept, dtable)
        d3 = time.perf_counter()
        t.update(ms_device_emit=(d1 - d0) * 1e3, ms_device_emit_kernels=tm["ms_emit_kernels"], ms_device_compress=(d2 - d1) * 1e3, ms_device_compress_kernels=tm["ms_bgzf_kernels"],
                 ms_device_tabix=(d3 - d2) * 1e3, ms_device_chain=(d3 - d0) * 1e3)
        if it == 0:
            assert kept.fetch() == text and dimage == image and bgzf.decompress(dtbi) == bgzf.decompress(tbi) and bgzf.decompress(zimage) == text
            info = dict(text_bytes=len(text), records=kept.n_records, image_bytes=len(image), rows_bytes=int(kept.rows.nbytes), tbi_bytes=len(tbi))
        if it >= warmup:
            for k in keys:
                runs[k].append(t[k])
    out = dict(info, **{k: stat(v) for k, v in runs.items()})
    out["k_vcf_write_gb_per_s"] = info["text_bytes"] / (out["ms_device_emit_kernels"]["median"] * 1e-3) / 1e9
    best = min(("ms_host_chain_device", "ms_host_chain_zlib"), key=lambda k: out[k]["median"])
    out["best_host_chain"] = best
    out["device_chain_below_best_host_chain_outside_spreads"] = out["ms_device_chain"]["max"] < out[best]["min"]
    return out


def contig_input(ctx, a, work):
    import bam_writer
    from bam_stage import CHROMS, make_records
    path = os.path.join(work, "stage.bam")
    recs = make_records(a.reads, a.seed)
    bam_writer.write_bam(path, [(c, CONTIG_LEN) for c in CHROMS],
                         [dict(d, seq=synth.pseudo_sequence(d["seq_len"], d["seq_key"]), refid=3, tags=[tuple(t) for t in d["tags"]]) for d in recs], level=1)
    rng = np.random.default_rng(a.seed)
    reference = {"7": np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 160_000_000, dtype=np.uint8)].tobytes()}
    os.environ["CUTESV_AMD_TRA_GT"] = "off"
    cp = call.CallParams(Params.ont(min_support=1))
    walls = dict(ms_call_bam_wall_host=[], ms_call_bam_wall_device=[])
    seen = []
    real = vcf.emit_records
    with bam.BamFile(path) as bf:
        for it in range(a.warmup + a.reps):
            for emit in ("host", "device"):
                t0 = time.perf_counter()
                body, _ = call.call_bam(bf, reference, cp, ctx=ctx, batch=CONTIG_LEN, report_readid=True, as_bytes=True, emit=emit)
                if it >= a.warmup:
                    walls["ms_call_bam_wall_" + emit].append((time.perf_counter() - t0) * 1e3)
                seen.append(body)
        assert len(set(seen)) == 1
        vcf.emit_records = lambda *x, **k: (seen.append((x, k)), real(*x, **k))[1]
        try:
            call.call_bam(bf, reference, cp, ctx=ctx, batch=CONTIG_LEN, report_readid=True, as_bytes=True, emit="device")      # leaves the kept rebuild on ctx
        finally:
            vcf.emit_records = real
    x, k = seen[-1]
    k = dict(k, svid=None, timings=None)
    segs, res = x[1], x[2]
    t = res.trimmed()
    header = vcf.header_text([("7", CONTIG_LEN)], "NULL", sys.argv[1:]).encode()
    sizes = {}

    def host_emit(tm):
        alt = call._gather_alt(ctx, segs, res, t)
        names = rebuild.support_join(ctx, t["support_off"], t["support_sig"])
        sizes.update(alt_bytes_down=len(alt[0]), rnames_bytes_down=len(names[0]))
        return real(*x, **dict(k, route="host", ctx=None, from_pool=None, keep=None, ins_alt=alt, rnames=names, as_bytes=True))[0]

    def device_emit(tm):
        return real(*x, **dict(k, keep=header, timings=tm))[0]
    out = chains(ctx, header, host_emit, device_emit, a.reps, a.warmup, a.threads)
    out.update(sizes, reads=a.reads, **{key: stat(v) for key, v in walls.items()})
    return out


def genome_input(ctx, a):
    st = synth.ont30(seed=20260103, scale=a.scale)
    p = Params.ont()
    hb = st.host_batch(st.tasks(), p)
    res = ctx.cluster_batch(hb)
    block = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(a.seed).integers(0, 4, 1 << 20, dtype=np.uint8)]
    reference = {c: np.resize(block, int(n)).tobytes() for c, n in zip(st.chroms, st.contig_len)} if getattr(st, "contig_len", None) is not None else None
    if reference is None:
        t = res.trimmed()
        top = np.zeros(len(st.chroms), np.int64)
        np.maximum.at(top, np.asarray(hb.segments["chrom"])[t["call_seg"]], t["bp1"] + np.maximum(t["bp2"], 0) + 2)
        reference = {c: np.resize(block, int(n) + 1000).tobytes() for c, n in zip(st.chroms, top)}
    kw = dict(min_size=p.min_size, max_size=p.max_size)
    header = vcf.header_text([(c, len(reference[c])) for c in st.chroms], "NULL", sys.argv[1:]).encode()
    out = chains(ctx, header, lambda tm: vcf.emit_records(st, hb.segments, res, reference, as_bytes=True, **kw)[0],
                 lambda tm: vcf.emit_records(st, hb.segments, res, reference, route="device", ctx=ctx, keep=header, timings=tm, **kw)[0], a.reps, a.warmup, a.threads)
    out.update(calls=res.n_calls, scale=a.scale, reference_bytes=sum(len(s) for s in reference.values()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-genome", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = dict(reps=a.reps, warmup=a.warmup, host_threads=a.threads, default_emit=call.DEFAULT_EMIT)

    def save():                                               # (after every input: the second one is the large one)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
    with tempfile.TemporaryDirectory() as work, engine.Context(0) as ctx:
        result["contig"] = contig_input(ctx, a, work)
        print(json.dumps(result["contig"]), flush=True)
        save()
        if not a.no_genome:
            result["genome"] = genome_input(ctx, a)
            print(json.dumps(result["genome"]), flush=True)
            save()


if __name__ == "__main__":
    main()
