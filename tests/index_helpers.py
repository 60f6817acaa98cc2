"""Shared by tests/test_bam_index.py and tests/test_index_calls.py: a three-contig BAM written with small blocks for the index
parser and the read grid, the planted BAM of call_helpers rewritten with small blocks, both indexed by bai_writer, and the
comparison of two chunks."""
import numpy as np

import bai_writer
import bam_writer

REFS = [("one", 2_000_000), ("none", 500_000), ("two", 1_000_000)]
BLOCK_BYTES = 700
WINDOW = 16384
LONG = ((1000, 600_000), (200_100, 140_000), (300_050, 20_000))           # (start, reference span) of the long records of "one"


def _seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def grid_records(seed=11):
    """about 400 short records on two contigs (with empty windows between their groups), three long records that start two or more
    windows in front of what lies under them, a placed unmapped record, and an unmapped tail - in coordinate order"""
    rng = np.random.default_rng(seed)
    recs = []

    def add(name, refid, start, cigar, flag=0):
        qlen = sum(n for op, n in cigar if op in (0, 1, 4))
        recs.append(dict(name=name, flag=flag, mapq=60, start=start, cigar=cigar, seq=_seq(rng, qlen), refid=refid))
    for k, (start, span) in enumerate(LONG):
        add("long%d" % k, 0, start, [(0, 60), (3, span - 120), (0, 60)])
    # groups of short records; windows 3, 6 - 11 and everything behind 45 hold no record START
    for g, base in enumerate((5, 16384 - 40, 2 * 16384 - 3, 4 * 16384 + 7, 12 * 16384 - 90, 20 * 16384, 30 * 16384 + 5000, 44 * 16384 + 16000)):
        for k in range(25):
            add("s%d_%02d" % (g, k), 0, base + 37 * k + int(rng.integers(0, 5)), [(0, 40 + int(rng.integers(0, 60)))], flag=16 if k % 3 == 0 else 0)
    add("placed_unmapped", 0, 20 * 16384 + 500, [], flag=4)
    recs[-1]["seq"] = _seq(rng, 50)
    add("long_two", 2, 16384 + 9, [(0, 50), (2, 140_000 - 100), (0, 50)])
    for g, base in enumerate((0, 16383, 3 * 16384 + 1, 5 * 16384 - 1, 9 * 16384, 12 * 16384 + 12, 20 * 16384 + 8000, 40 * 16384)):
        for k in range(25):
            add("t%d_%02d" % (g, k), 2, base + 29 * k + int(rng.integers(0, 5)), [(0, 30 + int(rng.integers(0, 80)))])
    recs.sort(key=lambda r: (r["refid"], r["start"]))
    for k in range(5):
        recs.append(dict(name="tail%d" % k, flag=4, mapq=0, start=-1, cigar=[], seq=_seq(rng, 60), refid=-1))
    return recs


def write_grid_bam(path, **bai):
    """the grid BAM with blocks of about BLOCK_BYTES bytes - records straddle them freely, and three records are made to start
    exactly on a block boundary - and its index -> (records, bai_writer's info)"""
    recs = grid_records()
    info = bam_writer.write_bam(str(path), REFS, recs, block_bytes=BLOCK_BYTES)
    on_boundary = [info["records"][k]["offset"] for k in (40, 150, 333)]
    info = bam_writer.write_bam(str(path), REFS, recs, block_bytes=BLOCK_BYTES, cuts=on_boundary)
    assert info["n_blocks"] >= 50
    return recs, bai_writer.write_bai(str(path), **bai)


def write_planted_small_blocks(path, extra=(), contigs=None, block_bytes=BLOCK_BYTES, **bai):
    """call_helpers' planted two-contig BAM with small blocks (+ `extra` records, merged in coordinate order) and its index -> reference"""
    import call_helpers
    recs, ref = call_helpers.planted_records()
    recs = sorted(list(recs) + list(extra), key=lambda r: (r["refid"], r["start"]))
    bam_writer.write_bam(str(path), contigs or call_helpers.CONTIGS, recs, block_bytes=block_bytes)
    bai_writer.write_bai(str(path), **bai)
    return ref


def same_chunk(a, b):
    """two Chunks hold the same records in the same order with the same two images"""
    return (a.n == b.n and a.more == b.more and np.array_equal(a.slim, b.slim) and np.array_equal(a.rec_off, b.rec_off) and np.array_equal(a.rec_len, b.rec_len)
            and np.array_equal(a.host, b.host) and np.array_equal(a.host_off, b.host_off))


def grid_points(n_intv, length):
    """region bounds worth trying: around every 16 384 boundary that matters, 0, inside empty windows, behind the last record, behind
    n_intv, and the contig's end"""
    pts = {0, 1, length, length + 5, (n_intv + 3) * WINDOW, n_intv * WINDOW}
    for k in (1, 2, 3, 4, 5, 6, 9, 12, 13, 20, 21, 30, 37, 38, 40, 44, 45, 46):
        pts.update((k * WINDOW - 1, k * WINDOW, k * WINDOW + 1))
    pts.update((3 * WINDOW + 8000, 7 * WINDOW + 100, 10 * WINDOW + 5, 46 * WINDOW + 77))          # inside windows where nothing starts
    return sorted(p for p in pts if p >= 0)


def store_route(ctx, bf, reference, params, regions, tasks, report_readid=False):
    """bed_helpers.bed_route driven by a given task list [(contig, t0, t1)] whose bounds may be fractional: single_pipe_bam with host
    gates per task - a task owns the records that start in [ceil(t0), ceil(t1)) and gets regions.for_task on the bounds as they
    are - then store_from_unsorted, cluster_batch, emit_records -> VCF body text"""
    import dataclasses
    import math
    import call_helpers
    from cutesv_amd import call, extract, rebuild, vcf
    from cutesv_amd.columns import NameTable
    cp = params
    p = dataclasses.replace(cp.resolve, genotype_tra=(call.tra_gt_mode(cp.resolve.genotype) == "reads_table"))
    chroms = sorted(bf.references)
    crank = {c: i for i, c in enumerate(chroms)}
    length = dict(zip(bf.references, bf.lengths))
    cands, reads_info = [], []
    for c in chroms:
        for name, s, e in tasks:
            if name != c:
                continue
            cand, ri = extract.single_pipe_bam(ctx, bf, c, math.ceil(s), math.ceil(e), crank, *cp.pipe_args(),
                                               bed_regions=None if regions is None else regions.for_task(c, s, e), gates="host")
            cands.append(cand); reads_info.extend(ri)
    cols, reads, uniq = call_helpers.per_type_columns(cands, reads_info if p.genotype else [], chroms)
    st, _ = rebuild.store_from_unsorted(ctx, chroms, cols, names=NameTable(uniq), reads=reads)
    if p.genotype_tra:
        st.contig_len = np.array([length[c] for c in chroms], np.int64)
    hb = st.host_batch(st.tasks(), p)
    res = ctx.cluster_batch(hb)
    text, _ = vcf.emit_records(st, hb.segments, res, reference, min_size=p.min_size, max_size=p.max_size, genotype=p.genotype, report_readid=report_readid)
    return text


def grid_pairs(points, length):
    """the (beg, end) pairs of the read grid: every point with the next one, the fourth one on, the contig's end and no end at all"""
    for i, beg in enumerate(points):
        for end in sorted({points[min(i + 1, len(points) - 1)], points[min(i + 4, len(points) - 1)], length, 1 << 62}):
            if end > beg:
                yield beg, end
