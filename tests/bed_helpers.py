"""Helpers of tests/test_include_bed.py: crafted records and region tables for the task gates
(cutesv_amd/csrc/gates.hip.h), the BAMs of the golden cases, and the BED-aware copy of call_helpers.parent_route."""
import ctypes as C

import numpy as np

from cutesv_amd import _abi, call, extract, rebuild, synth, vcf
from cutesv_amd._lib import lib
from cutesv_amd.columns import NameTable

import call_helpers

REF_LEN = {"1": 248956422, "10": 133797422, "2": 242193529, "7": 159345973, "X": 156040895}
GATE_REFS = [("7", 200000)]
# the gates of the crafted chunk: task start, min_read_len, min_mapq; B0 / B1: the region the crafted records touch
T0, MIN_LEN, MIN_MAPQ, B0, B1 = 5000, 500, 20, 20000, 30000
SA = ("SA", "7,1000,+,500S500M,60,0;")
CHUNK_SIZES = (1, 64, 65, 257, 1100)


def _rec(name, start, span, qlen=None, mapq=60, flag=0, sa=False, zero_span=False):
    """one record: `span` reference bases, query length qlen (soft clip behind the match); zero_span: no reference base at all"""
    qlen = span if qlen is None else qlen
    cigar = [(4, qlen)] if zero_span else [(0, span)] + ([(4, qlen - span)] if qlen > span else [])
    return dict(name=name, flag=flag, mapq=mapq, start=start, cigar=cigar, seq="A" * qlen, tags=[SA] if sa else [], refid=0)


def crafted_records():
    """records that sit on every equality of the gates (with T0, MIN_LEN, MIN_MAPQ and the regions of `region_tables`)"""
    r = [_rec("t_below", T0 - 1, 1000), _rec("t_at", T0, 1000),
         _rec("len_below", 6000, MIN_LEN - 1), _rec("len_at", 6000, MIN_LEN),
         _rec("mq_below", 7000, 1000, mapq=MIN_MAPQ - 1, sa=True), _rec("mq_at", 7000, 1000, mapq=MIN_MAPQ, sa=True),
         _rec("short_lowmq", 7500, MIN_LEN - 1, mapq=MIN_MAPQ - 1)]
    for k, (flag, sa) in enumerate([(256, False), (272, True), (0, False), (0, True), (16, False), (16, True), (2048, False), (2064, True), (4, True), (1, False)]):
        r.append(_rec("cls%02d" % k, 8000 + 10 * k, 1000, flag=flag, sa=sa))
    r += [_rec("end_at_b0", B0 - 1000, 1000, sa=True), _rec("end_b0_plus1", B0 - 1000, 1001, sa=True),
          _rec("start_b1_minus1", B1 - 1, 1000), _rec("start_at_b1", B1, 1000),
          _rec("seam_zero", B1, 0, qlen=600, zero_span=True), _rec("seam_zero_sa", B1, 0, qlen=600, zero_span=True, sa=True),
          _rec("inside", 25000, 1000, sa=True), _rec("zero_inside", 25000, 0, qlen=700, zero_span=True),
          _rec("behind_short", 50000, 1000, sa=True),           # inside (40000, 60000), behind (41000, 42000): the prefix maximum
          _rec("far", 150000, 1000)]
    return r


def gate_records(n, seed=11):
    """n records in coordinate order: the crafted ones first to go in, random ones to fill up"""
    rng = np.random.default_rng(seed)
    recs = crafted_records()[:n]
    for k in range(n - len(recs)):
        span = int(rng.integers(1, 3000))
        zero = rng.random() < 0.05
        recs.append(_rec("rnd%05d" % k, int(rng.integers(0, 100000)), span, qlen=span + int(rng.integers(0, 400)) if not zero else int(rng.integers(1, 900)),
                         mapq=int(rng.choice([0, 19, 20, 21, 60])), flag=int(rng.choice([0, 0, 16, 256, 272, 2048, 4])), sa=rng.random() < 0.4, zero_span=zero))
    recs.sort(key=lambda d: d["start"])
    return recs


def random_regions(rng, n, lo=-2000, hi=110000):
    """n regions sorted by (start, end): short and long, some with end < start"""
    beg = rng.integers(lo, hi, n)
    length = np.where(rng.random(n) < 0.1, rng.integers(-500, 0, n), np.where(rng.random(n) < 0.2, rng.integers(1, 30000, n), rng.integers(1, 800, n)))
    r = np.stack([beg, beg + length], 1).astype(np.int64)
    return r[np.lexsort((r[:, 1], r[:, 0]))]


def region_tables():
    rng = np.random.default_rng(12)
    return [("none", None), ("empty", np.zeros((0, 2), np.int64)), ("one", [(B0, B1)]), ("nested", [(40000, 60000), (41000, 42000)]),
            ("three_touching", [(B0, B1), (B1, B1 + 1000), (40000, 60000)]), ("thousand", random_regions(rng, 1000)), ("1025", random_regions(rng, 1025)),
            ("negative", [(-5000, -100), (-500, T0 + 1), (-1, 6500)]), ("equal_starts", [(B0, B0 + 1000), (B0, B0 + 500), (B0, B1), (B0, B0)]),
            ("end_before_beg", [(B1, B0), (25500, 19500), (26000, 25000)])]


def raw_task_gates(ctx, n, task_start, min_read_len, min_mapq, flags, n_regions, beg, end, bits=None):
    """csv_bam_task_gates as it is: -> the status"""
    return lib().csv_bam_task_gates(ctx._h if ctx is not None else None, n, task_start, min_read_len, min_mapq, flags, n_regions,
                                    None if beg is None else beg.ctypes.data, None if end is None else end.ctypes.data, None if bits is None else bits.ctypes.data, None)


def golden_records(case, chrom, lengths=None):
    """the records of a single_pipe / include_bed case as bam_writer takes them (+ the refs of the header)"""
    lengths = dict(REF_LEN, **(lengths or {}))
    refs = [(c, lengths[c]) for c in case["chroms"]]
    refid = case["chroms"].index(chrom)
    recs = [dict(d, seq=synth.pseudo_sequence(d["seq_len"], d["seq_key"]), refid=refid, tags=[tuple(t) for t in d["tags"]]) for d in case["reads"]]
    return refs, recs


def pipe_args(p):
    return (p["sv"], p["min_mapq"], p["parts"], p["min_read_len"], p["min_siglength"], p["md"], p["mi"], p["max_size"])


def pool_image(ctx, n_seg, n_reads, ins_segs):
    """what a task left in the pools: the row count, the rebuilt rows with their pool row numbers (read index = rank, as in
    test_bam_split), the sequence pool's counts, every row's x.5 flag and the bases of the rebuilt INS rows"""
    n = rebuild.pool_rows(ctx)
    zeros = np.zeros(n_seg, np.uint8)
    r = rebuild.rebuild_pool(ctx, np.arange(n_reads, dtype=np.int32), zeros, zeros, keep_on_device=False)
    out = {k: r[k].tolist() for k in ("seg_id", "a", "b", "read_id", "aux", "src_row", "seg_count")}
    out["n"], out["seq_rows"] = n, rebuild.seq_pool_rows(ctx)
    out["half"] = rebuild.seq_pool_half(ctx, np.arange(n)).tolist()
    out["seqs"] = rebuild.seq_pool_get(ctx, r["src_row"][np.isin(r["seg_id"], ins_segs)]) if out["seq_rows"][0] else []
    return out


def bed_route(ctx, bf, reference, params, regions, batch=10_000_000, report_readid=False):
    """call_helpers.parent_route with a BED: single_pipe_bam with host gates per task, each with regions.for_task -> VCF body text"""
    import dataclasses
    cp = params
    p = dataclasses.replace(cp.resolve, genotype_tra=(call.tra_gt_mode(cp.resolve.genotype) == "reads_table"))
    chroms = sorted(bf.references)
    crank = {c: i for i, c in enumerate(chroms)}
    length = dict(zip(bf.references, bf.lengths))
    cands, reads_info = [], []
    for c in chroms:
        for s, e in call.cut_tasks(length[c], batch):
            cand, ri = extract.single_pipe_bam(ctx, bf, c, s, e, crank, *cp.pipe_args(), bed_regions=regions.for_task(c, s, e), gates="host")
            cands.append(cand); reads_info.extend(ri)
    cols, reads, uniq = call_helpers.per_type_columns(cands, reads_info if p.genotype else [], chroms)
    st, _ = rebuild.store_from_unsorted(ctx, chroms, cols, names=NameTable(uniq), reads=reads)
    if p.genotype_tra:
        st.contig_len = np.array([length[c] for c in chroms], np.int64)
    tasks = st.tasks()
    hb = st.host_batch(tasks, p)
    res = ctx.cluster_batch(hb)
    text, _ = vcf.emit_records(st, hb.segments, res, reference, min_size=p.min_size, max_size=p.max_size, genotype=p.genotype, report_readid=report_readid)
    return text


def cigar_in_out(n, flags, use=None):
    """a csv_cigar_in / csv_cigar_out pair for a call that is expected to be refused"""
    cin = _abi.CigarIn(n_reads=n, flags=flags, use=None if use is None else use.ctypes.data, min_siglength=10, merge_ins_threshold=100, merge_del_threshold=0)
    return cin, _abi.CigarOut()


def sa_in_out(n, flags, sel=None):
    off = np.zeros(1, np.int64)
    sin = _abi.SaIn(n_records=n, sel=None if sel is None else sel.ctypes.data, flags=flags, min_mapq=20, task_rank=0, n_names=0, name_off=off.ctypes.data)
    return sin, _abi.SaOut(), off


def byref(x):
    return C.byref(x)
