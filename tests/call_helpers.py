"""Shared by tests/test_call_bam.py and scripts/call_stage.py: a small planted BAM for `call.call_bam`, and the route the same
file took before that entry existed - single_pipe_bam per task, store_from_unsorted with names, sequences and x.5 flags,
cluster_batch, emit_records - every link of which is pinned to the reference's goldens by the other test files."""
import numpy as np

from cutesv_amd import call, extract, rebuild, vcf
from cutesv_amd.columns import BND_CODE, NameTable, TYPES, intern_names

CONTIGS = [("chrB", 30000), ("chrA", 40000)]                      # (header order is not name order: indices and ranks differ)


def _bases(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def planted_records(seed=5):
    """-> (records for bam_writer.write_bam in coordinate order, {contig: reference sequence}).  What is planted:
    an INS of 300 bases at chrA:10000 in the CIGARs of 12 reads, joined by one reverse-strand split read whose candidate sits at
    10000.5; a second INS locus (chrA:20000, 150 bases) where two records of one name carry different bases (a tie group), two
    records of another name carry the same bases (a duplicate) and three more reads make up the support; a 200-base DEL at
    chrA:30000 in 12 reads; a DUP (chrA:16500-17000) and a TRA (chrA:25000 -> chrB:12000) in the SA tags of 4 reads each."""
    rng = np.random.default_rng(seed)
    ref = {c: _bases(rng, n) for c, n in CONTIGS}
    refid = {c: i for i, (c, _) in enumerate(CONTIGS)}
    recs = []

    def add(name, chrom, start, cigar, flag=0, tags=(), seq=None):
        qlen = sum(n for op, n in cigar if op in (0, 1, 4))
        recs.append(dict(name=name, flag=flag, mapq=60, start=start, cigar=cigar, seq=seq or _bases(rng, qlen), tags=list(tags), refid=refid[chrom]))

    def with_insert(left, ins, right):
        return _bases(rng, left) + ins + _bases(rng, right)
    ins300 = _bases(rng, 300)
    for k in range(12):                                              # INS 300 at chrA:10000; odd read lengths among them
        left = 1500 + 101 * k
        add("ins%02d" % k, "chrA", 10000 - left, [(0, left), (1, 300), (0, 2500 + k)], seq=with_insert(left, ins300, 2500 + k))
    # ... and one reverse-strand split read: 2000M2301S on the reference strand, the rest 1 base further on
    add("split_rev", "chrA", 8000, [(0, 2000), (4, 2301)], flag=16, tags=[("SA", "chrA,10002,-,2300S2001M,60,0;")])
    # the second INS locus: 150 bases at chrA:20000
    a150, b150, c150 = _bases(rng, 150), _bases(rng, 150), _bases(rng, 150)
    for name, left, ins in (("tieA", 1800, b150), ("tieA", 1800, a150), ("tieB", 1700, c150), ("tieB", 1700, c150), ("tieC", 1600, a150), ("tieD", 1500, a150),
                            ("tieE", 1400, b150)):
        add(name, "chrA", 20000 - left, [(0, left), (1, 150), (0, 2200)], seq=with_insert(left, ins, 2200))
    for k in range(12):                                              # DEL 200 at chrA:30000
        left = 1400 + 97 * k
        add("del%02d" % k, "chrA", 30000 - left, [(0, left), (2, 200), (0, 2600)])
    for k in range(4):                                               # DUP chrA:16500-17000 (split reads, forward strand)
        m = 2000 + 100 * k
        add("dup%d" % k, "chrA", 17000 - m, [(0, m), (4, 2000)], tags=[("SA", "chrA,16501,+,%dS2000M,60,0;" % m)])
    for k in range(4):                                               # TRA chrA:25000 -> chrB:12000
        m = 2100 + 100 * k
        add("tra%d" % k, "chrA", 25000 - m, [(0, m), (4, 2000)], tags=[("SA", "chrB,12001,+,%dS2000M,60,0;" % m)])
    for k in range(8):                                               # plain coverage on chrB
        add("cov%d" % k, "chrB", 9000 + 700 * k, [(0, 3000 + 13 * k)])
    recs.sort(key=lambda r: (r["refid"], r["start"]))
    return recs, ref


def write_planted_bam(path, seed=5):
    import bam_writer
    recs, ref = planted_records(seed)
    bam_writer.write_bam(path, CONTIGS, recs)
    return ref


def per_type_columns(cands, reads_info, chroms):
    """the candidate tuples of the tasks (dicts as single_pipe_bam returns them, in task order) and their reads-table rows ->
    (per_type columns for store_from_unsorted, reads dict or None, sorted unique names)"""
    cidx = {c: i for i, c in enumerate(chroms)}
    per = {t: [x for cand in cands for x in cand[t]] for t in TYPES}
    npos = {"DEL": 2, "INS": 2, "DUP": 2, "INV": 3, "TRA": 4}
    uniq, _ = intern_names([x[npos[t]] for t in per for x in per[t]] + [r[3] for r in reads_info])
    rank = {n: i for i, n in enumerate(uniq)}
    strands = ("++", "--")
    cols = {}
    for t, lst in per.items():
        d = dict(chrom=[cidx[x[-1]] for x in lst], read_id=[rank[x[npos[t]]] for x in lst])
        if t in ("DEL", "DUP"):
            d.update(a=[int(x[0]) for x in lst], b=[int(x[1]) for x in lst], aux=[0] * len(lst))
        elif t == "INS":
            d.update(a=[int(x[0]) for x in lst], b=[int(x[1]) for x in lst], aux=[len(x[3]) for x in lst], seq=[x[3] for x in lst], half=[int(x[0] != int(x[0])) for x in lst])
        elif t == "INV":
            d.update(a=[int(x[1]) for x in lst], b=[int(x[2]) for x in lst], aux=[strands.index(x[0]) for x in lst])
        else:
            d.update(a=[int(x[1]) for x in lst], b=[int(x[3]) for x in lst], aux=[cidx[x[2]] * 8 + BND_CODE[x[0]] for x in lst])
        cols[t] = d
    reads = None
    if reads_info:
        reads = dict(chrom=[cidx[r[4]] for r in reads_info], start=[r[0] for r in reads_info], end=[r[1] for r in reads_info], primary=[r[2] for r in reads_info],
                     read_id=[rank[r[3]] for r in reads_info])
    return cols, reads, uniq


def parent_route(ctx, bf, reference, params, batch=10_000_000, report_readid=False, timings=None):
    """the same file without call_bam: -> VCF body text.  params: a call.CallParams."""
    import dataclasses
    import time
    t0 = time.perf_counter()
    cp = params
    p = dataclasses.replace(cp.resolve, genotype_tra=(call.tra_gt_mode(cp.resolve.genotype) == "reads_table"))
    chroms = sorted(bf.references)
    crank = {c: i for i, c in enumerate(chroms)}
    length = dict(zip(bf.references, bf.lengths))
    cands, reads_info = [], []
    for c in chroms:
        for s, e in call.cut_tasks(length[c], batch):
            cand, ri = extract.single_pipe_bam(ctx, bf, c, s, e, crank, *cp.pipe_args())
            cands.append(cand); reads_info.extend(ri)
    t1 = time.perf_counter()
    cols, reads, uniq = per_type_columns(cands, reads_info if p.genotype else [], chroms)
    st, _ = rebuild.store_from_unsorted(ctx, chroms, cols, names=NameTable(uniq), reads=reads)
    if p.genotype_tra:
        st.contig_len = np.array([length[c] for c in chroms], np.int64)
    t2 = time.perf_counter()
    tasks = st.tasks()
    hb = st.host_batch(tasks, p)
    res = ctx.cluster_batch(hb)
    t3 = time.perf_counter()
    text, _ = vcf.emit_records(st, hb.segments, res, reference, min_size=p.min_size, max_size=p.max_size, genotype=p.genotype, report_readid=report_readid)
    t4 = time.perf_counter()
    if timings is not None:
        timings.update(ms_tasks=(t1 - t0) * 1e3, ms_rebuild=(t2 - t1) * 1e3, ms_cluster=(t3 - t2) * 1e3, ms_emit=(t4 - t3) * 1e3)
    return text
