"""BAM -> VCF body in one call: the chain the earlier stages built, connected.

    text, svid = call_bam("in.bam", fasta.Reference("ref.fa"), CallParams(Params.ont(min_support=3)))
    python -m cutesv_amd.call in.bam ref.fa -o out.body.vcf [--genotype] [--tra_gt MODE] [--report_readid] [--min_support N] [--batch B]
                               [--include_bed FILE] [--reads_table {host,device}] [--sigs_dir DIR] [--inflate {host,device}] [--frame {host,device}]

(cuteSV's own command line - BAM REF OUT.vcf WORK_DIR and its flags, a VCF with header - is cutesv_amd/cli.py: python -m cutesv_amd.)

Per task region the records are decoded, scanned and analysed on the device and their signatures, read names and inserted
bases stay there (extract.task_to_pool with the name pool and the sequence pool); one rebuild sorts and de-duplicates the pool
by read NAME with the INS tie groups settled from the sequences (rebuild.rebuild_pool_by_name, ties="seqs") and keeps the
columns on the device; csv_cluster_batch clusters them in place; the ALT bases of the INS calls and - with report_readid - the
RNAMES text are gathered on the device (rebuild.alt_gather / support_join) and handed to the native emitter as they are.
Nothing here loops in Python over records, signatures or supports: only over tasks, segments and contigs.

call_bam is that chain as a list of phases: resolve_options checks and defaults the option keywords without
touching a file or the device, _session opens or borrows the reader and the context, sets the routes and puts everything back, _Laps
keeps `timings` and `read_stats`; then _chrom_table, _task_list, _run_tasks, _rebuild, _cluster, the TRA genotyping, the two gathers, emit.

The text is the VCF BODY: the records of main script :1208-1237 in its order.  The header stays the driver's (DESIGN.md
section 11)."""
import collections
import contextlib
import dataclasses
import math
import os
import time
from dataclasses import dataclass, field

import numpy as np

from . import _abi, aln, bam as bam_mod, bed as bed_mod, engine, extract, fasta, reads as reads_mod, rebuild, vcf
from .columns import Params, TYPES, segment_record


@dataclass
class CallParams:
    """resolve's Params plus the extraction gates of single_pipe (cuteSV_Description.py defaults): what call_bam needs to know"""
    resolve: Params = field(default_factory=Params)
    min_mapq: int = 20
    max_split_parts: int = 7
    min_read_len: int = 500
    min_siglength: int = 10
    merge_del_threshold: int = 0
    merge_ins_threshold: int = 100

    def pipe_args(self):
        """the positional tail single_pipe_bam / task_to_pool take: sv_size .. max_size"""
        return (self.resolve.min_size, self.min_mapq, self.max_split_parts, self.min_read_len, self.min_siglength, self.merge_del_threshold,
                self.merge_ins_threshold, self.resolve.max_size)


def cut_tasks(length, batch):
    """the task regions of a contig of `length` bases with -b `batch`: [(start, end)] as main_ctrl cuts them - one task for a contig
    shorter than the batch, else int(length / batch) full ones and the rest.  (The reference also shrinks the batch of a contig
    that holds many reads, from the index statistics - that cut is cut_tasks_index: a matter of load balance - the calls do not
    depend on the cut, except with include_bed: a task's reads are tested against the regions of THAT task only, see bed.py.)"""
    if batch <= 0:
        raise ValueError("batch must be positive")
    if length < batch:
        return [(0, length)]
    tasks = [(k * batch, (k + 1) * batch) for k in range(length // batch)]
    if tasks[-1][1] < length:
        tasks.append((tasks[-1][1], length))
    return tasks


def cut_tasks_index(stats, lengths, batch, threads):
    """The reference's task cut from the index statistics (main_ctrl, main script :1022-1044) -> [(contig, start, end)] in the order
    of `stats`.  stats: [(contig, mapped, ...)] for every contig of the header (BamFile.index_statistics); lengths: {contig: bases};
    batch: -b; threads: -t.  A contig that holds more than total_mapped / threads / 10 mapped reads is cut into int(mapped / unit) + 1
    parts of a FRACTIONAL size, and the bounds stay the floats the reference's running sum makes them: pos can fall a rounding error
    short of the length, and the sliver task that follows is the reference's too.  Every operation below is the reference's, in
    its order, on Python numbers - nothing is simplified."""
    tasks = []
    total_mapped = 0
    for i in stats:
        total_mapped += i[1]
    mapped_unit = total_mapped / threads / 10
    for i in stats:
        local_ref_len = lengths[i[0]]
        if total_mapped == 0 or i[1] <= mapped_unit:
            batch_size = batch
        else:
            batch_size = local_ref_len / (int(i[1] / mapped_unit) + 1)
        if local_ref_len < batch_size:
            tasks.append((i[0], 0, local_ref_len))
        else:
            pos = 0
            task_round = int(local_ref_len / batch_size)
            for j in range(task_round):
                tasks.append((i[0], pos, pos + batch_size))
                pos += batch_size
            if pos < local_ref_len:
                tasks.append((i[0], pos, local_ref_len))
    return tasks


def task_bounds(t0, t1):
    """the records a task [t0, t1) owns, in integers: those that START in [ceil(t0), ceil(t1)) - Python's comparison of an int with a
    float bound (`start >= t0`, `start < t1`), which is what the reference's gate applies.  (What pysam's fetch does with a fractional
    bound cannot be observed here: see DESIGN.md section 28, open point.)"""
    return math.ceil(t0), math.ceil(t1)


def task_ranges(bf, chrom, regs, t0, t1):
    """What a task with the BED regions `regs` (bed.Regions.for_task) reads of [t0, t1) (integers): [] - nothing - for an empty list,
    else the union of the regions clipped to the task as sorted, disjoint (start, end) pairs.  A region written with end < start
    contributes its hull, one base wider.  Neighbours whose starting positions the index puts into the same or the adjacent BGZF block
    are merged: seeking between them would save no block.  A superset of what the gates pass - they still decide."""
    cut = []
    for b0, b1 in np.asarray(regs, np.int64).reshape(-1, 2).tolist():
        lo, hi = (b0, b1) if b0 <= b1 else (b1 - 1, b0 + 1)
        lo, hi = max(lo, t0), min(hi, t1)
        if lo < hi:
            cut.append((lo, hi))
    out, last = [], 0                                         # last: the block in which the range merged last starts (neighbour by neighbour,
    for lo, hi in sorted(cut):                                # so a chain of adjacent starts becomes one range)
        block = bf.index_block(chrom, lo)                     # (-1, "nothing from here on", merges as well: a superset is safe)
        if out and (lo <= out[-1][1] or block - last <= 1):
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
        last = block
    return out


DEFAULT_GATES = "device"        # where call_bam evaluates the task gates without a BED (decided by its measurement)
DEFAULT_READS_TABLE = "host"    # where call_bam builds the genotyping reads table: not measured yet, so it stays "host" until scripts/reads_stage.py has been run
                                # on an MI355X (DESIGN.md section 20 has the rule that decides)
DEFAULT_FRAME = "host"          # where call_bam frames the BAM's records: "device" is opt-in; DESIGN.md section 29 has the rule for a change
DEFAULT_INFLATE = "host"        # where call_bam inflates the BAM's BGZF blocks: "device" is opt-in until scripts/inflate_stage.py has been run on an MI355X
                                # and its figures pass the rule of DESIGN.md section 27
DEFAULT_EMIT = "host"           # where call_bam writes the record text: "device" is opt-in; DESIGN.md section 38 has the rule for a change
TRA_GT_MODES = ("alignments", "reads_table", "off")

# what call_bam returns in the text's place with bgzf_prefix=: the BGZF image of prefix + records, its .tbi, the bytes of that text, its records
Compressed = collections.namedtuple("Compressed", "image tbi text_bytes n_records")


def tra_gt_mode(genotype, tra_gt=None):
    """The TRA genotyping of call_bam -> "alignments" | "reads_table" | "off": `tra_gt` when given, else CUTESV_AMD_TRA_GT.
    alignments: every alignment of the BAM counts, as in the reference (aln.tra_genotype over the table the tasks fill);
    reads_table: the engine's walk over the gated reads table; off: the fields stay '.'.  "bam" (resolve's default) is refused:
    tra_bam reads the BAM through pysam, not through bam.BamFile"""
    mode = (os.environ.get("CUTESV_AMD_TRA_GT", "bam") if tra_gt is None else tra_gt) if genotype else "off"
    if mode not in TRA_GT_MODES:
        raise ValueError("call_bam genotypes TRA calls with CUTESV_AMD_TRA_GT=alignments (from every alignment, as the reference does) or "
                         "CUTESV_AMD_TRA_GT=reads_table, or leaves them with CUTESV_AMD_TRA_GT=off; %r is not available here "
                         "(the pysam-based mode needs resolve.phase3 with bam=)" % (mode,))
    return mode


def _genotype_tra_from_alignments(ctx, segs, res, contig_len, p):
    """alignments mode: the TRA calls of the result genotyped over the context's alignment table (aln.tra_genotype on the
    support_sig rows of the kept rebuild) and the answer written into the result - DR, and the GL table index of (DR, DV), -1
    where count_coverage gave up - with the TRA segments marked as genotyped: resolve._genotype_tra_from_bam's write-back"""
    from . import aln
    from .genotype import gl_index
    n = res.n_calls
    tra_seg = np.flatnonzero(segs["svtype"] == _abi.TRA)
    arr = res.arrays
    idx = np.flatnonzero(np.isin(arr["call_seg"][:n], tra_seg))
    if len(idx):
        soff = arr["support_off"][:n + 1]
        cnt = (soff[idx + 1] - soff[idx]).astype(np.int64)
        off = np.r_[0, np.cumsum(cnt)]
        pick = np.repeat(soff[idx] - off[:-1], cnt) + np.arange(int(off[-1]))          # the calls' support lists, back to back
        dr, status = aln.tra_genotype(ctx, segs["chrom"][arr["call_seg"][idx]], arr["bp1"][idx], arr["call_aux"][idx] >> 3, arr["bp2"][idx], off,
                                      arr["support_sig"][pick], contig_len, p.max_cluster_bias_TRA, p.gt_round, flags=aln.FROM_KEPT_REBUILD)
        for c, d, s, dv in zip(idx.tolist(), dr.tolist(), status.tolist(), arr["support"][idx].tolist()):
            if s == -1:
                arr["gl_idx"][c] = -1
            else:
                arr["dr"][c] = d
                arr["gl_idx"][c] = gl_index(d, dv)
    segs["genotype"][tra_seg] = 1


class _Shim:
    """what vcf.emit_records reads of a store when the strings come with ins_alt= / rnames="""

    def __init__(self, chroms, strands=("++", "--")):
        self.chroms, self.strands = list(chroms), tuple(strands)


# call_bam's option keywords, checked and with their defaults filled in (resolve_options; call_bam's docstring has the meanings).  regions: the bed.Regions
# of include_bed or None; mode: tra_gt_mode's answer; cp: the CallParams; p: cp.resolve with genotype_tra set for mode "reads_table"; reads_dev: the tasks
# append to the context's device-resident reads table; build_index: index="build" for a path - the session builds what the file lacks
Options = dataclasses.make_dataclass("Options", "reads_table frame inflate ref_route gates regions mode cp p reads_dev task_cut cut_threads index_format build_index emit".split(),
                                     frozen=True)


def _route(name, value, default):
    """a host/device option: None takes `default` (None is then kept); ValueError for anything else"""
    value = default if value is None else value
    if value not in (None, "host", "device"):
        raise ValueError("%s must be 'host' or 'device', not %r" % (name, value))
    return value


def resolve_options(bam, index, params, tra_gt=None, include_bed=None, gates=None, reads_table=None, inflate=None, frame=None, task_cut=None, cut_threads=16,
                    index_format="bai", ref_route=None, emit=None):
    """call_bam's keywords as they arrive -> Options.  Pure: of `bam` it reads whether it is an open reader with an index, it opens nothing
    but a BED file, and DEFAULT_* are read now.  The refusals fire in the order below; `gates` is task_to_pool's to
    check, and the second index check ("none was found for <path>") is the session's, which knows the reader."""
    is_reader = hasattr(bam, "references")
    if index_format not in ("bai", "csi"):
        raise ValueError("index_format must be 'bai' or 'csi', not %r" % (index_format,))
    ref_route = _route("ref_route", ref_route, None)
    emit = _route("emit", emit, DEFAULT_EMIT)
    if task_cut not in (None, "uniform", "index"):
        raise ValueError("task_cut must be None, 'uniform' or 'index', not %r" % (task_cut,))
    if task_cut == "index" and not (getattr(bam, "has_index", False) if is_reader else index is not False):
        raise ValueError("task_cut='index' needs a BAM index (.bai): this reader has none")
    reads_table = _route("reads_table", reads_table, DEFAULT_READS_TABLE)
    frame = _route("frame", frame, DEFAULT_FRAME)
    if frame == "device" and inflate == "host":
        raise ValueError("frame='device' needs the device inflate: inflate='host' cannot be combined with it")
    inflate = _route("inflate", inflate, "device" if frame == "device" else DEFAULT_INFLATE)
    regions = None if include_bed is None else include_bed if isinstance(include_bed, bed_mod.Regions) else bed_mod.load_bed(include_bed)
    if gates is None:
        gates = "device" if regions is not None else DEFAULT_GATES
    cp = params if isinstance(params, CallParams) else CallParams(resolve=params)
    mode = tra_gt_mode(cp.resolve.genotype, tra_gt)
    if task_cut == "index" and (not isinstance(cut_threads, (int, np.integer)) or cut_threads < 1):
        raise ValueError("cut_threads must be a positive integer, not %r" % (cut_threads,))
    p = dataclasses.replace(cp.resolve, genotype_tra=(mode == "reads_table"))
    return Options(reads_table, frame, inflate, ref_route, gates, regions, mode, cp, p, reads_table == "device" and p.genotype, task_cut, cut_threads, index_format,
                   not is_reader and isinstance(index, str) and index == "build", emit)


@contextlib.contextmanager
def _session(bam, ctx, opts, threads, index, timings, read_stats):
    """-> (reader, context, laps) for one call: on the call's inflate and frame routes, with the index built when that was asked for.  What
    the session opened is closed at the end, the reader before the context it may inflate on, and as soon as a later step fails; a reader
    that was handed in gets its previous inflate setting back, and device framing if it had it; a context that was handed in is left alone."""
    with contextlib.ExitStack() as stack:
        own_ctx = stack.enter_context(contextlib.ExitStack())          # (entered first, so released last: after the reader)
        bf = bam if isinstance(bam, bam_mod.BamFile) else stack.enter_context(
            contextlib.closing(bam_mod.BamFile(bam, threads=threads, index=None if opts.build_index else index)))
        if ctx is None:
            ctx = own_ctx.enter_context(contextlib.closing(engine.Context(0)))
        laps = _Laps(timings, read_stats)
        if opts.task_cut == "index" and not bf.has_index and not opts.build_index:
            raise ValueError("task_cut='index' needs a BAM index (.bai): none was found for %s" % bf.path)
        was_framed = bf.frame is not None
        previous = bf.set_inflate(ctx if opts.inflate == "device" else None)
        if bf is bam and was_framed:
            stack.callback(bf.set_frame, "device")
        if bf is bam:
            stack.callback(bf.set_inflate, previous)                   # (callbacks run last in, first out: the inflate setting goes back first)
        bf.set_frame(opts.frame)
        if opts.build_index:
            if not bf.has_index:
                bf.build_index(format=opts.index_format)
            laps.lap("ms_index")
        yield bf, ctx, laps


class _Laps:
    """the caller's `timings` and `read_stats` (either may be None): lap(key) adds the wall milliseconds since the last lap (or the start) to timings[key];
    add_task the sums of one task - `stats`: the reader's last_stats (a task reads its records in one call), `r`: what task_to_pool returned"""

    def __init__(self, timings, read_stats):
        self.timings, self.read_stats, self.clock = timings, read_stats, time.perf_counter()

    def lap(self, key):
        now = time.perf_counter()
        if self.timings is not None:
            self.timings[key] = self.timings.get(key, 0.0) + (now - self.clock) * 1e3
        self.clock = now

    def add_task(self, stats, r):
        if self.timings is not None:
            for key in ("ms_inflate", "ms_frame"):
                self.timings[key] = self.timings.get(key, 0.0) + stats[key]
        if self.read_stats is not None:
            self.read_stats["compressed_bytes"] = self.read_stats.get("compressed_bytes", 0) + stats["compressed_bytes"]
            self.read_stats["n_records"] = self.read_stats.get("n_records", 0) + r["n_records"]
            self.read_stats.setdefault("task_records", []).append(r["n_records"])


# the contigs' names sorted, {contig: bases}, {contig: name rank}, the lengths in rank order, the contigs to call on
_Chroms = collections.namedtuple("_Chroms", "names length crank contig_len wanted")


def _chrom_table(bf, chroms):
    """the chromosome table in name order: a chromosome's index is its name rank, the numbering of rebuild._segments and of a TRA row's mate"""
    names = sorted(bf.references)
    wanted = names if chroms is None else [c for c in names if c in set(chroms)]
    if chroms is not None and len(wanted) != len(set(chroms)):
        raise KeyError("no reference %r in the BAM header" % sorted(set(chroms) - set(names))[0])
    length = dict(zip(bf.references, bf.lengths))
    return _Chroms(names, length, {c: i for i, c in enumerate(names)}, np.array([length[c] for c in names], np.int64), wanted)


def _task_list(bf, ch, opts, batch):
    """-> [(contig, start, end)] in name order, which keeps the ordering contracts of the appends; the bounds as the cut makes them: floats under the index cut"""
    if opts.task_cut != "index":
        return [(c, t0, t1) for c in ch.wanted for t0, t1 in cut_tasks(ch.length[c], batch)]
    by_contig = {}
    for c, t0, t1 in cut_tasks_index(bf.index_statistics(), ch.length, batch, int(opts.cut_threads)):
        by_contig.setdefault(c, []).append((t0, t1))
    return [(c, t0, t1) for c in ch.wanted for t0, t1 in by_contig.get(c, [])]


def _run_tasks(ctx, bf, ch, tasks, opts, laps):
    """the pools reset, every task through extract.task_to_pool -> [(chromosome index, its reads-table columns)] for reads_table="host" with genotype, else []"""
    n_chrom, crank = len(ch.names), ch.crank
    seg_of = {t: ti * n_chrom for ti, t in enumerate(TYPES)}
    seg_base = [seg_of[t] for t in ("DEL", "INS", "DUP", "INV", "TRA")]
    rebuild.pool_reset(ctx)
    rebuild.name_pool_reset(ctx)
    if opts.mode == "alignments":
        aln.reset(ctx, n_chrom)
    if opts.reads_dev:
        reads_mod.reset(ctx, n_chrom)
    tables = []
    skip = opts.regions is not None and bf.has_index and opts.mode != "alignments"      # a task reads its regions only: the alignment table needs every record
    for c, t0, t1 in tasks:
        regs = None if opts.regions is None else opts.regions.for_task(c, t0, t1)      # (the bounds as they are)
        i0, i1 = task_bounds(t0, t1)
        r = extract.task_to_pool(ctx, bf, c, i0, i1, crank, *opts.cp.pipe_args(), seg_of["INS"] + crank[c], seg_of["DEL"] + crank[c], seg_base, None,
                                 name_pool=True, seq_pool=True, aln=(opts.mode == "alignments"), gates=opts.gates, reads="device" if opts.reads_dev else "host",
                                 bed_regions=regs, ranges=task_ranges(bf, c, regs, i0, i1) if skip else None)
        if opts.p.genotype and not opts.reads_dev:
            tables.append((crank[c], r))
        laps.add_task(bf.last_stats, r)
    return tables


def _empty_result(sigs_dir, as_bytes, svid):
    """no signature at all: an empty text, and with sigs_dir five empty files, as the reference's open(..., "w") leaves them"""
    if sigs_dir is not None:
        for t in TYPES:
            open(os.path.join(sigs_dir, t + ".sigs"), "wb").close()
    return (b"" if as_bytes else ""), (np.zeros(5, np.int64) if svid is None else svid)


def _rebuild(ctx, names):
    """the pool sorted and de-duplicated by read name, INS ties settled from the sequences, columns kept on the device -> (contig order, rebuild)"""
    order, _, major, nodedup = rebuild._segments(names, True)
    rb = rebuild.rebuild_pool_by_name(ctx, major, nodedup, keep_on_device=True, ties="seqs")
    if rb["n_ins_ties"]:
        raise ValueError("%d INS rows were not settled on the device" % rb["n_ins_ties"])
    return order, rb


def _cluster(ctx, ch, order, rb, tables, opts):
    """one segment record per (type, contig) with rows, the genotyping reads table (device, host or none), csv_cluster_batch in place -> (segs, result)"""
    n_chrom, p = len(ch.names), opts.p
    off = np.r_[0, np.cumsum(rb["seg_count"])]
    segs = [segment_record(TYPES[s // n_chrom], order[s % n_chrom], int(off[s]), int(off[s + 1]), p, have_contig_len=p.genotype_tra)
            for s in np.flatnonzero(rb["seg_count"]).tolist()]
    segs = np.array(segs, dtype=_abi.SEGMENT_DTYPE)
    reads = {}
    if opts.reads_dev:
        # (`wanted` is in name-rank order and a contig's tasks ran in order: the appends arrived grouped by chromosome)
        reads = dict(reads_dev=reads_mod.batch_columns(ctx, n_chrom, reads_mod.RANK_FROM_NAMES))
    elif p.genotype and tables:
        reads = reads_mod.table_host(tables, rebuild.name_ranks(ctx)["rank"], n_chrom)
    if reads and p.genotype_tra:
        reads["contig_len"] = ch.contig_len
    return segs, ctx.cluster_batch(_abi.HostBatch.on_device(segs, rb["dev"], rb["n_out"], n_chrom=n_chrom, keep=ctx, **reads))


def _gather_alt(ctx, segs, res, t):
    """the ALT bases of the INS calls, gathered on the device -> (blob, lengths)"""
    ins = np.flatnonzero(segs["svtype"][t["call_seg"]] == _abi.INS) if res.n_calls else np.zeros(0, np.int64)
    blob, aoff = rebuild.alt_gather(ctx, t["seq_pick"][ins], t["bp2"][ins])
    return blob, np.diff(aoff)


def _compressed_host(ctx, text):
    """a text that is on the host (a header without records) as call_bam's Compressed"""
    from . import bgzf
    image, table = bgzf.compress(text, ctx=ctx, route="device")
    return Compressed(image, bgzf.tabix_vcf(text, table, ctx=ctx, route="device"), len(text), 0)


def _emit_on_device(ctx, ch, segs, res, t, reference, opts, report_readid, ignore_sequence, svid, as_bytes, bgzf_prefix, timings, laps):
    """emit="device": the fused form of _gather_alt, support_join and the emitter - picks, clips and support offsets visit the host, the
    strings they select do not -> call_bam's result"""
    ins = np.flatnonzero(segs["svtype"][t["call_seg"]] == _abi.INS) if res.n_calls else np.zeros(0, np.int64)
    from_pool = (np.zeros(0, np.int64), np.zeros(0, np.int64)) if ignore_sequence else (t["seq_pick"][ins], t["bp2"][ins])
    own = {} if timings is None else timings
    out, svid = vcf.emit_records(_Shim(ch.names), segs, res, reference, min_size=opts.p.min_size, max_size=opts.p.max_size, genotype=opts.p.genotype,
                                 report_readid=report_readid, ignore_sequence=ignore_sequence, svid=svid, as_bytes=as_bytes, ref_ctx=ctx, ref_route=opts.ref_route,
                                 route="device", ctx=ctx, from_pool=from_pool, keep=bgzf_prefix, timings=own)
    laps.lap("ms_emit")
    if bgzf_prefix is None:
        return out, svid
    from . import bgzf
    image, table = bgzf.compress_kept(ctx, out, timings=timings)
    laps.lap("ms_bgzf")
    tbi = bgzf.tabix_rows(out, table, ctx=ctx, route="device")
    laps.lap("ms_tabix")
    return Compressed(image, tbi, out.n_bytes, out.n_records), svid


def call_bam(bam, reference, params, ctx=None, chroms=None, batch=10_000_000, report_readid=False, ignore_sequence=False, threads=None, svid=None,
             as_bytes=False, timings=None, tra_gt=None, include_bed=None, gates=None, reads_table=None, sigs_dir=None, inflate=None, index=None, task_cut=None,
             cut_threads=16, read_stats=None, frame=None, index_format="bai", ref_route=None, emit=None, bgzf_prefix=None):
    """-> (VCF body text, svid counters [INS, DEL, BND, DUP, INV]).

    bam        a path or an open bam.BamFile (coordinate-sorted; no index is needed, one beside the file is used - see `index`)
    reference  a fasta.Reference, a fasta.BgzfReference (fasta.open_reference gives either) or {contig: sequence}: the REF bases
    params     a CallParams, or a columns.Params (the gates then take the reference's defaults)
    ctx        an engine.Context (default: one on device 0 for the call); its pool, name pool and sequence pool are reset
    chroms     the contigs to call on (default: all of the header); TRA mates may lie on any contig of the header
    batch      reference bases per extraction task (the reference's -b)
    timings    a dict that receives the wall milliseconds of the stages (tasks, rebuild, sigs, cluster, tra_gt, gather, emit) and
               ms_inflate, the part of ms_tasks the reader spent inflating (either route: staging, copies, kernels and fallback included)
    tra_gt     how TRA calls are genotyped: "alignments", "reads_table" or "off"; None follows CUTESV_AMD_TRA_GT (ValueError for
               bam, see tra_gt_mode)
    include_bed  a BED file's path or a bed.Regions: only call where these regions are (the reference's -include_bed).  Every task
               gets `regions.for_task(contig, start, end)` - the reference's rule, under which a read that starts in one task and
               reaches only a region that begins in the next is dropped: with a BED the calls depend on `batch`.  TRA genotyping
               from every alignment (tra_gt="alignments") is not restricted, as in the reference.  None: no gate.
    gates      "host" or "device": where the task gates are evaluated (extract.task_to_pool); None: "device" with include_bed,
               else DEFAULT_GATES (also "device": DESIGN.md section 19 has the measurement that decided it)
    reads_table  "host" or "device": where the genotyping reads table is built (only with params.genotype; None: DEFAULT_READS_TABLE).
               host: every task's rows are cut out of the downloaded columns and the table is assembled with numpy (reads.table_host);
               device: the tasks append their rows to the context's device-resident table (reads.append_decoded), the name ranks are
               gathered there and the engine copies the columns device to device.  Same text either way.
    sigs_dir   a directory that receives the rebuilt signatures as cuteSV's --write_old_sigs files (DEL.sigs .. TRA.sigs, made on the
               device by rebuild.write_sigs right after the rebuild; empty files when the BAM yields no signature).  The
               returned text and svid do not depend on it.  None: no files.
    inflate    "host" or "device": where the BGZF blocks are inflated (None: DEFAULT_INFLATE).  device: on `ctx`, one wavefront per
               block; a BamFile that was handed in gets the context for the call and its previous setting back
               at the end.  Same text either way.
    frame      "host" or "device": where the records are framed (None: DEFAULT_FRAME).  device: on `ctx`, out of a window that never
               leaves it; it takes the device inflate when `inflate` is None (ValueError with an explicit
               inflate="host"); a BamFile that was handed in gets its previous setting back at the end.  Same text either way.
    index      for a path: None - the .bai beside the file is loaded when there is one; a path - that index; False - none
               (bam.BamFile's `index`); "build" - the .bai beside the file when there is one, else an index is built in memory
               (BamFile.build_index) once the call's inflate and frame routes are set, so on them; nothing is
               written, timings["ms_index"] says what it took (0 when a file was found), and the file is inflated twice - for the
               build, then for the tasks.  An open BamFile comes with what it has.  With an index every task's read starts at its
               linear-index entry, and under include_bed - unless tra_gt="alignments" fills the alignment table, which needs every
               record - a task reads only the union of its regions (task_ranges), and nothing when it has none.  The gates are
               unchanged and decide; the text does not depend on the index.  A .csi beside the file serves
               as well as a .bai.
    index_format  with index="build": "bai", or "csi" - the format a file with a contig of 2^29 bases or more needs (htslib's
               min_shift 14 and its rule for the depth).  The text does not depend on it.
    task_cut   None or "uniform": cut_tasks, every contig by `batch`.  "index": cut_tasks_index, the reference's cut from the index
               statistics with `cut_threads` as its -t - under include_bed the cut decides which reads survive, and this is the cut
               cuteSV makes.  ValueError without an index.
    ref_route  "host" or "device": where the REF bases of a fasta.BgzfReference are gathered (None: the reference's own route, else
               fasta.DEFAULT_REF_ROUTE).  device: on `ctx`.  Same text either way; no other kind of reference
               looks at it.
    emit       "host" or "device": where the record text is written (None: DEFAULT_EMIT).  device: on `ctx` - the ALT
               bases and the read names are gathered from the kept rebuild inside the emit and stay on the device, k_vcf_write writes
               the records; timings gets ms_emit_kernels.  Same text either way.
    bgzf_prefix  bytes (with emit="device"; ValueError otherwise): the text - these bytes, a VCF header, and the records behind them -
               stays on the device, is compressed there and indexed from the emitter's rows; the call returns
               (Compressed(image, tbi, text_bytes, n_records), svid) and the text never comes down.
    read_stats a dict that receives what the tasks' reads cost: compressed_bytes and n_records summed over the tasks, task_records - the
               records each task read, in task order."""
    opts = resolve_options(bam, index, params, tra_gt, include_bed, gates, reads_table, inflate, frame, task_cut, cut_threads, index_format, ref_route, emit)
    if bgzf_prefix is not None and opts.emit != "device":
        raise ValueError("bgzf_prefix needs emit='device': the host emitter's text is compressed by bgzf.compress")
    with _session(bam, ctx, opts, threads, index, timings, read_stats) as (bf, ctx, laps):
        ch = _chrom_table(bf, chroms)
        tables = _run_tasks(ctx, bf, ch, _task_list(bf, ch, opts, batch), opts, laps)
        laps.lap("ms_tasks")
        if rebuild.pool_rows(ctx) == 0:
            text, svid = _empty_result(sigs_dir, as_bytes, svid)
            return (text, svid) if bgzf_prefix is None else (_compressed_host(ctx, bytes(bgzf_prefix)), svid)
        order, rb = _rebuild(ctx, ch.names)
        laps.lap("ms_rebuild")
        if sigs_dir is not None:
            rebuild.write_sigs(ctx, rb, ch.names, sigs_dir)
            laps.lap("ms_sigs")
        segs, res = _cluster(ctx, ch, order, rb, tables, opts)
        laps.lap("ms_cluster")
        if opts.mode == "alignments":
            _genotype_tra_from_alignments(ctx, segs, res, ch.contig_len, opts.p)
        laps.lap("ms_tra_gt")
        t = res.trimmed()
        if opts.emit == "device":
            return _emit_on_device(ctx, ch, segs, res, t, reference, opts, report_readid, ignore_sequence, svid, as_bytes, bgzf_prefix, timings, laps)
        ins_alt = None if ignore_sequence else _gather_alt(ctx, segs, res, t)
        laps.lap("ms_alt_gather")
        rnames = rebuild.support_join(ctx, t["support_off"], t["support_sig"]) if report_readid else None
        laps.lap("ms_support_join")
        out = vcf.emit_records(_Shim(ch.names), segs, res, reference, min_size=opts.p.min_size, max_size=opts.p.max_size, genotype=opts.p.genotype, report_readid=report_readid,
                               ignore_sequence=ignore_sequence, svid=svid, as_bytes=as_bytes, ins_alt=ins_alt, rnames=rnames, ref_ctx=ctx, ref_route=opts.ref_route)
        laps.lap("ms_emit")
        return out


def add_route_options(ap):
    """the route options that python -m cutesv_amd.call and cli.py's own parser share, declared here once"""
    hd = ["host", "device"]
    ap.add_argument("--reads_table", default=None, choices=hd, help="with --genotype: where the genotyping reads table is built (default: %s)" % DEFAULT_READS_TABLE)
    ap.add_argument("--tra_gt", default=None, choices=list(TRA_GT_MODES),
                    help="with --genotype: how BND records are genotyped (default: CUTESV_AMD_TRA_GT, else alignments - every alignment counts, as in cuteSV)")
    ap.add_argument("--inflate", default=None, choices=hd, help="where the BAM's BGZF blocks are inflated (default: %s)" % DEFAULT_INFLATE)
    ap.add_argument("--frame", default=None, choices=hd, help="where the BAM's records are framed (default: %s; device takes the device inflate)" % DEFAULT_FRAME)
    ap.add_argument("--ref_route", default=None, choices=hd, help="where the REF bases of a BGZF-compressed reference are gathered (default: %s)" % fasta.DEFAULT_REF_ROUTE)
    ap.add_argument("--emit", default=None, choices=hd, help="where the record text is written (default: %s)" % DEFAULT_EMIT)


def command_line_tra_gt(tra_gt, genotype):
    """--tra_gt as a command line hands it to call_bam: with --genotype and neither the option nor CUTESV_AMD_TRA_GT, "alignments" - as cuteSV counts"""
    return "alignments" if tra_gt is None and genotype and "CUTESV_AMD_TRA_GT" not in os.environ else tra_gt


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m cutesv_amd.call", description="SV calls of a BAM file as VCF records (the body; no header)")
    ap.add_argument("bam")
    ap.add_argument("reference", help="reference FASTA, plain or BGZF-compressed (an .fai - and a .gzi - beside it is used, or built in memory)")
    ap.add_argument("-o", "--out", required=True)
    ap.add_argument("--preset", default="clr", choices=["ont", "hifi", "clr"], help="cluster bias / merging ratio of INS and DEL as the README of cuteSV suggests")
    ap.add_argument("--genotype", action="store_true")
    ap.add_argument("--report_readid", action="store_true")
    ap.add_argument("--ignore_sequence", action="store_true", help="<INS> instead of the inserted bases")
    for name, default in (("min_support", 10), ("min_size", 30), ("max_size", 100000), ("min_mapq", 20), ("min_read_len", 500), ("max_split_parts", 7),
                          ("min_siglength", 10), ("merge_del_threshold", 0), ("merge_ins_threshold", 100)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--batch", type=int, default=10_000_000, help="reference bases per extraction task")
    ap.add_argument("--threads", type=int, default=None, help="host threads that inflate the BAM")
    ap.add_argument("--chroms", default=None, help="comma-separated contigs (default: all)")
    ap.add_argument("--include_bed", "-include_bed", default=None, metavar="FILE",
                    help="only call where the regions of this BED file are (padded by 1000 bases, as in cuteSV); the calls then depend on --batch")
    add_route_options(ap)
    ap.add_argument("--sigs_dir", default=None, metavar="DIR", help="also write the rebuilt signatures there as cuteSV's --write_old_sigs files (DEL.sigs .. TRA.sigs)")
    a = ap.parse_args(argv)
    p = getattr(Params, a.preset)(min_support=a.min_support, min_size=a.min_size, max_size=a.max_size, genotype=a.genotype)
    cp = CallParams(p, min_mapq=a.min_mapq, max_split_parts=a.max_split_parts, min_read_len=a.min_read_len, min_siglength=a.min_siglength,
                    merge_del_threshold=a.merge_del_threshold, merge_ins_threshold=a.merge_ins_threshold)
    with fasta.opened_reference(a.reference, a.threads) as reference:
        text, svid = call_bam(a.bam, reference, cp, chroms=a.chroms.split(",") if a.chroms else None, batch=a.batch, report_readid=a.report_readid,
                              ignore_sequence=a.ignore_sequence, threads=a.threads, as_bytes=True, tra_gt=command_line_tra_gt(a.tra_gt, a.genotype),
                              include_bed=a.include_bed, reads_table=a.reads_table, sigs_dir=a.sigs_dir, inflate=a.inflate, frame=a.frame, ref_route=a.ref_route, emit=a.emit)
    with open(a.out, "wb") as f:
        f.write(text)
    print("%d records: INS %d, DEL %d, BND %d, DUP %d, INV %d" % (text.count(b"\n"), *svid.tolist()))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
