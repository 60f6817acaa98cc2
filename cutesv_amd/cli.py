"""cuteSV's command line on this project's chain:

    python -m cutesv_amd BAM REF OUT.vcf WORK_DIR [cuteSV's flags] [--reads_table {host,device}] [--tra_gt MODE] [--inflate {host,device}] [--frame {host,device}]
                         [--task_cut {index,uniform}] [--build_index] [--index_format {bai,csi}] [--bgzf {host,device}]
                         [--ref_route {host,device}] [--emit {host,device}] [--sort_input {host,device}]

`parse_args` accepts every option of cuteSV v2.1.4 under the same short and long spellings, with the same destination, type
and default, so a command line written for cuteSV runs here unchanged; `main` maps them onto call.call_bam and writes a complete
VCF file: vcf.header_text followed by the records.  With --write_old_sigs the work directory receives DEL.sigs, INS.sigs,
DUP.sigs, INV.sigs and TRA.sigs, made on the device (rebuild.write_sigs); without --retain_work_dir they are removed again at
the end, as cuteSV's cleanup removes its own.  An OUT name that ends in .gz or .bgz is written BGZF-compressed - header and records as
one stream - with its tabix index OUT.tbi beside it (bgzf.py; --bgzf picks the compressor: zlib on host threads
or csv_bgzf_deflate on the device); any other name receives the plain text, as before.

The files of this chain: cli.py (this command line) -> call.py (call_bam: BAM to VCF records in named phases, its options resolver and
reader session, and what the two command lines share) over bam.py (the reader), extract.py, rebuild.py, engine.py and genotype.py;
vcf.py (header and records), fasta.py (the reference), bgzf.py (the BGZF writer and the tabix index of a compressed OUT).

What differs from cuteSV, on purpose:
  * The extraction tasks: with a .bai beside the BAM file (cuteSV cannot run without one) they are cuteSV's own cut from the index
    statistics (call.cut_tasks_index with -t; --task_cut index).  Without one - or with --task_cut uniform -
    they are call.cut_tasks' uniform cut of every contig by -b, and one line on stderr says so; with --build_index the missing index
    is built in memory first (nothing is written; --index_format csi for a file with a contig of 2^29 bases or
    more) and the cut is cuteSV's.  A .csi beside the file serves as a .bai does.  The calls do not depend on the
    cut - except with -include_bed, where a task's reads are tested against the regions of that task only: there the uniform cut
    can differ from cuteSV's on contigs whose batch it would have shrunk.
  * --sort_input takes a BAM file in any order - what `minimap2 -a | samtools view -b` writes - or the SAM text `minimap2 -a` writes
    itself (told by content; converted first on the same route): it is sorted by coordinate first
    (bam.sort_bam; "device": keys, order, gather and compression on the GPU, "host": the same on the host) into
    WORK_DIR/<BAM's name minus .bam>.sorted.bam, and the run goes on with that file exactly as with a sorted input; the file is removed at
    the end unless --retain_work_dir is set.  Without the option an unsorted input is refused, as before.
  * reads.sigs is not written (its row order in cuteSV depends on which worker process wrote which task).
  * Force calling (-Ivcf) is not available, as in cuteSV v2.1.4 itself.
  * --read_range is accepted and unused, as on cuteSV's calling path.  -t sizes the BAM reader's inflate threads.
"""
import argparse
import contextlib
import os
import sys
import time

from .columns import Params, TYPES

VERSION = "2.1.4"                      # the cuteSV version whose command line and output this restates

# (flags, options of add_argument) per group, in cuteSV's order; every default and type is cuteSV v2.1.4's
_SWITCH = dict(action="store_true")
_GENERAL = (
    (("-t", "--threads"), dict(type=int, default=16, help="host threads (here: the BAM reader's inflate threads) [%(default)s]")),
    (("-b", "--batches"), dict(type=int, default=10000000, help="reference bases per extraction task [%(default)s]")),
    (("-S", "--sample"), dict(type=str, default="NULL", help="sample name of the VCF's last column [%(default)s]")),
    (("--retain_work_dir",), dict(help="keep the files written into WORK_DIR", **_SWITCH)),
    (("--write_old_sigs",), dict(help="write the rebuilt signatures as <TYPE>.sigs text files into WORK_DIR", **_SWITCH)),
    (("--report_readid",), dict(help="report the names of the supporting reads (RNAMES)", **_SWITCH)),
    (("--ignore_sequence",), dict(help="write <INS> / <DEL> instead of the bases", **_SWITCH)),
)
_COLLECT = (
    (("-p", "--max_split_parts"), dict(type=int, default=7, help="a read split into more alignments is ignored; -1: none is [%(default)s]")),
    (("-q", "--min_mapq"), dict(type=int, default=20, help="smallest mapping quality of an alignment that counts [%(default)s]")),
    (("-r", "--min_read_len"), dict(type=int, default=500, help="shorter reads are ignored [%(default)s]")),
    (("-md", "--merge_del_threshold"), dict(type=int, default=0, help="deletion signals at most this far apart are merged [%(default)s]")),
    (("-mi", "--merge_ins_threshold"), dict(type=int, default=100, help="insertion signals at most this far apart are merged [%(default)s]")),
    (("-include_bed",), dict(type=str, default=None, help="only call where the regions of this BED file are; the calls then depend on the task cut (see above)")),
)
_CLUSTER = (
    (("-s", "--min_support"), dict(type=int, default=10, help="reads that must support a call [%(default)s]")),
    (("-l", "--min_size"), dict(type=int, default=30, help="smallest SV reported [%(default)s]")),
    (("-L", "--max_size"), dict(type=int, default=100000, help="largest SV reported; -1: no limit [%(default)s]")),
    (("-sl", "--min_siglength"), dict(type=int, default=10, help="smallest signal extracted [%(default)s]")),
)
_GENOTYPE = (
    (("--genotype",), dict(help="compute genotypes", **_SWITCH)),
    (("--gt_round",), dict(type=int, default=500, help="rounds of the search for covering reads [%(default)s]")),
    (("--read_range",), dict(type=int, default=1000, help="accepted, unused [%(default)s]")),
)
_FORCE = (
    (("-Ivcf",), dict(type=str, default=None, help="force calling is not available (nor in cuteSV v2.1.4): use cuteFC")),
)
_ADVANCED = (
    (("--max_cluster_bias_INS",), dict(type=int, default=100, help="[%(default)s]")),
    (("--diff_ratio_merging_INS",), dict(type=float, default=0.3, help="[%(default)s]")),
    (("--max_cluster_bias_DEL",), dict(type=int, default=200, help="[%(default)s]")),
    (("--diff_ratio_merging_DEL",), dict(type=float, default=0.5, help="[%(default)s]")),
    (("--max_cluster_bias_INV",), dict(type=int, default=500, help="[%(default)s]")),
    (("--max_cluster_bias_DUP",), dict(type=int, default=500, help="[%(default)s]")),
    (("--max_cluster_bias_TRA",), dict(type=int, default=50, help="[%(default)s]")),
    (("--diff_ratio_filtering_TRA",), dict(type=float, default=0.6, help="[%(default)s]")),
    (("--remain_reads_ratio",), dict(type=float, default=1.0, help="[%(default)s]")),
)
_GROUPS = ((None, _GENERAL), ("Collection of SV signatures", _COLLECT), ("Generation of SV clusters", _CLUSTER), ("Computing genotypes", _GENOTYPE),
           ("Force calling", _FORCE), ("Advanced", _ADVANCED))


def _parser():
    ap = argparse.ArgumentParser(prog="cutesv_amd", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--version", "-v", action="version", version="%(prog)s (cuteSV " + VERSION + ")")
    ap.add_argument("input", metavar="[BAM]", type=str, help="coordinate-sorted BAM file")
    ap.add_argument("reference", type=str, help="reference FASTA")
    ap.add_argument("output", type=str, help="the VCF file to write")
    ap.add_argument("work_dir", type=str, help="an existing directory; holds the .sigs files of --write_old_sigs")
    for title, options in _GROUPS:
        where = ap if title is None else ap.add_argument_group(title)
        for flags, kw in options:
            where.add_argument(*flags, **kw)
    return ap


def _own_parser():
    """the eleven options cuteSV does not have (six are call.add_route_options'); parsed apart (split_own), so that they shadow no abbreviation of a cuteSV flag"""
    from . import call
    ap = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    call.add_route_options(ap)
    ap.add_argument("--task_cut", default=None, choices=["index", "uniform"])
    ap.add_argument("--build_index", action="store_true")
    ap.add_argument("--index_format", default="bai", choices=["bai", "csi"])
    ap.add_argument("--bgzf", default=None, choices=["host", "device"])
    ap.add_argument("--sort_input", default=None, choices=["host", "device"])
    return ap


def split_own(argv):
    """-> (namespace of --reads_table / --tra_gt / --inflate / --frame / --task_cut / --build_index / --index_format / --bgzf / --ref_route / --emit / --sort_input, argv without them)"""
    return _own_parser().parse_known_args(list(argv))


def parse_args(argv):
    """argv (cuteSV's options only) -> the namespace cuteSV's own parser gives: same names, types and defaults"""
    return _parser().parse_args(list(argv))


def call_params(a):
    """the namespace of parse_args -> call.CallParams: the flags are the values, no preset"""
    from .call import CallParams
    p = Params(min_support=a.min_support, min_size=a.min_size, max_size=a.max_size, genotype=a.genotype, gt_round=a.gt_round,
               max_cluster_bias_INS=a.max_cluster_bias_INS, diff_ratio_merging_INS=a.diff_ratio_merging_INS,
               max_cluster_bias_DEL=a.max_cluster_bias_DEL, diff_ratio_merging_DEL=a.diff_ratio_merging_DEL,
               max_cluster_bias_INV=a.max_cluster_bias_INV, max_cluster_bias_DUP=a.max_cluster_bias_DUP,
               max_cluster_bias_TRA=a.max_cluster_bias_TRA, diff_ratio_filtering_TRA=a.diff_ratio_filtering_TRA, remain_reads_ratio=a.remain_reads_ratio)
    return CallParams(p, min_mapq=a.min_mapq, max_split_parts=a.max_split_parts, min_read_len=a.min_read_len, min_siglength=a.min_siglength,
                      merge_del_threshold=a.merge_del_threshold, merge_ins_threshold=a.merge_ins_threshold)


def _log(msg):
    print("cutesv_amd: " + msg, file=sys.stderr)


def _write_bgzf(path, text, route):
    """header and records as one BGZF stream into `path`, its tabix index into path + ".tbi"; one log line each"""
    from . import bgzf
    route = bgzf.DEFAULT_ROUTE if route is None else route
    t0 = time.perf_counter()
    image, table = bgzf.compress(text, route=route)
    t1 = time.perf_counter()
    tbi = bgzf.tabix_vcf(text, table)
    t2 = time.perf_counter()
    with open(path, "wb") as f:
        f.write(image)
    with open(path + ".tbi", "wb") as f:
        f.write(tbi)
    _log("%-16s %10.1f ms  (%s: %d -> %d bytes in %d blocks)" % ("bgzf", 1e3 * (t1 - t0), route, len(text), len(image), len(table[0])))
    _log("%-16s %10.1f ms  (%s.tbi, %d bytes)" % ("tabix", 1e3 * (t2 - t1), os.path.basename(path), len(tbi)))


def sorted_input_path(work_dir, bam_path):
    """where --sort_input writes the sorted file: WORK_DIR/<the input's name minus .bam or .sam>.sorted.bam"""
    base = os.path.basename(bam_path)
    return os.path.join(work_dir, (base[:-4] if base.endswith((".bam", ".sam")) else base) + ".sorted.bam")


def _sort_input(a, own):
    """--sort_input: the input sorted by coordinate into WORK_DIR on the routes of --inflate / --frame -> the sorted file's path"""
    from . import bam as bam_mod
    out = sorted_input_path(a.work_dir, a.input)
    if os.path.exists(out):
        raise FileExistsError("[Errno 17] File exists: '%s'" % out)
    _log("%s is sorted by coordinate into %s (--sort_input %s)" % (a.input, out, own.sort_input))
    frame = own.frame if own.sort_input == "device" else None
    st = bam_mod.sort_bam(a.input, out, route=own.sort_input, inflate=own.inflate, frame=frame, threads=a.threads)
    if st.get("sam") is not None:
        sm = st["sam"]
        _log("%-16s %10.1f ms  (SAM text: %d lines, %d -> %d bytes in %d blocks, %d windows; device: lines %.2f, plan %.2f, write %.2f, deflate %.2f ms)"
             % ("sam_to_bam", sm["ms"], sm["lines"], sm["text_bytes"], sm["out_bytes"], sm["blocks"], sm["windows"], sm["ms_lines"], sm["ms_plan"], sm["ms_write"], sm["ms_deflate"]))
    _log("%-16s %10.1f ms  (%d records, %d adjacent inversions, %d -> %d bytes in %d blocks; device: keys %.2f, sort %.2f, gather %.2f, deflate %.2f ms)"
         % ("sort_input", st["ms"], st["records"], st["inversions"], st["inflated_bytes"], st["out_bytes"], st["blocks"], st["ms_keys"], st["ms_sort"], st["ms_gather"], st["ms_deflate"]))
    return out


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    own, rest = split_own(argv)
    a = parse_args(rest)
    if own.sort_input is None:
        return _run(a, own, argv)
    if not os.path.isdir(a.work_dir):
        raise FileNotFoundError("[Errno 2] No such directory: '%s'" % a.work_dir)
    sorted_path = _sort_input(a, own)
    try:
        a.input = sorted_path
        return _run(a, own, argv)
    finally:
        if not a.retain_work_dir:
            for path in (sorted_path, sorted_path + ".bai", sorted_path + ".csi"):
                if os.path.exists(path):
                    os.remove(path)
            _log("%s removed (--retain_work_dir keeps it)" % sorted_path)


def _run(a, own, argv):
    if a.Ivcf is not None:
        raise ValueError("force calling is not available here (it is disabled in cuteSV %s as well): use cuteFC to regenotype a given SV set" % VERSION)
    if not os.path.isfile(a.reference):
        raise FileNotFoundError("[Errno 2] No such file: '%s'" % a.reference)
    if not os.path.isdir(a.work_dir):
        raise FileNotFoundError("[Errno 2] No such directory: '%s'" % a.work_dir)
    for t in TYPES:
        path = os.path.join(a.work_dir, t + ".sigs")
        if os.path.exists(path):
            raise FileExistsError("[Errno 17] File exists: '%s'" % path)
    from . import bam as bam_mod, call, fasta, vcf
    tra_gt = call.command_line_tra_gt(own.tra_gt, a.genotype)
    sigs_dir = a.work_dir if a.write_old_sigs else None
    t0 = time.perf_counter()
    timings = {}
    bf = bam_mod.BamFile(a.input, threads=a.threads)
    try:
        contigs = list(zip(bf.references, bf.lengths))
        _log("%d contigs in %s" % (len(contigs), a.input))
        task_cut = own.task_cut
        source, index = bf, None
        if own.build_index and not bf.has_index:              # the call opens the file itself and builds the index on its routes
            _log("no BAM index (.bai) beside %s: one is built in memory (--build_index)" % a.input)
            bf.close()
            source, index = a.input, "build"
            if task_cut is None:
                task_cut = "index"
        if task_cut is None:
            task_cut = "index" if bf.has_index else "uniform"
            if not bf.has_index:
                _log("no BAM index (.bai) beside %s: the tasks are the uniform cut by -b, not cuteSV's cut from the index statistics" % a.input)
        # a compressed OUT with the device emitter and the device compressor: the header is the prefix of a text that never comes down,
        # and one context serves the whole run
        fused = a.output.endswith((".gz", ".bgz")) and own.emit == "device" and own.bgzf == "device"
        header = vcf.header_text(contigs, a.sample, argv).encode()
        with contextlib.ExitStack() as stack:
            reference = stack.enter_context(fasta.opened_reference(a.reference, a.threads))           # (plain text or BGZF, as pysam.FastaFile takes either)
            more = {}
            if fused:
                from . import engine
                more = dict(ctx=stack.enter_context(contextlib.closing(engine.Context(0))), bgzf_prefix=header)
            body, svid = call.call_bam(source, reference, call_params(a), batch=a.batches, report_readid=a.report_readid,
                                       ignore_sequence=a.ignore_sequence, as_bytes=True, timings=timings, tra_gt=tra_gt, include_bed=a.include_bed,
                                       reads_table=own.reads_table, sigs_dir=sigs_dir, inflate=own.inflate, frame=own.frame, task_cut=task_cut, cut_threads=a.threads,
                                       threads=a.threads, index=index, index_format=own.index_format, ref_route=own.ref_route, emit=own.emit, **more)
    finally:
        bf.close()
    for key, ms in timings.items():
        _log("%-16s %10.1f ms" % (key[3:] if key.startswith("ms_") else key, ms))
    if fused:
        n_records = body.n_records                            # (the rows count the records: the text is not here to be searched)
        with open(a.output, "wb") as f:
            f.write(body.image)
        with open(a.output + ".tbi", "wb") as f:
            f.write(body.tbi)
        _log("%-16s %d -> %d bytes on the device, %s.tbi %d bytes" % ("bgzf", body.text_bytes, len(body.image), os.path.basename(a.output), len(body.tbi)))
    else:
        n_records = body.count(b"\n")
        text = header + body
        if a.output.endswith((".gz", ".bgz")):
            _write_bgzf(a.output, text, own.bgzf)
        else:
            with open(a.output, "wb") as f:
                f.write(text)
    if sigs_dir is not None and not a.retain_work_dir:
        for t in TYPES:
            path = os.path.join(sigs_dir, t + ".sigs")
            if os.path.exists(path):
                os.remove(path)
    _log("%d records (INS %d, DEL %d, BND %d, DUP %d, INV %d) in %.2f s" % (n_records, *svid.tolist(), time.perf_counter() - t0))
    return 0
