"""VCF record emit for the clustering stage's calls.

`emit_records` hands the structure-of-arrays result straight to the native emitter (`csv_vcf_emit`,
cutesv_amd/csrc/vcf_emit.cpp), which restates generate_output (cuteSV_genotype.py:242-467) and main_ctrl's
SVID numbering (cuteSV main script :1208-1237) — no Python row lists in between.  Only the strings a call
needs from Python-side objects are gathered here: the sliced INS sequence (cuteSV_resolveINDEL.py:402), the
read names when --report_readid is on, and the genotype strings of the gl_idx values that occur.
"""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import VcfIn
from ._lib import lib
from .genotype import gl_fields


def _csr(strings):
    blob = "".join(strings).encode()
    off = np.zeros(len(strings) + 1, np.int64)
    if strings:
        off[1:] = np.cumsum([len(s) for s in strings])
    return blob, off


import threading

_TLS = threading.local()          # the recycled output buffer is per thread: csv_vcf_emit runs with the GIL released and supports
                                  # concurrent callers (a second caller gets a worker team of its own), so must its caller's buffer


ROUTES = ("host", "device", "core")
DEFAULT_ROUTE = "host"            # the rule of DESIGN.md section 38 decides a change; its measurement has not been made
KEEP_TEXT, ALT_FROM_POOL, RNAMES_FROM_POOL = 1, 2, 4        # CSV_VCF_* of include/cutesv_hip.h


class KeptText:
    """The text csv_vcf_emit_device left in device memory (emit_records(route="device", keep=prefix)): n_bytes - prefix and records;
    n_records; rows int64[n_records, 4] - {name index, beg, end, offset of the record in the text}; names - the chromosomes that
    emitted a record, in order of first appearance; fetch() - the bytes, brought down.  Good until the context's next device emit:
    after that every use raises."""

    def __init__(self, ctx, n_bytes, rows, names, ms_kernels):
        self.ctx, self.n_bytes, self.rows, self.names, self.ms_kernels = ctx, int(n_bytes), rows, list(names), ms_kernels
        self.n_records = len(rows)
        self._gen = self._info()[0]

    def _info(self):
        gen, nbytes = C.c_int64(0), C.c_int64(0)
        self.ctx._check(lib().csv_vcf_text_info(self.ctx._h, C.byref(gen), C.byref(nbytes)))
        return gen.value, nbytes.value

    def check(self):
        if self._info() != (self._gen, self.n_bytes):
            raise RuntimeError("the kept VCF text is gone: the context has emitted again since")

    def fetch(self):
        self.check()
        out, need = np.empty(max(self.n_bytes, 1), np.uint8), C.c_int64(0)
        self.ctx._check(lib().csv_vcf_text_fetch(self.ctx._h, out.ctypes.data, self.n_bytes, C.byref(need)))
        return out[:need.value].tobytes()


def _host_ref_gather(store, reference, seq_bytes, chrom, beg, end):
    """the bases of the ranges csv_vcf_ref_ranges gave, back to back, for a fasta.Reference or {name: sequence} -> (blob uint8, off int64[n + 1])"""
    from .fasta import Reference
    n = len(beg)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(end - beg, out=off[1:])
    parts = []
    mapped = isinstance(reference, Reference)
    for c in np.flatnonzero(end > beg).tolist():
        ch, b, e = int(chrom[c]), int(beg[c]), int(end[c])
        parts.append(reference.fetch(store.chroms[ch], b, e).encode() if mapped else seq_bytes[ch][b:e])
    blob = np.frombuffer(b"".join(parts), np.uint8)
    if len(blob) != int(off[-1]):
        raise RuntimeError("csv_vcf_emit: a reference sequence is missing or too short")
    return blob, off


def emit_records(store, segments, res, reference, min_size=30, max_size=100000, genotype=False, report_readid=False,
                 ignore_sequence=False, svid=None, as_bytes=False, as_view=False, ins_alt=None, rnames=None, ref_ctx=None, ref_route=None,
                 route=None, ctx=None, from_pool=None, keep=None, timings=None):
    """calls of one batch -> (VCF body text, svid counters).

    segments   the csv_segment records the batch was run with (HostBatch.segments)
    res        _abi.HostResult of that batch
    reference  a fasta.Reference (memory-mapped FASTA + .fai: bases are read in C straight from the mapping), a
               fasta.BgzfReference (a BGZF-compressed FASTA: csv_vcf_ref_ranges says which bases each call's record reads,
               reference.gather fetches them out of the blocks they touch, csv_vcf_emit_ref writes the records), or
               {chromosome name: sequence (str or bytes)}; may miss chromosomes without calls
    ref_ctx / ref_route   the context and the route ("host", "device"; None: the reference's own) of BgzfReference.gather;
               no other kind of reference looks at them
    svid       running counters [INS, DEL, BND, DUP, INV] (main script :1209-1213), advanced in place
    as_bytes   return the text as `bytes` (what a file is written from) instead of decoding it to `str`
    as_view    return a memoryview of this thread's output buffer instead (valid until the thread's next emit_records call):
               `f.write(view)` needs no copy of the text - with real REF sequences a 30x genome's records are ~30 MB
    ins_alt    (blob, bytes taken per INS call): the ALT bases of the INS calls, in call order, made elsewhere
               (rebuild.alt_gather: the bases live in the device's sequence pool) - `store.ins_seq` is not looked at.
               ValueError unless there is one length per INS call and the lengths add up to the blob
    rnames     (blob, off int64[n_calls + 1]): the RNAMES text of every call (rebuild.support_join) - `store.names` is not
               looked at; only read with report_readid.  ValueError unless the offsets cover exactly the calls and the blob
    With ins_alt / rnames `store` needs nothing but `chroms` and `strands`.
    route      None (DEFAULT_ROUTE), "host" - csv_vcf_emit / csv_vcf_emit_ref, the thread team; "device" - csv_vcf_emit_device on `ctx`
               (an engine.Context): the records are written by k_vcf_write; "core" - csv_vcf_emit_core_host, the
               device's record rule with one lane on the host, for checks.  The text is the same on every route.  On "device" and "core"
               the REF bases of every kind of reference come per call: csv_vcf_ref_ranges plus the reference's own gather.
    from_pool  (route="device") (pick, clip): the ALT bases of the INS calls and, with report_readid, the RNAMES text are gathered from
               the context's kept pool rebuild inside the call and never come down - pick / clip per INS call in call order, as
               rebuild.alt_gather takes them (None with ignore_sequence); the read names come from the result's support lists
    keep       (route="device") bytes that stand in front of the records (a VCF header; b"" for none): the text stays in device memory
               and a KeptText comes back in its place - (KeptText, svid)
    timings    a dict that receives ms_emit_kernels on the device route
    """
    route = DEFAULT_ROUTE if route is None else route
    if route not in ROUTES:
        raise ValueError("route must be one of %s, not %r" % (", ".join(ROUTES), route))
    if route == "device" and ctx is None:
        raise ValueError("emit_records: route='device' needs ctx")
    if route != "device" and (from_pool is not None or keep is not None):
        raise ValueError("emit_records: from_pool and keep belong to route='device'")
    L = lib()
    t = res.trimmed()
    n = res.n_calls
    segs = np.ascontiguousarray(segments, dtype=_abi.SEGMENT_DTYPE)
    call_type = segs["svtype"][t["call_seg"]] if n else np.zeros(0, np.int32)
    nch = len(store.chroms)
    names = (C.c_char_p * nch)(*[c.encode() for c in store.chroms])
    from .fasta import BgzfReference, Reference
    line_bases = line_width = None
    bgzf_ref = isinstance(reference, BgzfReference)
    if bgzf_ref:
        ref_idx = np.array([reference.index.get(c, -1) for c in store.chroms], np.int64)
        seqs = (C.c_char_p * nch)()
        clen = np.array([int(reference.length[i]) if i >= 0 else 0 for i in ref_idx], np.int64)
        seq_bytes = reference
    elif isinstance(reference, Reference):
        ent = [reference.contig(c) if c in reference else (0, 0, 0, 0) for c in store.chroms]
        seqs = (C.c_void_p * nch)(*[e[0] or None for e in ent])
        clen = np.array([e[1] for e in ent], np.int64)
        line_bases = np.array([e[2] for e in ent], np.int32)
        line_width = np.array([e[3] for e in ent], np.int32)
        seq_bytes = reference                              # (kept alive below)
    else:
        seq_bytes = [None if reference is None or c not in reference else
                     (reference[c] if isinstance(reference[c], bytes) else reference[c].encode()) for c in store.chroms]
        seqs = (C.c_char_p * nch)(*seq_bytes)
        clen = np.array([0 if s is None else len(s) for s in seq_bytes], np.int64)
    order = sorted(range(nch), key=lambda i: store.chroms[i])
    rank = np.zeros(nch, np.int32)
    rank[order] = np.arange(nch, dtype=np.int32)
    # inserted sequences of INS calls, sliced to SVLEN
    alt_blob, alt_off = None, None
    rn_blob, rn_off = None, None
    pooled = from_pool is not None
    if pooled:
        if ins_alt is not None or rnames is not None:
            raise ValueError("emit_records: from_pool takes the place of ins_alt and rnames")
        if n and report_readid and (t["support_sig"] is None or t["support_off"] is None):
            raise ValueError("emit_records: report_readid needs the support lists (the result was made with CSV_OUT_NO_SUPPORT_LIST)")
    elif ins_alt is not None and not ignore_sequence:
        ins = np.flatnonzero(call_type == _abi.INS)
        alt_blob, took = ins_alt
        took = np.asarray(took, np.int64)
        if took.shape != (len(ins),) or (took < 0).any() or int(took.sum()) != len(alt_blob):
            raise ValueError("emit_records: ins_alt must hold one length per INS call (%d) that add up to its blob (%d bytes)" % (len(ins), len(alt_blob)))
        alt_blob = bytes(alt_blob)
        alt_off = np.zeros(n + 1, np.int64)
        alt_off[ins + 1] = took
        np.cumsum(alt_off, out=alt_off)
    elif n and not ignore_sequence and (call_type == _abi.INS).any() and t["seq_pick"] is None:
        raise ValueError("emit_records: the result carries no seq_pick (a slim result without that field): INS records need it unless ignore_sequence")
    if rnames is not None and report_readid:
        rn_blob, rn_off = rnames
        rn_off = np.ascontiguousarray(rn_off, np.int64)
        if rn_off.shape != (n + 1,) or rn_off[0] != 0 or (np.diff(rn_off) < 0).any() or int(rn_off[-1]) != len(rn_blob):
            raise ValueError("emit_records: rnames must hold n_calls + 1 = %d offsets that start at 0, do not decrease and end at its blob (%d bytes)" % (n + 1, len(rn_blob)))
        rn_blob = bytes(rn_blob)
    elif n and report_readid and (t["support_sig"] is None or t["support_off"] is None):
        raise ValueError("emit_records: report_readid needs the support lists (the result was made with CSV_OUT_NO_SUPPORT_LIST)")
    if not pooled and ins_alt is None and n and not ignore_sequence and (call_type == _abi.INS).any():
        from . import _cols_native as cn                     # (built by the same make as the library; no Python fallback)
        ins = np.flatnonzero(call_type == _abi.INS)
        pick = np.ascontiguousarray(t["seq_pick"][ins], np.int64)
        ln = np.ascontiguousarray(t["bp2"][ins], np.int64)
        table = store.ins_seq
        if table is None:
            if store.names.names is not None:
                store.sequence(0)                             # (raises: real read names but no inserted sequences)
            ln = np.minimum(store.aux[pick].astype(np.int64), ln)      # synthetic stores: 'ACGT' repeated to the aux length
        from .columns import SpanList
        if isinstance(table, SpanList):                       # (a task store built from the reference's pickle: spans of the mapped file)
            alt_blob, took = table.join(pick, ln)
        else:
            took = np.empty(len(ins), np.int64)
            alt_blob = cn.clip_join(table, pick, ln, took)    # b"".join(sequence(pick)[:SVLEN]) in C (GT:297-309)
        alt_off = np.zeros(n + 1, np.int64)
        alt_off[ins + 1] = took
        np.cumsum(alt_off, out=alt_off)
    if not pooled and rnames is None and n and report_readid:
        nm = store.names.take(store.read_id[t["support_sig"]])
        so = t["support_off"].tolist()
        rn_blob, rn_off = _csr([",".join(nm[so[c]:so[c + 1]]) for c in range(n)])
    gl = t["gl_idx"]                                      # (a slim result may leave it out: no call is genotyped then)
    keys = np.unique(gl[gl >= 0]).astype(np.int32) if (n and gl is not None) else np.zeros(0, np.int32)
    gl_strs = (C.c_char_p * max(1, len(keys)))(*["\t".join(gl_fields(int(k))).encode() for k in keys])
    strands = (C.c_char_p * len(store.strands))(*[s.encode() for s in store.strands])
    if svid is None:
        svid = np.zeros(5, np.int64)
    vin = VcfIn(res=C.pointer(res.c), seg=segs.ctypes.data, n_seg=len(segs), n_chrom=nch,
                chrom_name=names, chrom_seq=C.cast(seqs, C.POINTER(C.c_char_p)), chrom_len=clen.ctypes.data, chrom_rank=rank.ctypes.data,
                chrom_line_bases=None if line_bases is None else line_bases.ctypes.data,
                chrom_line_width=None if line_width is None else line_width.ctypes.data,
                ins_alt=alt_blob, ins_alt_off=None if alt_off is None else alt_off.ctypes.data,
                rnames=rn_blob, rnames_off=None if rn_off is None else rn_off.ctypes.data,
                strand_name=strands, gl_key=keys.ctypes.data, gl_str=gl_strs, n_gl=len(keys),
                min_size=min_size, max_size=max_size, genotype=int(bool(genotype)), report_readid=int(bool(report_readid)),
                ignore_sequence=int(bool(ignore_sequence)))
    ref_blob = ref_off = None
    per_call = bgzf_ref or route != "host"
    if per_call:
        beg, end, chrom = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int32)
        rc = L.csv_vcf_ref_ranges(C.byref(vin), beg.ctypes.data, end.ctypes.data, chrom.ctypes.data)
        if rc != _abi.OK:
            raise RuntimeError("csv_vcf_emit: %s (a reference sequence is missing or too short?)" % _abi.ERR_NAME.get(rc, rc))
        ref_blob, ref_off = np.zeros(0, np.uint8), np.zeros(n + 1, np.int64)
        if not bgzf_ref:
            ref_blob, ref_off = _host_ref_gather(store, reference, seq_bytes, chrom, beg, end)
        elif (end > beg).any():                            # (an empty range reads nothing of any contig: it is asked of contig 0)
            idx = np.where(end > beg, ref_idx[chrom], 0)
            ref_blob, ref_off = reference.gather(idx, beg, end, ctx=ref_ctx, route=ref_route)
            ref_off = np.ascontiguousarray(ref_off, np.int64)
    if route == "device":
        return _emit_device(L, ctx, vin, n, ref_blob, ref_off, store, svid, from_pool, keep, as_bytes, timings,
                            (len(alt_blob) if alt_blob else 0) + (len(rn_blob) if rn_blob else 0), ignore_sequence)
    cap = 256 * max(n, 1) + (len(alt_blob) if alt_blob else 0) + (len(rn_blob) if rn_blob else 0) + (len(ref_blob) if ref_blob is not None else 0) + 4096
    for _ in range(2):
        buf = getattr(_TLS, "buf", None)
        if buf is None or len(buf) < cap:                 # (recycled: a fresh zero-filled buffer per call costs as much as the emitter)
            buf = _TLS.buf = np.empty(cap, np.uint8)
        need = C.c_int64(0)
        sv = svid.copy()
        if route == "core":
            rc = L.csv_vcf_emit_core_host(C.byref(vin), ref_blob.ctypes.data if len(ref_blob) else None, ref_off.ctypes.data, buf.ctypes.data, len(buf), C.byref(need), sv.ctypes.data)
        elif bgzf_ref:
            rc = L.csv_vcf_emit_ref(C.byref(vin), ref_blob.ctypes.data if len(ref_blob) else None, ref_off.ctypes.data, C.cast(buf.ctypes.data, C.c_char_p), len(buf), C.byref(need),
                                    sv.ctypes.data)
        else:
            rc = L.csv_vcf_emit(C.byref(vin), C.cast(buf.ctypes.data, C.c_char_p), len(buf), C.byref(need), sv.ctypes.data)
        if rc == _abi.E_CAPACITY:
            cap = need.value + 16
            continue
        if rc != _abi.OK:
            raise RuntimeError("csv_vcf_emit: %s (a reference sequence is missing or too short?)" % _abi.ERR_NAME.get(rc, rc))
        svid[:] = sv
        if as_view:
            return memoryview(buf)[:need.value], svid
        raw = buf[:need.value].tobytes()
        return (raw if as_bytes else raw.decode()), svid
    raise RuntimeError("csv_vcf_emit: capacity retry failed")


def _emit_device(L, ctx, vin, n, ref_blob, ref_off, store, svid, from_pool, keep, as_bytes, timings, string_bytes, ignore_sequence):
    """csv_vcf_emit_device with its capacity negotiated -> (text or KeptText, svid)"""
    flags, n_pick, pick, clip = 0, 0, None, None
    if from_pool is not None:
        flags |= RNAMES_FROM_POOL
        if not ignore_sequence:
            pick, clip = (np.ascontiguousarray(a, np.int64) for a in from_pool)
            if pick.shape != clip.shape or pick.ndim != 1:
                raise ValueError("emit_records: from_pool must be (pick, clip), one entry each per INS call")
            flags |= ALT_FROM_POOL
            n_pick = len(pick)
    prefix = b"" if keep is None else bytes(keep)
    if keep is not None:
        flags |= KEEP_TEXT
    rows, name_chrom = np.zeros((max(n, 1), 4), np.int64), np.zeros(max(len(store.chroms), 1), np.int32)
    n_rows, n_names, need, ms = C.c_int64(0), C.c_int32(0), C.c_int64(0), C.c_double(0)
    ptr = lambda a: a.ctypes.data if a is not None and len(a) else None            # noqa: E731
    cap = 0 if keep is not None else 256 * max(n, 1) + string_bytes + len(ref_blob) + 4096
    for _ in range(3):
        buf = None if keep is not None else np.empty(cap, np.uint8)
        sv = svid.copy()
        rc = L.csv_vcf_emit_device(ctx._h, C.byref(vin), ptr(ref_blob), ref_off.ctypes.data, n_pick, ptr(pick), ptr(clip), prefix if prefix else None, len(prefix), flags,
                                   None if buf is None else buf.ctypes.data, cap, C.byref(need), sv.ctypes.data, rows.ctypes.data, len(rows), C.byref(n_rows),
                                   name_chrom.ctypes.data, C.byref(n_names), C.byref(ms))
        if rc == _abi.E_CAPACITY and keep is None:
            cap = need.value + 16
            continue
        ctx._check(rc)
        svid[:] = sv
        if timings is not None:
            timings["ms_emit_kernels"] = timings.get("ms_emit_kernels", 0.0) + ms.value
        if keep is not None:
            return KeptText(ctx, need.value, rows[:n_rows.value].copy(), [store.chroms[i] for i in name_chrom[:n_names.value].tolist()], ms.value), svid
        raw = buf[:need.value].tobytes()
        return (raw if as_bytes else raw.decode()), svid
    raise RuntimeError("csv_vcf_emit_device: capacity retry failed")


# ------------------------------------------------------------------------------------ the header
SOURCE = "cutesv_amd (cuteSV-2.1.4)"
FILE_DATE_FORMAT = "%Y-%m-%d %H:%M:%S %w-%Z"              # the reference's fileDate (cuteSV_Description.py:270)
COLUMNS = ("#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT")

# (kind, ID, Number, Type, Description) in the order cuteSV v2.1.4 declares them; Number / Type None: the kind has none
HEADER_FIELDS = (
    ("ALT", "INS", None, None, "Insertion of novel sequence relative to the reference"),
    ("ALT", "DEL", None, None, "Deletion relative to the reference"),
    ("ALT", "DUP", None, None, "Region of elevated copy number relative to the reference"),
    ("ALT", "INV", None, None, "Inversion of reference sequence"),
    ("ALT", "BND", None, None, "Breakend of translocation"),
    ("INFO", "PRECISE", "0", "Flag", "Precise structural variant"),
    ("INFO", "IMPRECISE", "0", "Flag", "Imprecise structural variant"),
    ("INFO", "SVTYPE", "1", "String", "Type of structural variant"),
    ("INFO", "SVLEN", "1", "Integer", "Difference in length between REF and ALT alleles"),
    ("INFO", "CHR2", "1", "String", "Chromosome for END coordinate in case of a translocation"),
    ("INFO", "END", "1", "Integer", "End position of the variant described in this record"),
    ("INFO", "CIPOS", "2", "Integer", "Confidence interval around POS for imprecise variants"),
    ("INFO", "CILEN", "2", "Integer", "Confidence interval around inserted/deleted material between breakends"),
    ("INFO", "RE", "1", "Integer", "Number of read support this record"),
    ("INFO", "STRAND", "A", "String", "Strand orientation of the adjacency in BEDPE format (DEL:+-, DUP:-+, INV:++/--)"),
    ("INFO", "RNAMES", ".", "String", "Supporting read names of SVs (comma separated)"),
    ("INFO", "AF", "A", "Float", "Allele Frequency."),
    ("FILTER", "q5", None, None, "Quality below 5"),
    ("FORMAT", "GT", "1", "String", "Genotype"),
    ("FORMAT", "DR", "1", "Integer", "# High-quality reference reads"),
    ("FORMAT", "DV", "1", "Integer", "# High-quality variant reads"),
    ("FORMAT", "PL", "G", "Integer", "# Phred-scaled genotype likelihoods rounded to the closest integer"),
    ("FORMAT", "GQ", "1", "Integer", "# Genotype quality"),
)


def header_text(contigs, sample, argv, now=None):
    """The VCF header cuteSV v2.1.4 writes in front of the records (cuteSV_Description.py:265-305 and the column line of main
    script :1217) -> str.  contigs: [(name, length)] in the BAM header's order; sample: the last column's name; argv: the command
    line's arguments; now: a time.struct_time (default: the local time).  Line for line the reference's, except ##source (this
    project, and the version it restates), ##fileDate (the reference's format, this run's time) and ##CommandLine (this program's
    name)."""
    import time
    lines = ["##fileformat=VCFv4.2", "##source=" + SOURCE, "##fileDate=" + time.strftime(FILE_DATE_FORMAT, time.localtime() if now is None else now)]
    lines += ["##contig=<ID=%s,length=%d>" % (name, length) for name, length in contigs]
    for kind, ident, number, typ, desc in HEADER_FIELDS:
        typed = "" if number is None else "Number=%s,Type=%s," % (number, typ)
        lines.append('##%s=<ID=%s,%sDescription="%s">' % (kind, ident, typed, desc))
    lines.append('##CommandLine="cutesv_amd %s"' % " ".join(argv))
    lines.append("\t".join(COLUMNS + (sample,)))
    return "\n".join(lines) + "\n"


def emit_stage(results, reference, **kw):
    """VCF body text of a `resolve.cluster_stage(..., lazy=True)` result ({chr: rows.LazyRows}): the native emitter reads the
    structure of arrays the lazy rows are backed by - no row strings are created on the way (GT:242-467, main script
    :1208-1237).  Keyword arguments as emit_records."""
    backs = {id(b): b for b in (v.backing() if hasattr(v, "backing") else None for v in results.values()) if b is not None}
    if len(backs) != 1 or any(not hasattr(v, "backing") or v.backing() is None for v in results.values()):
        raise ValueError("emit_stage needs the untouched result of ONE cluster_stage(lazy=True) call")
    b = next(iter(backs.values()))
    # "untouched" is checked, not assumed (advisor, r05): the emitter writes EVERY call of the backing's result, so the rows
    # on offer must be exactly those calls - each once, none dropped with a chromosome, a task or a filtered row
    idx = np.concatenate([v.call_indices() for v in results.values()]) if results else np.zeros(0, np.int64)
    n = b.res.n_calls
    if len(idx) != n or (n and not np.array_equal(np.sort(idx), np.arange(n))):
        raise ValueError("emit_stage: the rows on offer are not exactly the calls of the stage's result (%d rows, %d calls): rows were "
                         "removed, repeated or filtered - write those with emit_records on a result of their own, or from the row lists" % (len(idx), n))
    return emit_records(b.store, b.segments, b.res, reference, **kw)
