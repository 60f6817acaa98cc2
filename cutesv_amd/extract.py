"""The CIGAR scan of cuteSV's extraction step on the GPU.

`cigar_signatures` is the face of `csv_cigar_signatures` (cutesv_amd/csrc/cigar.hip.h): the flat BAM-encoded CIGAR array
of a batch of reads -> the INS / DEL signatures parse_read + generate_combine_sigs (main script :606-655, :515-575) make
of them.  `candidates` turns the flat result into the reference's candidate tuples (the inserted sequence is cut out of
the reads' query sequences here: the bases never travel to the GPU).  `split_signatures` is the face of
`csv_split_signatures` (split.hip.h): organize_split_signal + analysis_split_read (:50-513) on the numbers of a batch of
primary alignments and SA-tag entries.  For a driver with pysam, BAM decode, the SA text (`encode_split_reads`) and
everything else of the extraction stay in Python, as north_star has it: a driver would collect
`read.cigartuples`, `read.reference_start`, `read.mapq >= min_mapq and read.query_length >= min_read_len` for a task's
reads, make one call here, and extend candidate["INS"] / candidate["DEL"] with the result.  `single_pipe_bam` is the same task
body fed from a BAM file by the native reader (cutesv_amd/bam.py): no pysam and no object per record.  With sa="device" the
SA text is parsed where the decode left it (`split_inputs_bam`, the face of `csv_bam_split_inputs`, sa.hip.h) and
`task_to_pool` takes a task's region of the file to rows of the context's device-resident pool with no Python per record.
With gates="device" the task gates - `_gates`: secondary records, the task's start, --include_bed, read length, MAPQ - are evaluated
by one kernel where the decoded columns are (`task_gates`, the face of `csv_bam_task_gates`, gates.hip.h) and the scans read them there.
"""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import (CigarIn, CigarOut, SplitIn, SplitOut, SaIn, SaOut,      # noqa: F401  (the mirrors live in _abi)
                   CIGAR_OUT as _OUT, SPLIT_OUT as _SPLIT_OUT, SA_CALL as _SA_CALL, SA_ENT as _SA_ENT)
from ._lib import lib


def encode_cigars(cigartuples_per_read):
    """[[(op, oplen), ...] per read] (pysam's read.cigartuples) -> (cig_off int64[n + 1], cigar uint32[n_ops]) in the BAM
    encoding oplen << 4 | op"""
    # (pysam returns None for a record without a CIGAR - an unmapped mate that fetch() still yields; the reference skips
    # such a read through its mapq gate, main script :614, and carries on)
    cigartuples_per_read = [c if c is not None else () for c in cigartuples_per_read]
    lens = np.fromiter((len(c) for c in cigartuples_per_read), np.int64, len(cigartuples_per_read))
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    flat = np.empty(int(off[-1]), np.uint32)
    k = 0
    for c in cigartuples_per_read:
        for op, ln in c:
            flat[k] = (int(ln) << 4) | int(op)
            k += 1
    return off, flat


def _negotiate(fn, handle, cin, out_type, table, classes, give, check, what, longer=()):
    """The one capacity-negotiating call of this module: fn([handle,] &cin, &out) with caller-allocated result columns.
    table: the out-struct's columns (name, dtype, capacity class); classes: {class: (capacity field, count field, first capacity,
    what a retry adds to the count)}; give: the columns handed over - the others stay NULL and empty, their capacities are still
    passed; longer: columns with one entry more than their class.  On CSV_E_CAPACITY the capacities are re-made from the counts
    of the failed call and it is repeated once.  -> ({column: array cut to its count}, out-struct)"""
    caps = {k: c[2] for k, c in classes.items()}
    for _ in range(2):
        arrs = {name: np.zeros(caps[k] + (name in longer) if name in give else 0, dt) for name, dt, k in table}
        cout = out_type(**{c[0]: caps[k] for k, c in classes.items()}, **{name: a.ctypes.data for name, a in arrs.items() if len(a)})
        rc = fn(handle, C.byref(cin), C.byref(cout)) if handle is not None else fn(C.byref(cin), C.byref(cout))
        if rc == _abi.E_CAPACITY:
            caps = {k: int(getattr(cout, c[1])) + c[3] for k, c in classes.items()}
            continue
        check(rc)
        n = {k: int(getattr(cout, c[1])) for k, c in classes.items()}
        return {name: arrs[name][:n[k] + (name in longer)] if name in give else arrs[name] for name, _, k in table}, cout
    raise RuntimeError("%s: capacity retry failed" % what)


def upload_read_sequences(ctx, data, off=None, l_seq=None, want=None):
    """csv_seq_reads_upload: the 4-bit sequences of the current batch's reads - read i = the (l_seq[i] + 1) // 2 bytes at
    data[off[i]:], high nibble first (data: uint8 array or bytes; for a bam.Chunk: chunk.host and chunk.sequence_columns()) - go to
    the device, where the calls with pool=dict(..., seqs=True) cut the INS rows' bases out of them.  want: per read, 0 = its bases
    are not needed (and are not sent).  They stay until the next upload or bam.decode.  The library checks every range
    (CsvError E_INVALID, nothing changes).
    data = a bam.FramedChunk (off and l_seq None): csv_seq_reads_framed takes the sequences out of its device image."""
    want = None if want is None else np.ascontiguousarray(want, np.uint8)
    if getattr(data, "framed", False):
        chunk = data
        if not chunk.fetched and chunk.ctx is ctx:
            chunk.check()
            if want is not None and len(want) != chunk.n:
                raise ValueError("one offset, one length and (with `want`) one flag per read are expected")
            ctx._check(lib().csv_seq_reads_framed(ctx._h, None if want is None or not chunk.n else want.ctypes.data))
            return
        off, l_seq = chunk.sequence_columns()
        data = chunk.host
    data = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, np.uint8)
    off = np.ascontiguousarray(off, np.int64); l_seq = np.ascontiguousarray(l_seq, np.int32)
    if len(off) != len(l_seq) or (want is not None and len(want) != len(off)):
        raise ValueError("one offset, one length and (with `want`) one flag per read are expected")
    n = len(off)
    ctx._check(lib().csv_seq_reads_upload(ctx._h, n, data.ctypes.data if len(data) else None, len(data), off.ctypes.data if n else None,
                                          l_seq.ctypes.data if n else None, None if want is None or not n else want.ctypes.data))


def seq_option(ctx, whole_image):
    """csv_seq_option(CSV_SEQ_OPT_WHOLE_IMAGE): a measurement aid - upload_read_sequences sends the image whole instead of packing
    the wanted reads (scripts/ins_seq_stage.py compares the two)"""
    ctx._check(lib().csv_seq_option(ctx._h, _abi.SEQ_OPT_WHOLE_IMAGE, 1 if whole_image else 0))


def seq_info(ctx):
    """figures of the context's last sequence upload and last seqs=True call (csv_seq_info)"""
    o = _abi.SeqInfo()
    ctx._check(lib().csv_seq_info_get(ctx._h, C.byref(o)))
    return {k: getattr(o, k) for k, _ in _abi.SeqInfo._fields_ if k != "reserved"}


def _to_pool(cin, pool):
    """CSV_CG_TO_POOL on a csv_cigar_in / csv_split_in: the results also become rows of the context's pool; with seqs=True the INS
    rows' bases go to its sequence pool (CSV_CG_SEQ_TO_POOL).
    -> the converted query_len column (or None): the caller holds it until the call has returned"""
    qlen = None if pool.get("query_len") is None else np.ascontiguousarray(pool["query_len"], np.int32)
    cin.flags |= _abi.CG_TO_POOL | (_abi.CG_SEQ_TO_POOL if pool.get("seqs") else 0)
    cin.read_base = int(pool["read_base"])
    cin.query_len = None if qlen is None else qlen.ctypes.data
    return qlen


def _run(fn, handle, cig_off, cigar, ref_start, use, min_siglength, merge_ins_threshold, merge_del_threshold, check, pool=None, host_outputs=True,
         from_bam=None):
    use_gates = isinstance(use, str)
    if use_gates and (use != "gates" or from_bam is None):
        raise ValueError("use: an array, None or - with from_bam - 'gates', not %r" % (use,))
    use = None if use is None or use_gates else np.ascontiguousarray(use, np.uint8)
    if from_bam is not None:                              # CSV_CG_FROM_BAM: the three columns are on the device already (bam.decode)
        n, n_ops = int(from_bam["n"]), int(from_bam["n_ops"])
        cin = CigarIn(n_reads=n, flags=_abi.CG_FROM_BAM | (_abi.CG_USE_FROM_GATES if use_gates else 0))
    else:
        cig_off = np.ascontiguousarray(cig_off, np.int64); cigar = np.ascontiguousarray(cigar, np.uint32)
        ref_start = np.ascontiguousarray(ref_start, np.int64)
        n, n_ops = len(ref_start), int(cig_off[-1])
        cin = CigarIn(n_reads=n, cig_off=cig_off.ctypes.data, cigar=cigar.ctypes.data if len(cigar) else None, ref_start=ref_start.ctypes.data)
    cin.use = None if use is None else use.ctypes.data
    cin.min_siglength, cin.merge_ins_threshold, cin.merge_del_threshold = int(min_siglength), int(merge_ins_threshold), int(merge_del_threshold)
    qlen = None
    if pool is not None:                                  # the signatures also become rows of the context's pool
        qlen = _to_pool(cin, pool)
        cin.seg_ins, cin.seg_del = int(pool["seg_ins"]), int(pool["seg_del"])
    to_host = host_outputs or pool is None                # (pool only: nothing but the counts comes back)
    cap = max(16, n // 4) if to_host else n_ops + 1
    classes = dict(i=("cap_sig_ins", "n_sig_ins", cap, 1), p=("cap_piece_ins", "n_piece_ins", cap, 1), d=("cap_sig_del", "n_sig_del", cap, 1))
    out, cout = _negotiate(fn, handle, cin, CigarOut, _OUT, classes, [name for name, _, _ in _OUT] if to_host else (), check, "csv_cigar_signatures")
    out["n_sig_ins"], out["n_sig_del"] = int(cout.n_sig_ins), int(cout.n_sig_del)
    out["ms_device"] = float(cout.ms_device)
    return out


def cigar_signatures(ctx, cig_off, cigar, ref_start, use=None, min_siglength=10, merge_ins_threshold=100, merge_del_threshold=0, pool=None, host_outputs=True,
                     from_bam=None):
    """flat CIGARs of a batch of reads -> dict of the signature arrays of csv_cigar_out (defaults: cuteSV_Description.py:123-152).
    pool = dict(seg_ins, seg_del, read_base, query_len=None, seqs=False): the signatures ALSO become rows of the context's device-resident
    pool (CSV_CG_TO_POOL; INS rows in segment seg_ins, DEL rows in seg_del, read index = read_base + index in this batch), in the
    order INS then DEL - what `rebuild.rebuild_pool` sorts without the rows ever crossing PCIe; host_outputs=False (with a pool):
    the arrays of the result stay empty, only the counts come back.  seqs=True: the INS rows' inserted bases are cut out of the
    sequences `upload_read_sequences` left on the device (one per read of this batch; query_len must be their l_seq) into the
    context's sequence pool (`rebuild.seq_pool_get`).
    from_bam = the columns `bam.decode(ctx, chunk)` returned: cig_off / cigar / ref_start are not taken from the arguments (pass
    None) but scanned where that decode left them on the device (CSV_CG_FROM_BAM); `use` is still the caller's - or "gates": the
    USE bit of the column `task_gates` left beside that decode (CSV_CG_USE_FROM_GATES), which then never leaves the device."""
    return _run(lib().csv_cigar_signatures, ctx._h, cig_off, cigar, ref_start, use, min_siglength, merge_ins_threshold, merge_del_threshold, ctx._check, pool=pool,
                host_outputs=host_outputs, from_bam=None if from_bam is None else dict(n=len(from_bam["ref_start"]), n_ops=from_bam["n_ops"]))


def candidates(sig, read_names, query_sequences, chrom):
    """signature arrays -> the reference's candidate tuples (main script :520-575):
    INS (pos, len, read, seq, "INS", chr), DEL (pos, len, read, "DEL", chr), in read order"""
    ins, dele = [], []
    qo, ql = sig["piece_qoff"].tolist(), sig["piece_len"].tolist()
    for r, pos, ln, p0, npc in zip(sig["ins_read"].tolist(), sig["ins_pos"].tolist(), sig["ins_len"].tolist(),
                                    sig["ins_piece0"].tolist(), sig["ins_npiece"].tolist()):
        q = query_sequences[r]
        seq = "".join(str(q[qo[p] : qo[p] + ql[p]]) for p in range(p0, p0 + npc))      # read.query_sequence[shift - oplen : shift] (:639-640)
        ins.append((pos, ln, read_names[r], seq, "INS", chrom))
    for r, pos, ln in zip(sig["del_read"].tolist(), sig["del_pos"].tolist(), sig["del_len"].tolist()):
        dele.append((pos, ln, read_names[r], "DEL", chrom))
    return ins, dele


# ------------------------------------------------------------------------------------ split reads (SA tag)
_CIGAR_RE = None


def clip_and_span(cigar_string):
    """acquire_clip_pos (main script :466-481) on the CIGAR text of an SA entry: [leading soft clip, trailing soft clip,
    reference span over M / D / = / X]"""
    global _CIGAR_RE
    if _CIGAR_RE is None:
        import re
        _CIGAR_RE = re.compile(r"(\d+)([MIDNSHP=XB])")
    ops = _CIGAR_RE.findall(cigar_string)
    first = int(ops[0][0]) if ops and ops[0][1] == "S" else 0
    last = int(ops[-1][0]) if ops and ops[-1][1] == "S" else 0
    return first, last, sum(int(n) for n, o in ops if o in "MD=X")


def encode_split_reads(reads, chrom_rank):
    """reads: [(primary_info or [], "chr,pos,strand,CIGAR,mapq,NM;..." SA tag value, query_length)] per read, as parse_read
    (main script :657-679) hands them to organize_split_signal; chrom_rank: {name: rank in Python string order}.
    -> dict of the flat csv_split_in arrays.  This is the text side of the step (the SA tag is a string): it stays here."""
    ent_off = [0]
    cols = {k: [] for k in ("c0", "c1", "f0", "f1", "chr", "mapq", "strand", "primary")}
    read_len = []
    for primary, sa, qlen in reads:
        read_len.append(int(qlen))
        if len(primary) > 0:
            for k, v in zip(("c0", "c1", "f0", "f1"), primary[:4]):
                cols[k].append(int(v))
            cols["chr"].append(chrom_rank[primary[4]]); cols["strand"].append(0 if primary[5] == "+" else 1)
            cols["mapq"].append(0); cols["primary"].append(1)
        for entry in sa.split(";")[:-1]:                       # (:676)
            seq = entry.split(",")
            first, last, span = clip_and_span(seq[3])
            cols["c0"].append(first); cols["c1"].append(last); cols["f0"].append(int(seq[1]) - 1); cols["f1"].append(span)      # (:497)
            cols["chr"].append(chrom_rank[seq[0]]); cols["strand"].append(0 if seq[2] == "+" else 1)
            cols["mapq"].append(int(seq[4])); cols["primary"].append(0)
        ent_off.append(len(cols["c0"]))
    dt = dict(c0=np.int64, c1=np.int64, f0=np.int64, f1=np.int64, chr=np.int32, mapq=np.int32, strand=np.uint8, primary=np.uint8)
    out = {k: np.asarray(v, dt[k]) for k, v in cols.items()}
    out["ent_off"] = np.asarray(ent_off, np.int64); out["read_len"] = np.asarray(read_len, np.int64)
    return out


# ------------------------------------------------------------------------------------ SA text parsed on the device
SA_ST_NUMBER, SA_ST_STRAND, SA_ST_CIGAR, SA_ST_FIELDS, SA_ST_NAME = 1, 2, 4, 8, 16
_SA_STRICT_CIGAR = None


def _sa_number(f, max_digits):
    return 0 < len(f) <= max_digits and f.isdigit()          # (bytes.isdigit: ASCII digits only)


def sa_names(names):
    """the contig names of a name table as sa_status takes them: a frozenset of bytes, made once for many values"""
    return frozenset(n.encode() if isinstance(n, str) else n for n in names)


def sa_status(value, names):
    """The strict grammar of the device parser (sa.hip.h) on the host: the status byte csv_bam_split_inputs gives a call with
    this SA value (bytes, or str) when `names` are the contigs of its name table (`sa_names(...)`; any other iterable of
    names is converted on every call).  0: the device parses the value itself, exactly as encode_split_reads would;
    anything else: the call is flagged and goes through encode_split_reads."""
    global _SA_STRICT_CIGAR
    if _SA_STRICT_CIGAR is None:
        import re
        _SA_STRICT_CIGAR = re.compile(rb"(?:([0-9]{1,18})([MIDNSHP=XB]))+")
    if isinstance(value, str):
        value = value.encode()
    known = names if isinstance(names, frozenset) else sa_names(names)
    st = 0
    for entry in value.split(b";")[:-1]:
        f = entry.split(b",")
        if f[0] not in known:
            st |= SA_ST_NAME
        if len(f) > 1 and not _sa_number(f[1], 18):
            st |= SA_ST_NUMBER
        if len(f) > 2 and len(f[2]) != 1:
            st |= SA_ST_STRAND
        if len(f) > 3 and f[3] != b"*":
            if not _SA_STRICT_CIGAR.fullmatch(f[3]):
                st |= SA_ST_CIGAR
            elif clip_and_span(f[3].decode())[2] > 1 << 62:      # (the device sums in 64 bits)
                st |= SA_ST_CIGAR
        if len(f) > 4 and not _sa_number(f[4], 9):
            st |= SA_ST_NUMBER
        if len(f) < 5:
            st |= SA_ST_FIELDS
    return st


def _name_table(chrom_rank):
    """chrom_rank -> (names back to back in byte order, offsets, the caller's ranks in that order)"""
    items = sorted((k.encode(), int(r)) for k, r in chrom_rank.items())
    off = np.zeros(len(items) + 1, np.int64)
    if items:
        np.cumsum([len(k) for k, _ in items], out=off[1:])
    blob = np.frombuffer(b"".join(k for k, _ in items), np.uint8)
    return blob, off, np.asarray([r for _, r in items], np.int32)


def split_inputs_bam(ctx, chunk, cols, sel, chrom_rank, chrom, min_mapq, host_outputs=True, gate_bits=None):
    """csv_bam_split_inputs on the context's last `bam.decode(ctx, chunk)` (= cols): the SA tags of the records with sel != 0,
    parsed where the decode left them -> the dict `encode_split_reads` returns for those reads built the old way
    (_primary_info + Chunk.sa_values; same keys, same dtypes), one call per (selected record, SA tag), plus call_rec (the
    call's record in the chunk), status (per call, see sa_status: a flagged call has NO entries here and is the caller's to
    send through encode_split_reads), n_calls, n_entries, n_flagged, ms_device.  The columns also stay on the device until
    the context's next decode / split inputs: split_signatures(ctx, None, from_bam=<this dict>) analyses them there.
    host_outputs=False: only call_rec and status come back (the entry columns and ent_off / read_len stay empty).
    sel="gates": the selection is the SEL bit of the column `task_gates` left beside the decode (CSV_SA_SEL_FROM_GATES) and is not
    sent; gate_bits = the bytes task_gates returned, for the one look the host takes at the selection (a contig without a rank)."""
    n = chunk.n
    sel_gates = isinstance(sel, str)
    if sel_gates:
        if sel != "gates" or gate_bits is None:
            raise ValueError("sel: an array or 'gates' with gate_bits=, not %r" % (sel,))
        sel = (np.asarray(gate_bits) & _abi.GATE_SEL) != 0
    sel = np.ascontiguousarray(sel, np.uint8)
    assert len(sel) == n
    if chrom not in chrom_rank and bool(np.any((sel != 0) & (np.asarray(cols["mapq"]) >= min_mapq))):
        raise KeyError(chrom)                              # (encode_split_reads looks the primary's contig up, too)
    blob, name_off, name_rank = _name_table(chrom_rank)
    sin = SaIn(n_records=n, sel=sel.ctypes.data if n and not sel_gates else None, flags=_abi.SA_SEL_FROM_GATES if sel_gates else 0, min_mapq=int(min_mapq), task_rank=int(chrom_rank.get(chrom, -1)), n_names=len(name_rank),
               names=blob.ctypes.data if len(blob) else None, name_bytes=len(blob), name_off=name_off.ctypes.data, name_rank=name_rank.ctypes.data if len(name_rank) else None)
    cap_calls = int(cols["n_sa"])
    # an entry the device accepts has at least ten bytes ("a,1,+,*,0;"), a flagged call has none: plus one primary entry per call
    cap_ent = int((cols["sa_end"] - cols["sa_beg"]).sum()) // 10 + cap_calls if cap_calls else 0
    cols_out = _SA_CALL + _SA_ENT
    out, sout = _negotiate(lib().csv_bam_split_inputs, ctx._h, sin, SaOut, cols_out, dict(c=("cap_calls", "n_calls", cap_calls, 0), e=("cap_entries", "n_entries", cap_ent, 0)),
                           [k for k, _, _ in cols_out] if host_outputs else ("call_rec", "status"), ctx._check, "csv_bam_split_inputs", longer=("ent_off",))
    if host_outputs:
        out.update({k: out[k].copy() for k, _, _ in _SA_ENT})
    out.update(n_calls=int(sout.n_calls), n_entries=int(sout.n_entries), n_flagged=int(sout.n_flagged), ms_device=float(sout.ms_device))
    return out


def _flagged_reads(chunk, cols, si, sel, chrom, min_mapq):
    """the calls `split_inputs_bam` flagged, as encode_split_reads takes them: (call indices, [(primary_info, SA value, query_length)])"""
    calls = np.flatnonzero(si["status"])
    per_rec = np.where(np.asarray(sel) != 0, np.diff(cols["sa_off"]), 0)
    first = np.concatenate([[0], np.cumsum(per_rec)])          # first call of every record
    reads = []
    for k in calls.tolist():
        i = int(si["call_rec"][k])
        t = int(cols["sa_off"][i]) + (k - int(first[i]))
        primary = _primary_info(int(cols["flag"][i]), cols["mapq"][i] >= min_mapq, int(cols["clip_left"][i]), int(cols["clip_right"][i]),
                                int(cols["query_len"][i]), int(cols["ref_start"][i]), int(cols["ref_end"][i]), chrom)
        reads.append((primary, chunk.text(cols["sa_beg"][t], cols["sa_end"][t]), int(cols["query_len"][i])))
    return calls, reads


def _run_split(fn, handle, enc, sv_size, min_mapq, max_split_parts, max_size, check, pool=None, from_bam=None, host_outputs=True):
    if from_bam is not None:                              # CSV_SP_FROM_BAM: calls and entry columns are on the device already (split_inputs_bam)
        n, n_ent = int(from_bam["n_calls"]), int(from_bam.get("n_entries", 0))
        sin = SplitIn(sv_size=int(sv_size), max_size=int(max_size), min_mapq=int(min_mapq), max_split_parts=int(max_split_parts), flags=_abi.SP_FROM_BAM)
    else:
        a = {k: np.ascontiguousarray(v) for k, v in enc.items()}
        n, n_ent = len(a["read_len"]), int(a["ent_off"][-1])
        ptr = lambda x: x.ctypes.data if len(x) else None                      # noqa: E731
        sin = SplitIn(n_reads=n, ent_off=a["ent_off"].ctypes.data, read_len=ptr(a["read_len"]), c0=ptr(a["c0"]), c1=ptr(a["c1"]), f0=ptr(a["f0"]),
                      f1=ptr(a["f1"]), chr=ptr(a["chr"]), mapq=ptr(a["mapq"]), strand=ptr(a["strand"]), primary=ptr(a["primary"]),
                      sv_size=int(sv_size), max_size=int(max_size), min_mapq=int(min_mapq), max_split_parts=int(max_split_parts))
    qlen = None
    if pool is not None:                                  # the candidates also become rows of the context's pool
        qlen = _to_pool(sin, pool)
        sin.pool_seg_base = (C.c_int32 * 5)(*[int(x) for x in pool["seg_base"]])
        if pool.get("seqs") and from_bam is None:         # the strand of every read, beside the uploaded sequences (from_bam: the decode's flags)
            rev = np.zeros(n, np.uint8) if pool.get("query_reverse") is None else np.ascontiguousarray(pool["query_reverse"], np.uint8)
            if len(rev) != n:
                raise ValueError("query_reverse: one entry per read is expected")
            check(lib().csv_seq_query_reverse(handle, n, rev.ctypes.data if n else None))
    to_host = host_outputs or pool is None                # (pool only: nothing but the count comes back; no entry yields more than 12 candidates)
    out, sout = _negotiate(fn, handle, sin, SplitOut, _SPLIT_OUT, dict(n=("cap", "n", max(16, 2 * n) if to_host else 12 * n_ent, 1)),
                           [name for name, _, _ in _SPLIT_OUT] if to_host else (), check, "csv_split_signatures")
    out["ms_device"] = float(sout.ms_device)
    if not to_host:
        out["n"] = int(sout.n)
    return out


def split_signatures(ctx, enc, sv_size=30, min_mapq=20, max_split_parts=7, max_size=100000, pool=None, from_bam=None, host_outputs=True):
    """flat split-read entries of a batch of reads (encode_split_reads) -> dict of the candidate arrays of csv_split_out
    (defaults: cuteSV_Description.py: --min_size 30, --min_mapq 20, --max_split_parts 7, --max_size 100000).
    pool = dict(seg_base=[segment of chromosome rank 0 for kind DEL, INS, DUP, INV, TRA], read_base, query_len=None, seqs=False,
    query_reverse=None): the candidates ALSO become rows of the context's device-resident pool (`pool_rows_of_split` is the same
    mapping on the host); host_outputs=False (with a pool): the arrays of the result stay empty and the result gains the key `n`,
    the number of candidates.  seqs=True: the INS candidates' bases and x.5 flags go to the context's sequence pool, cut out of the
    sequences `upload_read_sequences` left on the device (one per read of `enc`); query_reverse[r] = 1: read r's record has flag 16,
    so the query parse_read analyses is the reverse complement of the uploaded sequence (None: no read is reversed).
    An INS candidate's c:d is the reference's query[c:d] and has Python's slice meaning wherever it becomes a length (the pool row's
    aux) or bytes (the sequence pool): a negative bound counts from the read's end, both are clamped to [0, read length], start >= stop
    is empty.  A short first segment that overlaps the next one on the reference gives c < 0; such a batch is not refused.
    from_bam = the dict `split_inputs_bam` returned (pass enc=None): the reads are its calls and the entry columns are read where
    it left them on the device (CSV_SP_FROM_BAM); the result's `read` is the call index, a pool row's read index is
    read_base + call_rec[call] and the pool's query_len is the decode's; with seqs=True the uploaded sequences are the chunk's
    records' and the strands are the decode's flags."""
    return _run_split(lib().csv_split_signatures, ctx._h, enc, sv_size, min_mapq, max_split_parts, max_size, ctx._check, pool=pool, from_bam=from_bam,
                      host_outputs=host_outputs)


def pool_rows_of_split(sig, seg_base, read_base, query_len):
    """the rows csv_split_signatures appends to the pool for the candidates `sig` (host restatement, for tests and for callers
    that build the rows themselves): dict(seg, a, b, read, aux) in candidate order"""
    kind = sig["kind"].astype(np.int64); aux = sig["aux"].astype(np.int64)
    a = np.where((kind == 1) & ((aux & 2) != 0), sig["a"] >> 1, sig["a"])
    ql = np.asarray(query_len, np.int64)[sig["read"]]
    # q[c:d] as Python cuts it (py_slice in split.hip.h): a negative bound counts from the end, then [0, len], empty when start >= stop
    lo, hi = (np.clip(np.where(x < 0, x + ql, x), 0, ql) for x in (sig["c"].astype(np.int64), sig["d"].astype(np.int64)))
    ax = np.where(kind == 1, np.maximum(hi - lo, 0), np.where(kind == 3, aux, np.where(kind == 4, sig["c"] * 8 + aux, 0)))
    return dict(seg=(np.asarray(seg_base, np.int64)[kind] + sig["chr"]).astype(np.int32), a=a.astype(np.int64), b=sig["b"].astype(np.int64),
                read=(read_base + sig["read"]).astype(np.int32), aux=ax.astype(np.int32))


_COMP = str.maketrans("ACGTNacgtn", "TGCANtgcan")


def split_candidates(sig, read_names, queries, chrom_names):
    """candidate arrays -> the reference's candidate tuples per SV type (main script :50-464), in the order of its five lists.
    queries[r] = the query string parse_read passes for read r (already reverse-complemented for reverse-strand reads, :673);
    the inserted sequences are cut out of it here."""
    cand = {t: [] for t in ("DEL", "INS", "DUP", "INV", "TRA")}
    rc_cache = {}
    for kind, r, ch, aux, a, b, c, d in zip(sig["kind"].tolist(), sig["read"].tolist(), sig["chr"].tolist(), sig["aux"].tolist(),
                                            sig["a"].tolist(), sig["b"].tolist(), sig["c"].tolist(), sig["d"].tolist()):
        name, chrom = read_names[r], chrom_names[ch]
        if kind == 0:
            cand["DEL"].append((a, b, name, "DEL", chrom))
        elif kind == 1:
            q = queries[r]
            if aux & 1:
                if r not in rc_cache:
                    rc_cache[r] = str(q).translate(_COMP)[::-1]
                q = rc_cache[r]
            cand["INS"].append((a / 2 if aux & 2 else a, b, name, str(q[c:d]), "INS", chrom))
        elif kind == 2:
            cand["DUP"].append((a, b, name, "DUP", chrom))
        elif kind == 3:
            cand["INV"].append(("--" if aux else "++", a, b, name, "INV", chrom))
        else:
            cand["TRA"].append(("ABCD"[aux], a, chrom_names[c], b, name, "TRA", chrom))
    return cand


def pool_ins_sequences_host(queries, query_reverse, sig, ssig, call_read=None):
    """What the sequence pool holds for the INS rows a batch appends, on the host: -> [(bytes, half)] in pool order, the CIGAR
    scan's INS signatures `sig` first, then the kind-1 candidates of the split analysis `ssig` (either may be None).  queries[r]:
    the STORED sequence of read r (str or bytes, as the BAM record has it); query_reverse[r]: the record's flag is 16 (None: no
    read is); call_read[k]: the read of split-read call k (None: the call index is the read index).  CIGAR rows: the pieces
    query[qoff : qoff + len] (extract.candidates).  Split rows: q[c:d] as split_candidates cuts it - q the stored sequence or,
    reversed read, its reverse complement, reverse-complemented once more when aux bit 0 is set - as Python slices; half = aux
    bit 1 and an odd position numerator.  The CPU checker of seqs.hip.h, like name_ranks_host and decode_host."""
    text = lambda q: q.decode() if isinstance(q, (bytes, bytearray)) else str(q)      # noqa: E731
    out = []
    if sig is not None:
        qo, ql = sig["piece_qoff"].tolist(), sig["piece_len"].tolist()
        for r, p0, npc in zip(sig["ins_read"].tolist(), sig["ins_piece0"].tolist(), sig["ins_npiece"].tolist()):
            q = text(queries[r])
            out.append(("".join(q[qo[p]:qo[p] + ql[p]] for p in range(p0, p0 + npc)).encode(), 0))
    if ssig is not None:
        flipped = {}
        for kind, k, aux, a, c, d in zip(ssig["kind"].tolist(), ssig["read"].tolist(), ssig["aux"].tolist(), ssig["a"].tolist(), ssig["c"].tolist(), ssig["d"].tolist()):
            if kind != 1:
                continue
            r = k if call_read is None else int(call_read[k])
            rev = bool(query_reverse[r]) if query_reverse is not None else False
            if rev != bool(aux & 1):
                if r not in flipped:
                    flipped[r] = text(queries[r]).translate(_COMP)[::-1]
                q = flipped[r]
            else:
                q = text(queries[r])
            out.append((q[c:d].encode(), 1 if (aux & 2) and (a & 1) else 0))
    return out


# ------------------------------------------------------------------------------------ parse_read for a batch of reads
def parse_reads(reads, chrom, chrom_rank, sv_size, min_mapq, max_split_parts, min_read_len, min_siglength, merge_del_threshold,
                merge_ins_threshold, max_size, cigar_fn, split_fn):
    """What calling the reference's parse_read (main script :606-681) on every read of `reads`, in order, appends to
    candidate["DEL" | "INS" | "DUP" | "INV" | "TRA"] - with the CIGAR scan and the split-read analysis done per BATCH by
    `cigar_fn(cig_off, cigar, ref_start, use, **kw)` / `split_fn(enc, **kw)` (a context's cigar_signatures /
    split_signatures; the tests also pass the oracle's).  reads: pysam.AlignedSegment-like objects (query_length, flag,
    mapq, reference_start, reference_end, cigartuples, query_sequence, query_name, get_tags()); chrom_rank: {chromosome
    name: rank in Python string order} over every name an SA tag can mention.

    Everything that is text or per-read bookkeeping stays here, as the reference has it: the read-length gate (:607), the
    flag classes (:613), the clip lengths that make primary_info (:619-668), the SA tag (:671-679)."""
    cand = {t: [] for t in ("DEL", "INS", "DUP", "INV", "TRA")}
    keep = [r for r in reads if r.query_length >= min_read_len]                                    # (:607)
    if not keep:
        return cand
    cig_off, cigar = encode_cigars([r.cigartuples for r in keep])
    ref_start = np.fromiter((r.reference_start for r in keep), np.int64, len(keep))
    use = np.fromiter((1 if r.mapq >= min_mapq else 0 for r in keep), np.uint8, len(keep))          # (:614)
    sig = cigar_fn(cig_off, cigar, ref_start, use, min_siglength=min_siglength, merge_ins_threshold=merge_ins_threshold,
                   merge_del_threshold=merge_del_threshold)
    names = [r.query_name for r in keep]
    # reads with an SA tag on a primary record (flag 0 / 16, :657): their segments go through the split-read analysis
    sp = []
    for i, r in enumerate(keep):
        if r.flag not in (0, 16):
            continue
        sa = [v for k, v in r.get_tags() if k == "SA"]
        if not sa:
            continue
        ct = r.cigartuples or ((0, 0),)                                                             # (no CIGAR: no clips)
        left = ct[0][1] if ct[0][0] in (4, 5) else 0                                                # soft clip, or the hard clip that replaces it (:619-652)
        right = ct[-1][1] if ct[-1][0] in (4, 5) else 0
        primary = _primary_info(r.flag, r.mapq >= min_mapq, left, right, r.query_length, r.reference_start, r.reference_end, chrom)
        sp.append((i, primary, sa, r.query_length, r.flag == 16))
    return _assemble(sig, names, [r.query_sequence for r in keep], sp, chrom, chrom_rank, sv_size, min_mapq, max_split_parts, max_size, split_fn)


def _primary_info(flag, mapq_ok, left, right, query_length, reference_start, reference_end, chrom):
    """primary_info of parse_read (:660-668) for a primary record (flag 0 / 16): [] when its mapq does not pass"""
    if not mapq_ok:
        return []
    return ([left, query_length - right, reference_start, reference_end, chrom, "+"] if flag == 0 else
            [right, query_length - left, reference_start, reference_end, chrom, "-"])


class _SplitQueries:
    """queries[k] of split_candidates: the query parse_read passes for split-read call k - the read's sequence, reverse-
    complemented for a reverse-strand read (:673-675) - made when a candidate asks for it (only INS candidates do)"""

    def __init__(self, seqs, idx, reverse):
        self.seqs, self.idx, self.reverse, self.cache = seqs, idx, reverse, {}

    def __getitem__(self, k):
        if k not in self.cache:
            q = self.seqs[self.idx[k]]
            self.cache[k] = str(q).translate(_COMP)[::-1] if self.reverse[k] else q
        return self.cache[k]


def _assemble(sig, names, seqs, sp, chrom, chrom_rank, sv_size, min_mapq, max_split_parts, max_size, split_fn):
    """The second half of parse_reads, shared by the object path and the BAM path: the CIGAR signatures `sig` and the
    split-read inputs `sp` = [(read index, primary_info, [SA values], query_length, reverse strand)] in read order -> the
    five candidate lists.  names / seqs: indexable by read index (lists, or lazy views that slice a BAM chunk's host image)."""
    c_ins, c_del = candidates(sig, names, seqs, chrom)
    sp_reads, sp_idx, sp_query = [], [], []
    for i, primary, sa, qlen, reverse in sp:
        for tag in sa:                                                                              # (one call per SA tag, :671)
            sp_reads.append((primary, tag, qlen)); sp_idx.append(i); sp_query.append(reverse)
    ssig = None
    if sp_reads:
        enc = encode_split_reads(sp_reads, chrom_rank)
        ssig = split_fn(enc, sv_size=sv_size, min_mapq=min_mapq, max_split_parts=max_split_parts, max_size=max_size)
    return _merge(sig, names, seqs, c_ins, c_del, ssig, sp_idx, sp_query, chrom_rank)


def _merge(sig, names, seqs, c_ins, c_del, ssig, sp_idx, sp_query, chrom_rank):
    """the tail of _assemble: the CIGAR candidates c_ins / c_del and the split-read candidates `ssig` (None: no split-read
    call; its `read` numbers the calls, sp_idx[call] = read index, sp_query[call] = reverse strand) -> the five lists"""
    cand = {t: [] for t in ("DEL", "INS", "DUP", "INV", "TRA")}
    s_cand = {t: [] for t in cand}
    s_read = {t: [] for t in cand}
    if ssig is not None:
        s_cand = split_candidates(ssig, [names[i] for i in sp_idx], _SplitQueries(seqs, sp_idx, sp_query), sorted(chrom_rank, key=chrom_rank.get))
        kind_name = ("DEL", "INS", "DUP", "INV", "TRA")
        for k, rd in zip(ssig["kind"].tolist(), ssig["read"].tolist()):
            s_read[kind_name[k]].append(sp_idx[rd])
    # per type: read order; inside a read the CIGAR signatures come first (:656-657 before :671-679)
    for t, c_list, c_reads in (("INS", c_ins, sig["ins_read"].tolist()), ("DEL", c_del, sig["del_read"].tolist())):
        out, j = [], 0
        sl, sr = s_cand[t], s_read[t]
        for x, rd in zip(c_list, c_reads):
            while j < len(sl) and sr[j] < rd:
                out.append(sl[j]); j += 1
            out.append(x)
        out.extend(sl[j:])
        cand[t] = out
    for t in ("DUP", "INV", "TRA"):
        cand[t] = s_cand[t]
    return cand


# ------------------------------------------------------------------------------------ single_pipe: one extraction task
def _in_bed(start, end, bed_regions):
    """--include_bed (:715-723): the reads [start, end) that overlap one of the chromosome's regions"""
    in_bed = np.zeros(len(start), bool)
    for b0, b1 in bed_regions:                               # not (pos_end <= b0 or pos_start >= b1)
        in_bed |= (end > b0) & (start < b1)
    return in_bed


def single_pipe(alignments, chrom, task_start, chrom_rank, sv_size, min_mapq, max_split_parts, min_read_len, min_siglength, merge_del_threshold,
                merge_ins_threshold, max_size, cigar_fn, split_fn, bed_regions=None):
    """What the reference's single_pipe (main script :697-743) pickles for one task region: the five candidate lists of the
    reads that pass its gates and the reads table rows `(start, end, is_primary, name, chr)` (:709-733).

    alignments: what `samfile.fetch(chr, task[1], task[2])` yields, in that order.  Gates, as the reference applies them:
    secondary records (flag 256 / 272) are skipped (:711); a read belongs to the task in which it STARTS
    (`reference_start >= task[1]`, :725) and, with --include_bed, must overlap one of the chromosome's regions (:715-723);
    such a read goes through parse_read (here: one batched call, `parse_reads`), and enters the reads table when its mapq
    passes (:729-733) - whatever parse_read did with it (a read shorter than min_read_len still counts as coverage)."""
    recs = [r for r in alignments if r.flag != 256 and r.flag != 272]
    if recs:
        start = np.fromiter((r.reference_start for r in recs), np.int64, len(recs))
        keep = start >= task_start
        if bed_regions is not None:
            keep &= _in_bed(start, np.fromiter((r.reference_end for r in recs), np.int64, len(recs)), bed_regions)
        recs = [r for r, k in zip(recs, keep.tolist()) if k]
    cand = parse_reads(recs, chrom, chrom_rank, sv_size, min_mapq, max_split_parts, min_read_len, min_siglength, merge_del_threshold,
                       merge_ins_threshold, max_size, cigar_fn, split_fn)
    reads_info = [(r.reference_start, r.reference_end, 1 if r.flag in (0, 16) else 0, r.query_name, chrom) for r in recs if r.mapq >= min_mapq]
    return cand, reads_info


# ------------------------------------------------------------------------------------ single_pipe from a BAM file
class _Lazy:
    """names / sequences of a BAM chunk by record index, sliced out of its host image on first use"""

    def __init__(self, get):
        self.get, self.cache = get, {}

    def __getitem__(self, i):
        if i not in self.cache:
            self.cache[i] = self.get(i)
        return self.cache[i]


def single_pipe_bam(ctx_or_fns, bamfile, chrom, task_start, task_end, chrom_rank, sv_size, min_mapq, max_split_parts, min_read_len, min_siglength,
                    merge_del_threshold, merge_ins_threshold, max_size, bed_regions=None, sa="host", gates="host"):
    """`single_pipe` for the records `fetch(chrom, task_start, task_end)` would yield, read from `bamfile` (a bam.BamFile)
    without an object per record: -> (cand, reads_info) exactly as `single_pipe` returns them.

    ctx_or_fns: an engine.Context - the records are decoded by csv_bam_decode and the CIGAR scan runs on the device columns
    it leaves (the CIGARs cross PCIe once, inside the slim image, and never come back) - or a pair (cigar_fn, split_fn) as
    `single_pipe` takes them: then `bam.decode_host` decodes, the CPU path of the tests.

    The gates are single_pipe's, applied to the columns: secondary records are skipped (:711), a read belongs to the task
    it starts in (:725), the bed overlap (:715-723), reads-table rows for mapq >= min_mapq (:729-733); parse_read's own
    gates (query_length >= min_read_len, :607; mapq, :614) become the `use` column of the CIGAR scan.  Read indices are
    chunk indices throughout: a record that fails a gate has use = 0 and no split-read input, so it contributes nothing.

    sa: "host" - the SA values are sliced out of the chunk and parsed by encode_split_reads - or "device" (needs a Context): they
    are parsed where the decode left them (split_inputs_bam) and analysed in place; only the calls the device flags (text
    outside its strict grammar) go through encode_split_reads, and their candidates are merged at their place in read order.
    Same result either way.

    gates: "host" - `_gates` on the downloaded columns, `use` (and `sel`) uploaded again - or "device" (needs a Context): one kernel
    evaluates them where the columns are (`task_gates`), the scans read its byte column in place, and the host takes the reads rows
    and the selection from the bytes it returns.  Same result either way.  bed_regions: None, or the regions OF THIS TASK
    (bed.Regions.for_task) - an empty list passes no read."""
    from . import bam as bam_mod
    on_device = not isinstance(ctx_or_fns, (tuple, list))
    if sa not in ("host", "device"):
        raise ValueError("sa must be 'host' or 'device', not %r" % (sa,))
    if sa == "device" and not on_device:
        raise ValueError("sa='device' needs an engine.Context: a (cigar_fn, split_fn) pair has no device to parse on")
    _check_gates(gates, on_device)
    chunk = bamfile.records(chrom, task_start, task_end)
    cols = bam_mod.decode(ctx_or_fns, chunk, host_outputs=False) if on_device else bam_mod.decode_host(chunk)
    start, end, flag, mapq, qlen = cols["ref_start"], cols["ref_end"], cols["flag"], cols["mapq"], cols["query_len"]
    _, use, sel, in_table, bits = _task_gates(ctx_or_fns, cols, task_start, bed_regions, min_read_len, min_mapq, gates)
    kw = dict(min_siglength=min_siglength, merge_ins_threshold=merge_ins_threshold, merge_del_threshold=merge_del_threshold)
    if on_device:
        sig = cigar_signatures(ctx_or_fns, None, None, None, use, from_bam=cols, **kw)
        split_fn = lambda enc, **k: split_signatures(ctx_or_fns, enc, **k)             # noqa: E731
    else:
        cigar_fn, split_fn = ctx_or_fns
        sig = cigar_fn(cols["cig_off"], cols["cigar"], start, use, **kw)
    names, seqs = _Lazy(chunk.name), _Lazy(chunk.sequence)
    if sa == "device":
        cand = _assemble_device(ctx_or_fns, chunk, cols, sig, names, seqs, sel, chrom, chrom_rank, sv_size, min_mapq, max_split_parts, max_size, gate_bits=bits)
    else:
        sp = []
        for i in np.flatnonzero(sel).tolist():
            primary = _primary_info(int(flag[i]), mapq[i] >= min_mapq, int(cols["clip_left"][i]), int(cols["clip_right"][i]), int(qlen[i]),
                                    int(start[i]), int(end[i]), chrom)
            sp.append((i, primary, chunk.sa_values(cols, i), int(qlen[i]), int(flag[i]) == 16))
        cand = _assemble(sig, names, seqs, sp, chrom, chrom_rank, sv_size, min_mapq, max_split_parts, max_size, split_fn)
    reads_info = [(int(start[i]), int(end[i]), 1 if cols["cls"][i] == 1 else 0, names[i], chrom) for i in np.flatnonzero(in_table).tolist()]
    return cand, reads_info


def _gates(cols, task_start, bed_regions, min_read_len, min_mapq):
    """single_pipe's gates on the decoded columns of a task's chunk -> (gate: the records of the task, parsed: those parse_read
    does not return from at once (:607), use: the `use` column of the CIGAR scan (:614), sel: the primary records with an SA tag)"""
    gate = (cols["cls"] != 0) & (cols["ref_start"] >= task_start)
    if bed_regions is not None:
        gate &= _in_bed(cols["ref_start"], cols["ref_end"], bed_regions)
    parsed = gate & (cols["query_len"] >= min_read_len)
    use = (parsed & (cols["mapq"] >= min_mapq)).astype(np.uint8)
    return gate, parsed, use, parsed & (cols["cls"] == 1) & (cols["sa_off"][1:] > cols["sa_off"][:-1])


def gate_bits_host(cols, task_start, regions, min_read_len, min_mapq):
    """The byte column csv_bam_task_gates makes, on the host: `_gates` as CSV_GATE_* bits per record (TASK = gate, PARSED, USE, SEL,
    READS = gate & mapq >= min_mapq: the rows of the reads table).  regions: None or the task's (k, 2) list (bed.Regions.for_task).
    The CPU checker of gates.hip.h and the statement of its contract."""
    gate, parsed, use, sel = _gates(cols, task_start, regions, min_read_len, min_mapq)
    reads = gate & (cols["mapq"] >= min_mapq)
    return (gate * _abi.GATE_TASK + parsed * _abi.GATE_PARSED + (use != 0) * _abi.GATE_USE + sel * _abi.GATE_SEL + reads * _abi.GATE_READS).astype(np.uint8)


def task_gates(ctx, n, task_start, min_read_len, min_mapq, regions=None, timing=None):
    """csv_bam_task_gates on the context's last `bam.decode` (n = its record count): the gates of a task evaluated where the columns
    are -> bits, uint8 per record (`gate_bits_host` is the same on the host).  regions: None - no BED gate - or the task's list of
    (b0, b1) (bed.Regions.for_task; any order: the call wants the starts ascending, so an unsorted list is sorted here, which
    changes no answer); an empty list passes no record.  The column also stays on the device until the next decode:
    cigar_signatures(use="gates") and split_inputs_bam(sel="gates") read it there.  timing: a dict that receives ms_device."""
    flags, nr, beg, end = 0, 0, None, None
    if regions is not None:
        r = np.asarray(regions, np.int64).reshape(-1, 2)
        if len(r) > 1 and bool(np.any(r[1:, 0] < r[:-1, 0])):
            r = r[np.argsort(r[:, 0], kind="stable")]
        flags, nr, beg, end = _abi.GT_BED, len(r), np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
    bits = np.zeros(int(n), np.uint8)
    ms = C.c_float(0)
    ctx._check(lib().csv_bam_task_gates(ctx._h, int(n), int(task_start), int(min_read_len), int(min_mapq), flags, nr, beg.ctypes.data if nr else None,
                                        end.ctypes.data if nr else None, bits.ctypes.data if n else None, C.byref(ms)))
    if timing is not None:
        timing["ms_device"] = float(ms.value)
    return bits


def _task_gates(ctx, cols, task_start, bed_regions, min_read_len, min_mapq, gates):
    """the gates of a task, on the host (`_gates`) or on the device (`task_gates`) -> (gate, use, sel, reads rows, bits or None):
    the same arrays either way; with "device" `use` is the string "gates" - the column stays where the scans read it"""
    if gates == "host":
        gate, _, use, sel = _gates(cols, task_start, bed_regions, min_read_len, min_mapq)
        return gate, use, sel, gate & (cols["mapq"] >= min_mapq), None
    bits = task_gates(ctx, len(cols["ref_start"]), task_start, min_read_len, min_mapq, bed_regions)
    return (bits & _abi.GATE_TASK) != 0, "gates", (bits & _abi.GATE_SEL) != 0, (bits & _abi.GATE_READS) != 0, bits


def _check_gates(gates, on_device):
    if gates not in ("host", "device"):
        raise ValueError("gates must be 'host' or 'device', not %r" % (gates,))
    if gates == "device" and not on_device:
        raise ValueError("gates='device' needs an engine.Context: a (cigar_fn, split_fn) pair has no device to evaluate them on")


def _split_on_device(ctx, chunk, cols, sel, chrom, chrom_rank, min_mapq, skw, pool=None, gate_bits=None):
    """The split-read analysis of the records `sel` of the context's last decode: their SA tags are parsed on the device and
    analysed in place (with `pool`: straight to pool rows, only the count comes back); the calls the device flags go through
    encode_split_reads and the host-fed analysis.  -> (split inputs, device-side result or None when there is no call, indices
    of the flagged calls, their reads, host-side candidates or None when nothing is flagged).  gate_bits (the bytes of task_gates):
    the device takes the selection from its own gates column; `sel` is the same selection on the host, for the flagged calls"""
    si = split_inputs_bam(ctx, chunk, cols, sel if gate_bits is None else "gates", chrom_rank, chrom, min_mapq, host_outputs=False, gate_bits=gate_bits)
    dsig = split_signatures(ctx, None, from_bam=si, pool=pool, host_outputs=pool is None, **skw) if si["n_calls"] else None
    calls, reads, fsig = np.zeros(0, np.int64), [], None
    if si["n_flagged"]:
        calls, reads = _flagged_reads(chunk, cols, si, sel, chrom, min_mapq)
        fsig = split_signatures(ctx, encode_split_reads(reads, chrom_rank), **skw)
    return si, dsig, calls, reads, fsig


def _assemble_device(ctx, chunk, cols, sig, names, seqs, sel, chrom, chrom_rank, sv_size, min_mapq, max_split_parts, max_size, gate_bits=None):
    """_assemble for sa="device": the split-read inputs of the records `sel` are parsed and analysed on the device; the calls
    it flags go through encode_split_reads and their candidates are merged at their place in call (= read) order"""
    si, ssig, calls, _, fsig = _split_on_device(ctx, chunk, cols, sel, chrom, chrom_rank, min_mapq,
                                                dict(sv_size=sv_size, min_mapq=min_mapq, max_split_parts=max_split_parts, max_size=max_size), gate_bits=gate_bits)
    if fsig is not None:
        both = {k: np.concatenate([ssig[k], calls[fsig[k]].astype(np.int32) if k == "read" else fsig[k]]) for k, _, _ in _SPLIT_OUT}
        order = np.argsort(both["read"], kind="stable")      # (a call's candidates all come from one side, in their order)
        ssig = {k: v[order] for k, v in both.items()}
    c_ins, c_del = candidates(sig, names, seqs, chrom)
    return _merge(sig, names, seqs, c_ins, c_del, ssig, si["call_rec"].tolist(), (cols["flag"][si["call_rec"]] == 16).tolist(), chrom_rank)


# ------------------------------------------------------------------------------------ a task's region -> rows of the pool
def task_to_pool(ctx, bamfile, chrom, task_start, task_end, chrom_rank, sv_size, min_mapq, max_split_parts, min_read_len, min_siglength,
                 merge_del_threshold, merge_ins_threshold, max_size, seg_ins, seg_del, seg_base, read_base, bed_regions=None, name_pool=False, seq_pool=False, aln=False,
                 gates="host", reads="host", ranges=None):
    """The body of an extraction task without a candidate tuple, a name string or a sequence: the records of the region
    (`bamfile.records`) are decoded on the device, the CIGAR scan appends its signatures to the context's pool from the decoded
    columns (CSV_CG_FROM_BAM | CSV_CG_TO_POOL), the SA tags are parsed there (split_inputs_bam) and the split-read analysis appends
    its candidates (CSV_SP_FROM_BAM | CSV_CG_TO_POOL).  Gates and parameters are single_pipe_bam's.  seg_ins / seg_del: the pool
    segments of the task's INS / DEL signatures; seg_base: per candidate kind (DEL, INS, DUP, INV, TRA) the segment of chromosome
    rank 0; a row's read index is read_base + the record's index in the region's chunk.  Calls the device flags go through
    encode_split_reads and are appended with pool_append before the function returns: the pool is complete then.

    -> dict: n_records, n_sig_ins, n_sig_del, n_calls, n_entries, n_split (candidates of the device path), n_split_host (of the
    flagged calls), n_flagged, flagged_calls / flagged_records (indices of the flagged calls and of their records), and the
    columns of the reads table rows (:729-733) reads_start, reads_end, reads_primary, reads_index (index in the chunk) - or, with
    reads="device", n_reads_rows.

    name_pool=True: the chunk's read names are appended to the context's name pool (rebuild.name_pool_append_chunk) after the
    decode, so that a row's read index IS its name's index: read_base must equal the name pool's row count (ValueError before
    anything is appended) or be None to take it.  The result gains name_base (= that read_base); with `ranks` =
    rebuild.name_ranks(ctx)["rank"] the read ids of the task's reads-table rows are ranks[name_base + reads_index], the id
    space of rebuild.rebuild_pool_by_name's read_id column.

    seq_pool=True: the 4-bit sequences of the records the scans look at (use | sel) are uploaded out of the chunk's host image
    (upload_read_sequences) and both calls run with seqs=True: every INS row gets its inserted bases and its x.5 flag in the
    context's sequence pool, cut on the device.  The INS rows of flagged calls get theirs through rebuild.seq_pool_put, cut on
    the host as single_pipe_bam cuts them.  The pool rows are the same either way; the result gains n_seq_rows / n_seq_bytes
    (the sequence pool's counts after the task).

    aln=True (needs name_pool=True): the records that START in [task_start, task_end) - all of them, whatever their flag or MAPQ -
    become rows of the context's alignment table (aln.append_decoded, on the device, right after the decode) with their name-pool
    indices as ids: what aln.tra_genotype walks.  The caller resets the table (aln.reset) and runs a contig's tasks in order; the
    result gains n_aln_rows.  The table is filled in front of the gates: a BED does not restrict it (the reference's call_gt reads the BAM
    whatever the BED says).

    gates="device": the gates are evaluated by a kernel where the columns are (`task_gates`) and `use` / `sel` never leave the
    device; the reads rows and the `want` flags of the sequence upload come from the bytes it returns.  Same rows either way.

    reads="device" (needs name_pool=True): the rows of the reads table are not cut out of the downloaded columns but appended to the
    context's device-resident reads table (reads.append_decoded, right after the gates) with their name-pool indices as ids - under
    gates="device" straight from the gates column (GATE_READS), under gates="host" from the host's mask.  The caller resets the
    table (reads.reset) and runs the chromosomes in ascending index order; the result carries n_reads_rows instead of the four
    reads_* arrays.

    ranges: None - the task reads `bamfile.records(chrom, task_start, task_end)` - or sorted, disjoint (start, end) pairs inside the
    task: only the records that overlap one of them are read (bam.BamFile.records(ranges=); an empty list reads nothing).  The
    gates are unchanged and decide, so any superset of what they pass gives the same rows; not with aln=True, whose table needs
    every record of the task (ValueError)."""
    from . import bam as bam_mod, rebuild
    _check_gates(gates, True)
    if ranges is not None and aln:
        raise ValueError("aln=True needs every record of the task: ranges= cannot be combined with it")
    if reads not in ("host", "device"):
        raise ValueError("reads must be 'host' or 'device', not %r" % (reads,))
    if reads == "device" and not name_pool:
        raise ValueError("reads='device' needs name_pool=True: a row's id is its name's index")
    table_on_device = reads == "device"                       # (`reads` below: the flagged calls' reads)
    if aln and not name_pool:
        raise ValueError("aln=True needs name_pool=True: a row's id is its name's index")
    if name_pool:
        n_names = rebuild.name_pool_rows(ctx)
        if read_base is None:
            read_base = n_names
        elif read_base != n_names:
            raise ValueError("read_base is %d but the name pool holds %d names: a row's read index must be its name's index" % (read_base, n_names))
    elif read_base is None:
        raise ValueError("read_base=None needs name_pool=True")
    chunk = bamfile.records(chrom, task_start, task_end) if ranges is None else bamfile.records(chrom, ranges=ranges)
    cols = bam_mod.decode(ctx, chunk, host_outputs=False)
    if name_pool:
        rebuild.name_pool_append_chunk(ctx, chunk)
    n_aln = 0
    if aln:
        from . import aln as aln_mod
        n_aln = aln_mod.append_decoded(ctx, chrom_rank[chrom], task_start, task_end, read_base)
    start, end, mapq, qlen = cols["ref_start"], cols["ref_end"], cols["mapq"], cols["query_len"]
    _, use, sel, in_table, bits = _task_gates(ctx, cols, task_start, bed_regions, min_read_len, min_mapq, gates)
    if table_on_device:
        from . import reads as reads_mod
        n_rows = reads_mod.append_decoded(ctx, chrom_rank[chrom], chunk.n, read_base, keep=None if bits is not None else in_table)
    if seq_pool:
        want = (use != 0) | sel if bits is None else (bits & (_abi.GATE_USE | _abi.GATE_SEL)) != 0
        if getattr(chunk, "framed", False):
            upload_read_sequences(ctx, chunk, want=want)
        else:
            s_off, l_seq = chunk.sequence_columns()
            upload_read_sequences(ctx, chunk.host, s_off, l_seq, want=want)
    sig = cigar_signatures(ctx, None, None, None, use, min_siglength=min_siglength, merge_ins_threshold=merge_ins_threshold, merge_del_threshold=merge_del_threshold,
                           pool=dict(seg_ins=seg_ins, seg_del=seg_del, read_base=read_base, query_len=qlen, seqs=seq_pool), host_outputs=False, from_bam=cols)
    si, dsig, calls, reads, fsig = _split_on_device(ctx, chunk, cols, sel, chrom, chrom_rank, min_mapq,
                                                    dict(sv_size=sv_size, min_mapq=min_mapq, max_split_parts=max_split_parts, max_size=max_size),
                                                    pool=dict(seg_base=seg_base, read_base=read_base, seqs=seq_pool), gate_bits=bits)
    n_split, n_host = 0 if dsig is None else dsig["n"], 0
    if fsig is not None:
        rows = pool_rows_of_split(fsig, seg_base, 0, [r[2] for r in reads])
        first_row = rebuild.pool_rows(ctx)
        rec = si["call_rec"][calls]                          # the record of every flagged call
        rebuild.pool_append(ctx, rows["seg"], rows["a"], rows["b"], read_base + rec[fsig["read"]], rows["aux"])
        n_host = len(fsig["kind"])
        ins = np.flatnonzero(fsig["kind"] == 1)
        if seq_pool and len(ins):                             # their INS rows: cut on the host, as single_pipe_bam does
            cut = pool_ins_sequences_host(_Lazy(chunk.sequence), cols["flag"] == 16, None, fsig, call_read=rec)
            rebuild.seq_pool_put(ctx, first_row + ins, [b for b, _ in cut], [h for _, h in cut])
    extra = dict(name_base=read_base) if name_pool else {}
    if table_on_device:
        extra["n_reads_rows"] = n_rows
    else:
        keep = np.flatnonzero(in_table)
        extra.update(reads_start=start[keep], reads_end=end[keep], reads_primary=(cols["cls"][keep] == 1).astype(np.uint8), reads_index=keep)
    if seq_pool:
        extra["n_seq_rows"], extra["n_seq_bytes"] = rebuild.seq_pool_rows(ctx)
    if aln:
        extra["n_aln_rows"] = n_aln
    return dict(**extra, n_records=chunk.n, n_sig_ins=sig["n_sig_ins"], n_sig_del=sig["n_sig_del"], n_calls=si["n_calls"], n_entries=si["n_entries"], n_split=n_split,
                n_split_host=n_host, n_flagged=si["n_flagged"], flagged_calls=calls, flagged_records=si["call_rec"][calls])
