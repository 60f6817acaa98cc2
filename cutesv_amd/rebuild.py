"""The rebuild step on the GPU: unsorted signature rows -> a `SigStore` in the order
contract of cuteSV's process_process_sigs_type (main script :750-857).

`rebuild_columns` is the thin face of `csv_rebuild_signatures` (stable LSD radix sort of a row permutation on
(segment, [aux], pos, len/pos2, read id) + adjacent de-duplication, cutesv_amd/csrc/sort.hip.h);
`store_from_unsorted` assembles the flat store from per-type unsorted columns the extraction step produced.

INS rows are special: the reference sorts them by (chr, int(pos), len, read, sequence) and removes a row only when the
WHOLE tuple repeats - including the sequence and the x.5 of a split-read position ((a + b) / 2, main script :228,
:774-775, :958-969).  The GPU sorts on the integer columns (stable, so equal keys stay in input order) and leaves INS
segments un-deduplicated; the host then finishes the few groups of INS rows that agree in (chr, int(pos), len, read):
ordered by sequence, exact duplicates dropped.  Everything else is exact on the integer columns alone."""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import RebuildIn, RebuildOut, TIE_ORDER_FN, NameRankOut
from ._lib import lib
from .columns import SigStore, NameTable, TYPES


def tie_callback(seq_of_src, half_of_src):
    """csv_tie_order_fn for INS rows (include/cutesv_hip.h): every tie group - rows that agree in (segment, int(pos), len, read)
    - ordered by its sequences (Python's stable sort, like the reference's list.sort with the sequence as the last key, main
    script :774-775) and adjacent rows whose sequence AND x.5 flag are equal too dropped (:958-969).  seq_of_src(row) /
    half_of_src(row): the caller's data by input row.  Returns the ctypes callback (keep a reference while it is in use)."""
    def fn(_user, n_groups, group_off, src_row, order, drop):
        try:
            for g in range(n_groups):
                g0, g1 = group_off[g], group_off[g + 1]
                rows = list(range(g0, g1))
                seq = {i: seq_of_src(src_row[i]) for i in rows}        # (one look-up per row)
                rows.sort(key=seq.__getitem__)
                prev = None
                for pos, i in enumerate(rows):
                    order[i] = pos
                    cur = (seq[i], int(half_of_src(src_row[i])))
                    drop[i] = 1 if (prev is not None and cur == prev) else 0
                    prev = cur
            return 0
        except Exception:                      # noqa: BLE001  (an exception must not cross the C frame)
            import traceback
            traceback.print_exc()
            return 1
    return TIE_ORDER_FN(fn)


def rebuild_columns(ctx, seg_id, a, b, read_id, aux, seg_aux_major, seg_nodedup=None, keep_on_device=False, tie_order=None, src_row_out=None):
    """-> dict(seg_id, a, b, read_id, aux, src_row, ms_device, n_passes, seg_count, n_ins_ties): sorted, de-duplicated rows.
    tie_order: a `tie_callback(...)`: the tie groups of the keep-every-row segments are settled inside the call (n_ins_ties 0).
    keep_on_device: the sorted columns stay in device memory (CSV_RB_KEEP_ON_DEVICE): the dict then holds `dev` (device
    addresses of a / b / read_id / aux, valid until the context's next rebuild / extraction call) and, from the host side,
    only src_row and seg_count - 4 instead of 28 bytes per row cross PCIe.
    src_row_out: an int32 array of at least n entries to receive src_row (a page-locked one lands by DMA)."""
    seg_id = np.ascontiguousarray(seg_id, np.int32); a = np.ascontiguousarray(a, np.int64); b = np.ascontiguousarray(b, np.int64)
    read_id = np.ascontiguousarray(read_id, np.int32); aux = np.ascontiguousarray(aux, np.int32)
    n = len(a)
    if src_row_out is not None and (src_row_out.dtype != np.int32 or len(src_row_out) < n or not src_row_out.flags.c_contiguous):
        raise ValueError("src_row_out must be a contiguous int32 array of at least %d entries" % n)
    return _rebuild(ctx, n, dict(seg_id=seg_id, a=a, b=b, read_id=read_id, aux=aux), None, seg_aux_major, seg_nodedup, keep_on_device, tie_order, src_row_out)


def last_route(ctx):
    """csv_rebuild_route: the sort the context's last successful rebuild took - _abi.RB_ROUTE_COMPACT (16-byte composite-key
    elements), RB_ROUTE_WIDE (32-byte ones), RB_ROUTE_PERM (the permutation sort); RB_ROUTE_NONE before any rebuild"""
    return int(lib().csv_rebuild_route(ctx._h))


def _check_ties(ties, from_pool, seg_nodedup, tie_order):
    """the argument rules of ties="seqs" (CSV_RB_TIES_FROM_SEQS), before anything is asked of the context"""
    if ties not in (None, "seqs"):
        raise ValueError("ties must be None or 'seqs', not %r" % (ties,))
    if ties == "seqs" and (not from_pool or seg_nodedup is None or tie_order is not None):
        raise ValueError("ties='seqs' settles the tie groups of the pool's keep-every-row segments from the sequence pool: it needs the pool and "
                         "seg_nodedup, and excludes tie_order")


def _rebuild(ctx, n_out, cols, read_rank, seg_aux_major, seg_nodedup, keep_on_device, tie_order, src_row_out=None, ties=None):
    """The one csv_rebuild_signatures call: over the caller's columns `cols` (converted to the ABI's widths), or, cols=None, over
    the context's pool with its read indices replaced through `read_rank` (None: through the ranks of the context's name pool,
    CSV_RB_RANK_FROM_NAMES).  n_out: rows the result arrays must hold.  ties="seqs" (pool only): CSV_RB_TIES_FROM_SEQS."""
    _check_ties(ties, cols is None, seg_nodedup, tie_order)
    major = np.ascontiguousarray(seg_aux_major, np.uint8)
    nodedup = None if seg_nodedup is None else np.ascontiguousarray(seg_nodedup, np.uint8)
    rank = None if read_rank is None else np.ascontiguousarray(read_rank, np.int32)
    o = {}
    if not keep_on_device:                                # (else the five sorted columns stay on the device: no host arrays for them)
        o = dict(seg_id=np.empty(n_out, np.int32), a=np.empty(n_out, np.int64), b=np.empty(n_out, np.int64), read_id=np.empty(n_out, np.int32),
                 aux=np.empty(n_out, np.int32))
    o["src_row"] = src_row_out if src_row_out is not None else np.empty(n_out, np.int32)
    seg_count = np.zeros(len(major), np.int64)
    rin = RebuildIn(n_seg=len(major), flags=_abi.RB_KEEP_ON_DEVICE if keep_on_device else 0, seg_aux_major=major.ctypes.data,
                    seg_nodedup=None if nodedup is None else nodedup.ctypes.data, tie_order=None if tie_order is None else C.cast(tie_order, C.c_void_p))
    if cols is None:
        rin.flags |= _abi.RB_FROM_POOL | (_abi.RB_TIES_FROM_SEQS if ties == "seqs" else 0)
        if rank is None:                                  # (the ranks of the context's name pool, on the device already)
            rin.flags |= _abi.RB_RANK_FROM_NAMES
        else:
            rin.read_rank, rin.n_rank = rank.ctypes.data, len(rank)
    else:
        rin.n = n_out
        for k, v in cols.items():
            setattr(rin, k, v.ctypes.data)
    rout = RebuildOut(seg_count=seg_count.ctypes.data, **{k: v.ctypes.data for k, v in o.items()})
    ctx._check(lib().csv_rebuild_signatures(ctx._h, C.byref(rin), C.byref(rout)))
    k = int(rout.n_out)
    out = {key: v[:k] for key, v in o.items()}
    out.update(ms_device=float(rout.ms_device), n_passes=int(rout.n_passes), seg_count=seg_count, n_ins_ties=int(rout.n_ins_ties),
               n_tie_rows=int(rout.n_tie_rows), n_tie_dropped=int(rout.n_tie_dropped), n_out=k)
    if keep_on_device:
        out["dev"] = dict(a=rout.dev_a, b=rout.dev_b, read_id=rout.dev_read_id, aux=rout.dev_aux, seg_id=rout.dev_seg_id, src_row=rout.dev_src_row)
    return out


def _segments(chroms, ins_nodedup):
    """Segment s = type index * len(chroms) + rank of the chromosome's name: -> (chromosome indices in name order, rank per
    chromosome, seg_aux_major: INV / TRA sort on aux first, seg_nodedup: the INS segments keep every row when ins_nodedup)"""
    order = sorted(range(len(chroms)), key=lambda i: chroms[i])
    crank = np.zeros(len(chroms), np.int64)
    crank[order] = np.arange(len(chroms))
    n = len(chroms)
    major, nodedup = np.zeros(len(TYPES) * n, np.uint8), np.zeros(len(TYPES) * n, np.uint8)
    for ti, t in enumerate(TYPES):
        if t in ("INV", "TRA"):
            major[ti * n:(ti + 1) * n] = 1
        if t == "INS" and ins_nodedup:
            nodedup[ti * n:(ti + 1) * n] = 1
    return order, crank, major, nodedup


def _reads_by_chrom(reads, n_chrom):
    """the reads table as keyword arguments of SigStore / HostBatch: blocks by chromosome only, as main script :810 leaves them"""
    if reads is None:
        return {}
    rc = np.asarray(reads["chrom"], np.int64)
    o = np.argsort(rc, kind="stable")
    return dict(reads_off=np.searchsorted(rc[o], np.arange(n_chrom + 1)).astype(np.int64), r_start=np.asarray(reads["start"], np.int64)[o],
                r_end=np.asarray(reads["end"], np.int64)[o], r_primary=np.asarray(reads["primary"], np.uint8)[o], r_id=np.asarray(reads["read_id"], np.int32)[o])


_STAGE = (("seg", np.int32), ("a", np.int64), ("b", np.int64), ("rid", np.int32), ("aux", np.int32), ("src_row", np.int32))


_FILL_CHUNK = 1 << 19                                   # rows per copy job
_POOL = []


def _fill_pool():
    if not _POOL:
        import concurrent.futures
        import os
        _POOL.append(concurrent.futures.ThreadPoolExecutor(max_workers=max(2, min(8, (os.cpu_count() or 2) // 2)), thread_name_prefix="csv-stage"))
    return _POOL[0]


def _staging(ctx, n):
    """views [:n] of the context's page-locked staging columns (grown by half when too small)"""
    from .engine import pinned_empty
    st = getattr(ctx, "_rb_stage", None)
    if st is None or st["cap"] < n:
        cap = max(1024, n + n // 2 if st is not None else n)
        st = {"cap": cap}
        for k, dt in _STAGE:
            st[k] = pinned_empty(cap, dt)
        ctx._rb_stage = st
    return {k: st[k][:n] for k, _ in _STAGE}


def rebuild_to_device_batch(ctx, chroms, per_type, params_segment, reads=None):
    """The rebuild -> cluster hand-off without a host round trip (the reference's dataflow main script :750-857 -> :1113-1199):
    unsorted per-type rows (as store_from_unsorted takes them) are sorted and de-duplicated on the device and STAY there;
    returns (batch, tasks, src_row) where `batch` is an `_abi.HostBatch.on_device` whose columns are the rebuild's device
    buffers, `tasks` the (type, chromosome) pairs of its segments in the reference's order and `src_row` the input row of every
    sorted row (to carry read names / sequences on the host).  Like the batch's device columns, `src_row` lives in the
    context's staging memory: both are valid until the context's next rebuild call (copy src_row to keep it longer).
    params_segment(svtype, chrom_index, begin, end) -> csv_segment record.
    INS rows with `seq` (and `half`): rows that tie on (chromosome, int(pos), len, read) are ordered by their sequences and
    de-duplicated on the whole tuple as the reference does - the few tie rows' indices visit the host through the library's
    tie_order callback, the columns do not (r03 raised on the first tie and sent the whole genome through host memory).
    Without `seq` the integer columns decide."""
    ins = per_type.get("INS")
    ins_ties = ins is not None and ins.get("seq") is not None and len(ins["a"]) > 0
    order, crank, major, nodedup = _segments(chroms, ins_ties)
    # The five columns are written ONCE, in the ABI's widths, into page-locked staging arrays the context keeps (no per-type
    # temporaries, no concatenate pass, and the upload is a DMA at the link's rate instead of a staged copy of pageable memory:
    # the 80 MB of a 30x genome's rows took 4 of the chain's 8.6 ms)
    live = [(ti, t) for ti, t in enumerate(TYPES) if t in per_type and len(per_type[t]["a"])]
    n_rows = sum(len(per_type[t]["a"]) for _, t in live)
    cat = _staging(ctx, n_rows)
    # (one core copies ~20 GB/s: the pieces go to a few threads - numpy's copy / take loops run without the interpreter lock)
    jobs = []
    lo = 0
    for ti, t in live:
        d = per_type[t]
        hi = lo + len(d["a"])
        ch = np.asarray(d["chrom"])
        if len(ch) and (int(ch.min()) < 0 or int(ch.max()) >= len(chroms)):
            raise ValueError("%s rows: chromosome index outside [0, %d)" % (t, len(chroms)))
        seg_of_chrom = (ti * len(chroms) + crank).astype(np.int32)
        src = {"a": np.asarray(d["a"]), "b": np.asarray(d["b"]), "rid": np.asarray(d["read_id"]), "aux": np.asarray(d["aux"])}
        for c0 in range(0, hi - lo, _FILL_CHUNK):
            c1 = min(hi - lo, c0 + _FILL_CHUNK)
            jobs.append((np.take, (seg_of_chrom, ch[c0:c1]), dict(out=cat["seg"][lo + c0:lo + c1], mode="clip")))
            for k, v in src.items():
                jobs.append((np.copyto, (cat[k][lo + c0:lo + c1], v[c0:c1]), dict(casting="unsafe")))
        lo = hi
    if len(jobs) > 8:
        for f in [_fill_pool().submit(fn, *args, **kw) for fn, args, kw in jobs]:
            f.result()
    else:
        for fn, args, kw in jobs:
            fn(*args, **kw)
    n_seg = len(TYPES) * len(chroms)
    ti_ins = TYPES.index("INS")
    cb = None
    if ins_ties:
        ins_base = sum(len(per_type[t]["a"]) for t in TYPES[:ti_ins] if t in per_type)
        seqs = ins["seq"]
        half = ins.get("half")
        cb = tie_callback(lambda s_: seqs[s_ - ins_base], (lambda s_: half[s_ - ins_base]) if half is not None else (lambda s_: 0))
    r = rebuild_columns(ctx, cat["seg"], cat["a"], cat["b"], cat["rid"], cat["aux"], major, nodedup, keep_on_device=True, tie_order=cb,
                        src_row_out=cat["src_row"])
    if r["n_ins_ties"]:                                     # (with a tie callback the device order is final; never with `assert`: -O strips it)
        raise ValueError("%d INS rows tie on (position, length, read) and were not settled on the device: the batch is not in the "
                         "reference's order" % r["n_ins_ties"])
    off = np.r_[0, np.cumsum(r["seg_count"])]
    segs, tasks = [], []
    for s in range(n_seg):
        if r["seg_count"][s] == 0:
            continue
        t, ci = TYPES[s // len(chroms)], order[s % len(chroms)]
        segs.append(params_segment(t, ci, int(off[s]), int(off[s + 1])))
        tasks.append((t, chroms[ci]))
    batch = _abi.HostBatch.on_device(np.array(segs, dtype=_abi.SEGMENT_DTYPE), r["dev"], r["n_out"], n_chrom=len(chroms), keep=ctx,
                                     **_reads_by_chrom(reads, len(chroms)))
    return batch, tasks, r["src_row"]


# ------------------------------------------------------------------------------------ the device-resident signature pool
def pool_reset(ctx):
    ctx._check(lib().csv_pool_reset(ctx._h))


def pool_rows(ctx):
    n = C.c_int64(0)
    ctx._check(lib().csv_pool_rows(ctx._h, C.byref(n)))
    return int(n.value)


def pool_append(ctx, seg_id, a, b, read, aux):
    """rows made on the host (the split-read candidates: they are built from text) -> the context's pool"""
    seg_id = np.ascontiguousarray(seg_id, np.int32); a = np.ascontiguousarray(a, np.int64); b = np.ascontiguousarray(b, np.int64)
    read = np.ascontiguousarray(read, np.int32); aux = np.ascontiguousarray(aux, np.int32)
    ctx._check(lib().csv_pool_append(ctx._h, len(a), seg_id.ctypes.data, a.ctypes.data, b.ctypes.data, read.ctypes.data, aux.ctypes.data))


def seq_pool_rows(ctx):
    """-> (pool rows that hold a sequence, bytes of the sequence pool's blob)"""
    n, b = C.c_int64(0), C.c_int64(0)
    ctx._check(lib().csv_seq_pool_rows(ctx._h, C.byref(n), C.byref(b)))
    return int(n.value), int(b.value)


def seq_pool_put(ctx, rows, seqs, half=None):
    """csv_seq_pool_put: host-made sequences (str or bytes, one per entry of `rows`) and their x.5 flags for EXISTING pool rows -
    the INS rows appended with pool_append.  A sequence's length must be its row's aux, and a row takes one sequence only
    (CsvError E_INVALID, nothing changes)."""
    rows = np.ascontiguousarray(rows, np.int32)
    raw = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    if len(raw) != len(rows) or (half is not None and len(half) != len(rows)):
        raise ValueError("one sequence and (with `half`) one flag per row are expected")
    n = len(rows)
    length = np.fromiter((len(s) for s in raw), np.int32, n)
    off = np.zeros(n, np.int64)
    if n:
        np.cumsum(length[:-1], out=off[1:])
    blob = np.frombuffer(b"".join(raw), np.uint8)
    hv = None if half is None else np.ascontiguousarray(half, np.uint8)
    ctx._check(lib().csv_seq_pool_put(ctx._h, n, rows.ctypes.data if n else None, blob.ctypes.data if len(blob) else None, len(blob), off.ctypes.data if n else None,
                                      length.ctypes.data if n else None, None if hv is None or not n else hv.ctypes.data))


def seq_pool_get(ctx, rows, raw=False):
    """csv_seq_pool_get: the inserted bases of the pool rows `rows` (gathered on the device) -> list of str (raw=True: of bytes).
    A row without a sequence fails the call (CsvError E_INVALID)."""
    rows = np.ascontiguousarray(rows, np.int32)
    n = len(rows)
    off = np.zeros(n + 1, np.int64)
    out = np.empty(1, np.uint8)
    rc = lib().csv_seq_pool_get(ctx._h, n, rows.ctypes.data if n else None, out.ctypes.data, 0, off.ctypes.data)
    if rc == _abi.E_CAPACITY:                             # (the lengths live on the device: the first call reports the need)
        out = np.empty(int(off[-1]), np.uint8)
        rc = lib().csv_seq_pool_get(ctx._h, n, rows.ctypes.data, out.ctypes.data, len(out), off.ctypes.data)
    ctx._check(rc)
    blob, o = out[:int(off[-1])].tobytes(), off.tolist()
    seqs = [blob[o[k]:o[k + 1]] for k in range(n)]
    return seqs if raw else [x.decode() for x in seqs]


def seq_pool_half(ctx, rows):
    """the x.5 flags of the pool rows `rows` (0 for a row without a sequence) -> uint8 array"""
    rows = np.ascontiguousarray(rows, np.int32)
    out = np.zeros(len(rows), np.uint8)
    ctx._check(lib().csv_seq_pool_half(ctx._h, len(rows), rows.ctypes.data if len(rows) else None, out.ctypes.data if len(rows) else None))
    return out


def rebuild_pool(ctx, read_rank, seg_aux_major, seg_nodedup=None, keep_on_device=True, tie_order=None, ties=None):
    """csv_rebuild_signatures over the context's pool (CSV_RB_FROM_POOL): the rows the extraction kernels left on the device
    (extract.cigar_signatures(pool=...)) and those appended with pool_append, sorted and de-duplicated; a row's read index is
    replaced by read_rank[index] (rank of the read's name in Python string order).  Same result dict as rebuild_columns;
    src_row numbers the pool's rows (extraction order).  ties="seqs": the INS tie groups are settled on the device from the
    context's sequence pool under tie_callback's contract (CSV_RB_TIES_FROM_SEQS; needs seg_nodedup, excludes tie_order)."""
    _check_ties(ties, True, seg_nodedup, tie_order)
    return _rebuild(ctx, pool_rows(ctx), None, read_rank, seg_aux_major, seg_nodedup, keep_on_device, tie_order, ties=ties)


# ------------------------------------------------------------------------------------ the device-resident name pool
def name_pool_reset(ctx):
    ctx._check(lib().csv_name_pool_reset(ctx._h))


def name_pool_rows(ctx):
    n = C.c_int64(0)
    ctx._check(lib().csv_name_pool_rows(ctx._h, C.byref(n)))
    return int(n.value)


def name_pool_append(ctx, data, off, length):
    """csv_name_pool_append: name i = data[off[i] : off[i] + length[i]] (data: uint8 array or bytes) -> the index of the first
    appended name; the others follow it.  The ranges are checked by the library (CsvError E_INVALID, pool unchanged)."""
    data = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, np.uint8)
    off = np.ascontiguousarray(off, np.int64); length = np.ascontiguousarray(length, np.int32)
    if len(off) != len(length):
        raise ValueError("one offset and one length per name are expected")
    first = C.c_int64(0)
    ctx._check(lib().csv_name_pool_append(ctx._h, len(off), data.ctypes.data if len(data) else None, len(data), off.ctypes.data if len(off) else None,
                                          length.ctypes.data if len(off) else None, C.byref(first)))
    return int(first.value)


def name_pool_append_chunk(ctx, chunk):
    """the read names of a bam.Chunk, straight out of its host image: name index = returned base + record index"""
    if getattr(chunk, "framed", False) and not chunk.fetched and chunk.ctx is ctx:      # (a device chunk: csv_name_pool_append_framed takes the names where they lie)
        chunk.check()
        first = C.c_int64(0)
        ctx._check(lib().csv_name_pool_append_framed(ctx._h, C.byref(first)))
        return int(first.value)
    off, length = chunk.name_columns()
    return name_pool_append(ctx, chunk.host, off, length)


def name_ranks(ctx, host=True):
    """csv_name_ranks -> dict(rank, first, n, n_distinct, ms_device, n_passes, max_len): rank[i] = index of name i in
    sorted(set(names)) (unsigned bytes; Python's str order for ASCII names), first[r] = smallest index holding the name of rank
    r.  The ranks stay on the device for rebuild_pool_by_name; host=False leaves them there (rank / first are None)."""
    n = name_pool_rows(ctx)
    rank = np.empty(n, np.int32) if host else None
    first = np.empty(n, np.int32) if host else None
    o = NameRankOut(rank=rank.ctypes.data if host and n else None, first=first.ctypes.data if host and n else None, cap_first=n if host else 0)
    ctx._check(lib().csv_name_ranks(ctx._h, C.byref(o)))
    return dict(rank=rank, first=first[:int(o.n_distinct)] if host else None, n=int(o.n), n_distinct=int(o.n_distinct), ms_device=float(o.ms_device),
                n_passes=int(o.n_passes), max_len=int(o.max_len))


def name_pool_get(ctx, index, raw=False):
    """csv_name_pool_get: the names at `index` (gathered on the device) -> list of str (raw=True: of bytes)"""
    index = np.ascontiguousarray(index, np.int32)
    n = len(index)
    out = np.empty(max(1, 255 * n), np.uint8)
    off = np.zeros(n + 1, np.int64)
    ctx._check(lib().csv_name_pool_get(ctx._h, n, index.ctypes.data if n else None, out.ctypes.data, len(out), off.ctypes.data))
    blob, o = out[:int(off[-1])].tobytes(), off.tolist()
    names = [blob[o[k]:o[k + 1]] for k in range(n)]
    return names if raw else [x.decode() for x in names]


def name_ranks_host(data, off, length):
    """What csv_name_ranks computes, in numpy: -> (rank int32[n], first int32[n_distinct]).  The names become rows of a
    zero-padded fixed-width bytes column (NUL cannot occur inside a BAM name, so the padding orders a prefix first) and
    np.unique does the rest.  The CPU path and the checker of the kernels, like bam.decode_host."""
    data = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data, np.uint8)
    off = np.asarray(off, np.int64); length = np.asarray(length, np.int64)
    n = len(off)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    if (length < 0).any() or (length > 255).any() or (off < 0).any() or (off + length > len(data)).any():
        raise ValueError("a name lies outside the bytes given or is longer than 255 bytes")
    width = max(1, int(length.max()))
    mat = np.zeros((n, width), np.uint8)
    row = np.repeat(np.arange(n), length)
    col = np.arange(int(length.sum())) - np.repeat(np.cumsum(length) - length, length)
    mat[row, col] = data[np.repeat(off, length) + col]
    _, first, rank = np.unique(mat.view("S%d" % width).ravel(), return_index=True, return_inverse=True)
    return rank.astype(np.int32).ravel(), first.astype(np.int32)


def rebuild_pool_by_name(ctx, seg_aux_major, seg_nodedup=None, keep_on_device=True, tie_order=None, ties=None):
    """rebuild_pool with a row's read index replaced by the rank of that index in the context's NAME pool
    (CSV_RB_FROM_POOL | CSV_RB_RANK_FROM_NAMES): the ranks are computed on the device when an append made them stale and never
    visit the host.  A pool row whose read index has no name fails the call (CsvError E_INVALID).  Same result dict; ties="seqs" as
    in rebuild_pool."""
    _check_ties(ties, True, seg_nodedup, tie_order)
    return _rebuild(ctx, pool_rows(ctx), None, None, seg_aux_major, seg_nodedup, keep_on_device, tie_order, ties=ties)


# ------------------------------------------------------------------------------------ the VCF strings of a kept pool rebuild
def _negotiated(ctx, call, n_off, guess):
    """one of the two gathers below: call(out pointer, cap, off pointer) -> status; a first try with `guess` bytes, a second one with
    the need the library reported (CSV_E_CAPACITY) -> (blob bytes, off int64[n_off + 1])"""
    off = np.zeros(n_off + 1, np.int64)
    out = np.empty(max(1, int(guess)), np.uint8)
    rc = call(out.ctypes.data, len(out), off.ctypes.data)
    if rc == _abi.E_CAPACITY:
        out = np.empty(int(off[-1]), np.uint8)
        rc = call(out.ctypes.data, len(out), off.ctypes.data)
    ctx._check(rc)
    return out[:int(off[-1])].tobytes(), off


def _int_column(x):
    """a pick / clip / support column in one of the ABI's two widths: int32 stays (CSV_OUT_COORD_I32 results), everything else is int64"""
    x = np.asarray(x)
    return np.ascontiguousarray(x, np.int32 if x.dtype == np.int32 else np.int64)


def alt_gather(ctx, pick, clip, raw=False):
    """csv_seq_alt_gather: entry k = bases(pool row src_row[pick[k]])[:clip[k]] over the context's last kept pool rebuild
    (rebuild_pool / rebuild_pool_by_name with keep_on_device=True) - pick = the seq_pick of INS calls, clip = their SVLEN (bp2),
    int64 or both int32 -> (blob: bytes, off: int64[n + 1]); raw=True: the blob as a uint8 array.  CsvError E_INVALID: no kept
    rebuild or the pools changed since, a pick outside the rebuilt rows, a negative clip, a picked row without a sequence."""
    pick, clip = _int_column(pick), _int_column(clip)
    if pick.shape != clip.shape or pick.ndim != 1:
        raise ValueError("one clip per pick is expected")
    if pick.dtype != clip.dtype:
        pick, clip = pick.astype(np.int64), clip.astype(np.int64)
    n = len(pick)
    flags = _abi.OUT_COORD_I32 if pick.dtype == np.int32 else 0
    guess = int(np.clip(clip, 0, None).sum()) if n else 0
    blob, off = _negotiated(ctx, lambda o, cap, po: lib().csv_seq_alt_gather(ctx._h, n, pick.ctypes.data if n else None, clip.ctypes.data if n else None, flags, o, cap, po), n, guess)
    return (np.frombuffer(blob, np.uint8) if raw else blob), off


def support_join(ctx, support_off, support_sig, raw=False):
    """csv_name_support_join: entry c = ",".join(name(first[read_id[s]]) for s in support_sig[support_off[c]:support_off[c + 1]])
    over the context's last kept rebuild_pool_by_name - the RNAMES text of the calls of a result (its support_off / support_sig,
    int64 or int32) -> (blob: bytes, off: int64[n_calls + 1]); raw=True: the blob as a uint8 array.  CsvError E_INVALID: no kept
    rebuild by name or the pools changed since, a support outside the rebuilt rows, offsets that do not start at 0 or decrease."""
    support_off = np.ascontiguousarray(support_off, np.int64)
    sup = _int_column(support_sig)
    if support_off.ndim != 1 or len(support_off) < 1:
        raise ValueError("support_off needs n_calls + 1 entries")
    if len(support_off) and int(support_off[-1]) > len(sup):
        raise ValueError("support_off names %d supports, %d are given" % (int(support_off[-1]), len(sup)))
    n = len(support_off) - 1
    p64, p32 = (None, sup.ctypes.data) if sup.dtype == np.int32 else (sup.ctypes.data, None)
    if not len(sup):
        p64 = p32 = None
    blob, off = _negotiated(ctx, lambda o, cap, po: lib().csv_name_support_join(ctx._h, n, support_off.ctypes.data, p64, p32, o, cap, po), n, 64 * len(sup) + 4096)
    return (np.frombuffer(blob, np.uint8) if raw else blob), off


def alt_gather_host(seqs_by_pool_row, src_row, pick, clip):
    """What csv_seq_alt_gather computes, in numpy and Python slices: seqs_by_pool_row[r] = the bases of pool row r (str or bytes;
    None or missing: the row has no sequence), src_row = the rebuild's column -> (blob, off).  The checker of the kernels and the
    statement of the contract: ValueError for what the entry refuses."""
    src_row = np.asarray(src_row, np.int64); pick = np.asarray(pick, np.int64); clip = np.asarray(clip, np.int64)
    if pick.shape != clip.shape or pick.ndim != 1:
        raise ValueError("one clip per pick is expected")
    if len(pick) and (int(pick.min()) < 0 or int(pick.max()) >= len(src_row)):
        raise ValueError("a pick lies outside the %d rebuilt rows" % len(src_row))
    if (clip < 0).any():
        raise ValueError("a clip is negative")
    get = seqs_by_pool_row.get if hasattr(seqs_by_pool_row, "get") else (lambda r: seqs_by_pool_row[r] if 0 <= r < len(seqs_by_pool_row) else None)
    parts = []
    for r, c in zip(src_row[pick].tolist(), clip.tolist()):
        s = get(r)
        if s is None:
            raise ValueError("pool row %d has no sequence" % r)
        parts.append((s.encode() if isinstance(s, str) else bytes(s))[:c])
    off = np.zeros(len(parts) + 1, np.int64)
    if parts:
        np.cumsum([len(x) for x in parts], out=off[1:])
    return b"".join(parts), off


def support_join_host(names, first, read_id, support_off, support_sig):
    """What csv_name_support_join computes: names[i] = name i of the name pool (str or bytes), first = name_ranks()["first"],
    read_id = the rebuild's column (ranks) -> (blob, off); ValueError for what the entry refuses."""
    first = np.asarray(first, np.int64); read_id = np.asarray(read_id, np.int64)
    support_off = np.asarray(support_off, np.int64); sup = np.asarray(support_sig, np.int64)
    if len(support_off) < 1 or support_off[0] != 0 or (np.diff(support_off) < 0).any() or support_off[-1] > len(sup):
        raise ValueError("support_off must start at 0, not decrease and stay inside the support list")
    sup = sup[:int(support_off[-1])]
    if len(sup) and (int(sup.min()) < 0 or int(sup.max()) >= len(read_id)):
        raise ValueError("a support lies outside the %d rebuilt rows" % len(read_id))
    rk = read_id[sup]
    if len(rk) and (int(rk.min()) < 0 or int(rk.max()) >= len(first)):
        raise ValueError("a read id is no rank of the name pool")
    nm = [names[i].encode() if isinstance(names[i], str) else bytes(names[i]) for i in first[rk].tolist()]
    so = support_off.tolist()
    parts = [b",".join(nm[so[c]:so[c + 1]]) for c in range(len(so) - 1)]
    off = np.zeros(len(parts) + 1, np.int64)
    if parts:
        np.cumsum([len(x) for x in parts], out=off[1:])
    return b"".join(parts), off


# ------------------------------------------------------------------------------------ the text signature files of a kept pool rebuild
_COORD_END = 1 << 42                                    # positions and lengths live in [0, 2^42)


def _chrom_table(chroms):
    """chromosome names in name-rank order (the numbering of _segments) as the blob + offsets csv_pool_sigs_text takes"""
    enc = [c.encode() if isinstance(c, str) else bytes(c) for c in sorted(chroms)]
    off = np.zeros(len(enc) + 1, np.int64)
    if enc:
        np.cumsum([len(x) for x in enc], out=off[1:])
    return b"".join(enc), off


def sigs_text(ctx, chroms, row_begin, row_end, strands=("++", "--"), raw=False, timing=None):
    """csv_pool_sigs_text: rows [row_begin, row_end) of the context's last kept rebuild_pool_by_name as the lines of cuteSV's
    <TYPE>.sigs files (main script :763-808), made on the device -> bytes (raw=True: a uint8 array).  chroms: the chromosome
    names the segments were numbered over (rebuild._segments: rank = position in sorted(chroms)).  timing: a dict whose
    "ms_kernels" grows by the kernels' HIP-event time.  CsvError E_INVALID: no kept rebuild by name or the pools changed since,
    a row range outside the rebuilt rows, and every row sigs_text_host raises ValueError for."""
    if len(strands) != 2:
        raise ValueError("two strand strings are expected")
    blob, off = _chrom_table(chroms)
    s0, s1 = [s.encode() if isinstance(s, str) else bytes(s) for s in strands]
    row_begin, row_end = int(row_begin), int(row_end)
    need, ms = C.c_int64(0), C.c_float(0)
    out = np.empty(max(1, 96 * max(0, row_end - row_begin)), np.uint8)

    def call():
        return lib().csv_pool_sigs_text(ctx._h, row_begin, row_end, blob, off.ctypes.data, len(off) - 1, s0, s1, out.ctypes.data, len(out), C.byref(need), C.byref(ms))
    rc = call()
    if rc == _abi.E_CAPACITY:                             # (the lengths live on the device: the first call reports the need)
        out = np.empty(int(need.value), np.uint8)
        rc = call()
    ctx._check(rc)
    if timing is not None:
        timing["ms_kernels"] = timing.get("ms_kernels", 0.0) + float(ms.value)
    return out[:int(need.value)] if raw else out[:int(need.value)].tobytes()


def sigs_text_host(cols, names, first, seqs_by_pool_row, chroms, row_begin, row_end, strands=("++", "--")):
    """What csv_pool_sigs_text computes, in Python: cols = the rebuild's sorted columns (seg_id, a, b, read_id, aux, src_row),
    names[i] = name i of the name pool (str or bytes), first = name_ranks()["first"], seqs_by_pool_row[r] = the bases of pool row r
    (None or missing: no sequence) -> bytes.  The checker of the kernels and the statement of the contract: ValueError for what
    the entry refuses."""
    from .columns import BND_NAME
    ch = [c.encode() if isinstance(c, str) else bytes(c) for c in sorted(chroms)]
    st = [s.encode() if isinstance(s, str) else bytes(s) for s in strands]
    n_chrom = len(ch)
    row_begin, row_end = int(row_begin), int(row_end)
    n = len(cols["a"])
    if not 0 <= row_begin <= row_end <= n:
        raise ValueError("rows [%d, %d) lie outside the %d rebuilt rows" % (row_begin, row_end, n))
    sl = slice(row_begin, row_end)
    seg, a, b, rid, aux, src = (np.asarray(cols[k], np.int64)[sl].tolist() for k in ("seg_id", "a", "b", "read_id", "aux", "src_row"))
    first = np.asarray(first, np.int64)
    get = seqs_by_pool_row.get if hasattr(seqs_by_pool_row, "get") else (lambda r: seqs_by_pool_row[r] if 0 <= r < len(seqs_by_pool_row) else None)
    as_bytes = lambda s: s.encode() if isinstance(s, str) else bytes(s)
    lines = []
    for k in range(row_end - row_begin):
        if not 0 <= seg[k] < len(TYPES) * n_chrom:
            raise ValueError("row %d: segment %d lies outside 5 * n_chrom" % (row_begin + k, seg[k]))
        if not (0 <= a[k] < _COORD_END and 0 <= b[k] < _COORD_END):
            raise ValueError("row %d: a position or length is negative or at least 2^42" % (row_begin + k))
        if not 0 <= rid[k] < len(first):
            raise ValueError("row %d: read id %d is no rank of the name pool" % (row_begin + k, rid[k]))
        t, c = TYPES[seg[k] // n_chrom], ch[seg[k] % n_chrom]
        name = as_bytes(names[int(first[rid[k]])])
        head = [t.encode(), c]
        tail = []
        if t == "INS":
            s = get(src[k])
            if s is None or aux[k] < 0:
                raise ValueError("row %d: the INS row has no sequence" % (row_begin + k))
            tail = [as_bytes(s)[:aux[k]]]
        elif t == "INV":
            if not 0 <= aux[k] <= 1:
                raise ValueError("row %d: strand code %d is above 1" % (row_begin + k, aux[k]))
            head.append(st[aux[k]])
        elif t == "TRA":
            if aux[k] < 0 or (aux[k] & 7) > 3 or (aux[k] >> 3) >= n_chrom:
                raise ValueError("row %d: TRA type code above 3 or a mate chromosome outside the table" % (row_begin + k))
            lines.append(b"\t".join(head + [BND_NAME[aux[k] & 7].encode(), b"%d" % a[k], ch[aux[k] >> 3], b"%d" % b[k], name]) + b"\n")
            continue
        lines.append(b"\t".join(head + [b"%d" % a[k], b"%d" % b[k], name] + tail) + b"\n")
    return b"".join(lines)


def type_row_ranges(seg_count, n_chrom):
    """{TYPE: (first row, end row)} of a rebuild over rebuild._segments' numbering, from its seg_count"""
    off = np.r_[0, np.cumsum(np.asarray(seg_count, np.int64))]
    return {t: (int(off[ti * n_chrom]), int(off[(ti + 1) * n_chrom])) for ti, t in enumerate(TYPES)}


def write_sigs(ctx, rb, chroms, out_dir, rows_per_chunk=1 << 20, strands=("++", "--"), timing=None):
    """The five files cuteSV leaves under --write_old_sigs (DEL.sigs, INS.sigs, DUP.sigs, INV.sigs, TRA.sigs in `out_dir`) from the
    kept rebuild `rb` (the dict rebuild_pool_by_name returned), each the rows of its type in the rebuild's order, made by
    sigs_text in chunks of rows_per_chunk rows - no buffer scales with the genome.  A type without rows gives an empty file, as
    the reference's open(..., "w") does.  -> {TYPE: bytes written}"""
    import os
    if rows_per_chunk < 1:
        raise ValueError("rows_per_chunk must be positive")
    written = {}
    for t, (r0, r1) in type_row_ranges(rb["seg_count"], len(chroms)).items():
        total = 0
        with open(os.path.join(out_dir, t + ".sigs"), "wb") as f:
            for c0 in range(r0, r1, rows_per_chunk):
                part = sigs_text(ctx, chroms, c0, min(r1, c0 + rows_per_chunk), strands, raw=True, timing=timing)
                f.write(memoryview(part))
                total += len(part)
        written[t] = total
    return written


def finish_ins_ties(r, ins_segs, seq_of_src, half_of_src):
    """The INS tie groups of a sorted (not de-duplicated) row set `r` (dict of arrays from rebuild_columns): rows that agree
    in (segment, a, b, read_id).  Each group is ordered by sequence (stable: equal sequences keep the concatenation order
    of the extraction files, as the reference's stable sort does) and adjacent rows whose sequence and half-position are
    equal too are dropped (main script :774-775, :958-969).  Returns the index array to apply to r's arrays."""
    n = len(r["a"])
    idx = np.arange(n)
    if n < 2:
        return idx
    is_ins = np.isin(r["seg_id"], ins_segs)
    same = np.zeros(n, bool)
    same[1:] = (is_ins[1:] & (r["seg_id"][1:] == r["seg_id"][:-1]) & (r["a"][1:] == r["a"][:-1]) &
                (r["b"][1:] == r["b"][:-1]) & (r["read_id"][1:] == r["read_id"][:-1]))
    if not same.any():
        return idx
    starts = np.flatnonzero(same & ~np.r_[False, same[:-1]]) - 1          # first row of every tie group
    keep = np.ones(n, bool)
    order = idx.copy()
    for g0 in starts.tolist():
        g1 = g0 + 1
        while g1 < n and same[g1]:
            g1 += 1
        rows = list(range(g0, g1))
        src = r["src_row"][g0:g1].tolist()
        rows.sort(key=lambda i: seq_of_src(src[i - g0]))                    # Python's sort is stable
        order[g0:g1] = rows
        prev = None
        for pos, i in enumerate(rows):
            cur = (seq_of_src(src[i - g0]), int(half_of_src(src[i - g0])))
            if prev is not None and cur == prev:
                keep[g0 + pos] = False
            prev = cur
    return order[keep]


def store_from_unsorted(ctx, chroms, per_type, names=None, strands=("++", "--"), reads=None):
    """per_type: {"DEL": dict(chrom=int[], a=, b=, read_id=, aux=), ...} unsorted rows (chrom = index into `chroms`).
    An INS entry may carry `seq` (list of str, one per row) and `half` (0/1 per row: the position is x.5): the rows are
    then ordered and de-duplicated exactly as the reference does and the store holds the sequences; without them INS rows
    are de-duplicated on their integer columns only.
    Segments come out in the reference's order: types as main_ctrl submits them, chromosomes by name.
    `reads`: optional dict(chrom, start, end, primary, read_id): blocks keep their input order (csv_cluster_batch orders
    every block by start on the device)."""
    ins_seq_in = per_type.get("INS", {}).get("seq") if "INS" in per_type else None
    order, crank, major, nodedup = _segments(chroms, ins_seq_in is not None)
    cols = {k: [] for k in ("seg", "a", "b", "rid", "aux")}
    ins_base, ins_n = 0, 0
    n_rows = 0
    for ti, t in enumerate(TYPES):
        if t not in per_type or len(per_type[t]["a"]) == 0:
            continue
        d = per_type[t]
        ch = np.asarray(d["chrom"], np.int64)
        if t == "INS":
            ins_base, ins_n = n_rows, len(ch)
        cols["seg"].append((ti * len(chroms) + crank[ch]).astype(np.int32))
        cols["a"].append(np.asarray(d["a"], np.int64)); cols["b"].append(np.asarray(d["b"], np.int64))
        cols["rid"].append(np.asarray(d["read_id"], np.int32)); cols["aux"].append(np.asarray(d["aux"], np.int32))       # (the ABI's widths: no conversion pass later)
        n_rows += len(ch)
    cat = {k: np.concatenate(v) if v else np.zeros(0, np.int64) for k, v in cols.items()}
    ti_ins = TYPES.index("INS")
    r = rebuild_columns(ctx, cat["seg"], cat["a"], cat["b"], cat["rid"], cat["aux"], major, nodedup)
    ins_seq = None
    if ins_seq_in is not None:
        half = per_type["INS"].get("half")
        half = np.zeros(ins_n, np.uint8) if half is None else np.asarray(half, np.uint8)
        sel = finish_ins_ties(r, np.arange(ti_ins * len(chroms), (ti_ins + 1) * len(chroms)),
                              lambda s: ins_seq_in[s - ins_base], lambda s: half[s - ins_base])
        for k in ("seg_id", "a", "b", "read_id", "aux", "src_row"):
            r[k] = r[k][sel]
        is_ins = (r["seg_id"] // len(chroms)) == ti_ins
        ins_seq = {int(i): ins_seq_in[int(r["src_row"][i]) - ins_base] for i in np.flatnonzero(is_ins).tolist()}
    seg_sorted = r["seg_id"]
    bounds = np.flatnonzero(np.r_[True, seg_sorted[1:] != seg_sorted[:-1], True]) if len(seg_sorted) else np.zeros(1, np.int64)
    seg_index = {}
    for i in range(len(bounds) - 1):
        s = int(seg_sorted[bounds[i]])
        seg_index[(TYPES[s // len(chroms)], chroms[order[s % len(chroms)]])] = (int(bounds[i]), int(bounds[i + 1]))
    st = SigStore(chroms=list(chroms), a=r["a"], b=r["b"], read_id=r["read_id"], aux=r["aux"], seg_index=seg_index,
                  names=names or NameTable(), strands=tuple(strands), ins_seq=ins_seq, **_reads_by_chrom(reads, len(chroms)))
    return st, r
