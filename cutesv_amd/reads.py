"""The genotyping reads table in device memory (csrc/reads.hip.h).

The reference's reads table (main script :729-733) has one row per record that passed the gates of its task with
mapq >= min_mapq: (reference_start, reference_end, is_primary, name).  extract.task_to_pool(reads="device") cuts those rows out of
the decoded columns where they are (append_decoded), call_bam hands the table to the engine where it lies (batch_columns ->
_abi.HostBatch.on_device(reads_dev=...)).  table_host is the same table from the per-task arrays of the host path: the CPU
checker and the statement of the contract.
"""
import ctypes as C

import numpy as np

from . import _abi
from ._lib import lib

RANK_FROM_NAMES = _abi.RD_RANK_FROM_NAMES
INT32_MAX = 2 ** 31 - 1


def reset(ctx, n_chrom):
    """an empty table for chromosomes 0 .. n_chrom - 1"""
    ctx._check(lib().csv_reads_reset(ctx._h, n_chrom))


def rows(ctx):
    n = C.c_int64(0)
    ctx._check(lib().csv_reads_rows(ctx._h, C.byref(n)))
    return int(n.value)


def append_decoded(ctx, chrom, n_records, name_base, keep=None):
    """the records of the context's last bam.decode (n_records = its record count) that belong in the table -> rows of `chrom`
    with the name ids name_base + index in the chunk, made on the device -> the number of rows appended.  keep=None: the records
    whose byte of the gates column `extract.task_gates` left beside that decode has GATE_READS; else one byte per record,
    non-zero = keep (the host-gated path).  chrom must be at least the last appended one."""
    if keep is not None:
        keep = np.ascontiguousarray(keep, np.uint8)
        if keep.shape != (int(n_records),):
            raise ValueError("keep: one byte per record is expected")
        if not len(keep):
            keep = np.zeros(1, np.uint8)                   # (an empty chunk: the address still says "host-gated")
    n = C.c_int64(0)
    ctx._check(lib().csv_reads_append_decoded(ctx._h, chrom, int(n_records), None if keep is None else keep.ctypes.data, int(name_base), C.byref(n)))
    return int(n.value)


def append(ctx, chrom, start, end, primary, id):
    """rows of chromosome `chrom` from host arrays (0 <= start <= end, id >= 0); chrom must be at least the last appended one"""
    start = np.ascontiguousarray(start, np.int32); end = np.ascontiguousarray(end, np.int32)
    primary = np.ascontiguousarray(primary, np.uint8); id = np.ascontiguousarray(id, np.int32)
    if not (start.shape == end.shape == primary.shape == id.shape and start.ndim == 1):
        raise ValueError("start, end, primary and id need one entry per row")
    n = len(start)
    ctx._check(lib().csv_reads_append(ctx._h, chrom, n, *(x.ctypes.data if n else None for x in (start, end, primary, id))))


def get(ctx, first=0, n=None):
    """rows [first, first + n) (default: all) -> dict(start, end: int32, primary: uint8, id: int32)"""
    if n is None:
        n = rows(ctx) - first
    out = dict(start=np.empty(n, np.int32), end=np.empty(n, np.int32), primary=np.empty(n, np.uint8), id=np.empty(n, np.int32))
    ctx._check(lib().csv_reads_get(ctx._h, first, n, *(out[k].ctypes.data if n else None for k in ("start", "end", "primary", "id"))))
    return out


def batch_columns(ctx, n_chrom, flags=0):
    """csv_reads_batch_columns: the table as HostBatch.on_device(reads_dev=...) takes it -> dict(reads_off: int64[n_chrom + 1] on the
    host; r_start, r_end, r_primary, r_id: DEVICE addresses (None for an empty table); n_reads).  flags=RANK_FROM_NAMES: r_id holds
    the name pool's rank of every row's name id (the id space of rebuild.rebuild_pool_by_name's read_id column), gathered on the
    device into a column of its own.  The addresses are valid until the table's next append, reset or batch_columns."""
    off = np.zeros(int(n_chrom) + 1, np.int64)
    d = _abi.ReadsDev()
    ctx._check(lib().csv_reads_batch_columns(ctx._h, int(flags), int(n_chrom), off.ctypes.data, C.byref(d)))
    return dict(reads_off=off, r_start=d.r_start, r_end=d.r_end, r_primary=d.r_primary, r_id=d.r_id, n_reads=int(d.n_reads))


def timing(ctx):
    """-> (ms of the kernels of the last append, ms of the rank gather of the last batch_columns): HIP events"""
    a, g = C.c_float(0), C.c_float(0)
    ctx._check(lib().csv_reads_timing(ctx._h, C.byref(a), C.byref(g)))
    return float(a.value), float(g.value)


def decoded_rows(cols, keep, name_base):
    """what append_decoded makes of the decoded columns `cols` (bam.decode / decode_host) and a keep mask, on the host ->
    dict(start, end, primary, id) as `get` returns them"""
    k = np.flatnonzero(np.asarray(keep))
    return dict(start=np.asarray(cols["ref_start"])[k].astype(np.int32), end=np.minimum(np.asarray(cols["ref_end"], np.int64)[k], INT32_MAX).astype(np.int32),
                primary=(np.asarray(cols["cls"])[k] == 1).astype(np.uint8), id=(int(name_base) + k).astype(np.int32))


def table_host(tasks, ranks, n_chrom):
    """The reads table of a call on the host.  tasks: [(chromosome index, r)] in task order, r the dict extract.task_to_pool
    returns with reads="host" (reads_start, reads_end, reads_primary, reads_index, name_base); ranks: the name pool's rank column
    (rebuild.name_ranks(ctx)["rank"]) -> the keyword arguments of HostBatch (reads_off, r_start, r_end, r_primary, r_id): the rows
    of all tasks, their ids ranks[name_base + reads_index], stably ordered by chromosome (rebuild._reads_by_chrom)."""
    from .rebuild import _reads_by_chrom
    if not tasks:
        return {}
    ranks = np.asarray(ranks)
    rd = dict(chrom=np.concatenate([np.full(len(r["reads_index"]), ci, np.int64) for ci, r in tasks]),
              start=np.concatenate([r["reads_start"] for _, r in tasks]), end=np.concatenate([r["reads_end"] for _, r in tasks]),
              primary=np.concatenate([r["reads_primary"] for _, r in tasks]),
              read_id=ranks[np.concatenate([r["name_base"] + r["reads_index"] for _, r in tasks]).astype(np.int64)])
    return _reads_by_chrom(rd, n_chrom)
