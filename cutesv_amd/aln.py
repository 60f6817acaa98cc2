"""The alignment table and the TRA genotyping over it (csrc/aln.hip.h).

The reference genotypes a TRA call from the BAM itself (call_gt, cuteSV_resolveTRA.py:258-309): every alignment fetch() yields
counts - secondary, supplementary, low-MAPQ and placed-unmapped records included - and a record is primary when its flag is 0
or 16, whatever its MAPQ.  The table holds one row per BAM record (start, end, primary, name id), grouped by chromosome, in file
order, on the device; extract.task_to_pool(aln=True) fills it from the decoded columns, tra_genotype walks it with one
wavefront per call.  tra_genotype_host is the same over tra_bam.window_status: the CPU checker and the statement of the contract.
"""
import ctypes as C
import types

import numpy as np

from . import _abi
from ._lib import lib
from .tra_bam import threshold_ref_count, window_status

FROM_KEPT_REBUILD = _abi.ALN_FROM_KEPT_REBUILD
INT32_MAX = 2 ** 31 - 1


def reset(ctx, n_chrom):
    """an empty table for chromosomes 0 .. n_chrom - 1"""
    ctx._check(lib().csv_aln_reset(ctx._h, n_chrom))


def rows(ctx):
    n = C.c_int64(0)
    ctx._check(lib().csv_aln_rows(ctx._h, C.byref(n)))
    return int(n.value)


def append(ctx, chrom, start, end, primary, id):
    """rows of chromosome `chrom` from host arrays (0 <= start < end, id >= 0).  chrom must be at least the last appended one and
    the starts must ascend inside a chromosome, across appends too (CsvError E_UNSORTED; the table is unchanged then)."""
    start = np.ascontiguousarray(start, np.int32); end = np.ascontiguousarray(end, np.int32)
    primary = np.ascontiguousarray(primary, np.uint8); id = np.ascontiguousarray(id, np.int32)
    if not (start.shape == end.shape == primary.shape == id.shape and start.ndim == 1):
        raise ValueError("start, end, primary and id need one entry per row")
    n = len(start)
    ctx._check(lib().csv_aln_append(ctx._h, chrom, n, *(x.ctypes.data if n else None for x in (start, end, primary, id))))


def append_decoded(ctx, chrom, beg, end, name_base):
    """the records of the context's last bam.decode with beg <= pos < end -> rows of `chrom` with the name ids name_base + index in
    the chunk, made on the device -> the number of rows appended"""
    n = C.c_int64(0)
    ctx._check(lib().csv_aln_append_decoded(ctx._h, chrom, beg, end, name_base, C.byref(n)))
    return int(n.value)


def get(ctx, first=0, n=None):
    """rows [first, first + n) (default: all) -> dict(start, end: int32, primary: uint8, id: int32)"""
    if n is None:
        n = rows(ctx) - first
    out = dict(start=np.empty(n, np.int32), end=np.empty(n, np.int32), primary=np.empty(n, np.uint8), id=np.empty(n, np.int32))
    ctx._check(lib().csv_aln_get(ctx._h, first, n, *(out[k].ctypes.data if n else None for k in ("start", "end", "primary", "id"))))
    return out


def layout(ctx, n_chrom):
    """-> (off int64[n_chrom + 1]: first row of every chromosome, maxlen int32[n_chrom]: its longest end - start)"""
    off, maxlen = np.zeros(n_chrom + 1, np.int64), np.zeros(n_chrom, np.int32)
    ctx._check(lib().csv_aln_layout(ctx._h, n_chrom, off.ctypes.data, maxlen.ctypes.data if n_chrom else None))
    return off, maxlen


def timing(ctx):
    """-> (ms of the kernels of the last append, ms of the kernels of the last tra_genotype): HIP events"""
    a, g = C.c_float(0), C.c_float(0)
    ctx._check(lib().csv_aln_timing(ctx._h, C.byref(a), C.byref(g)))
    return float(a.value), float(g.value)


def _calls(chrom1, pos1, chrom2, pos2, support_off):
    chrom1 = np.ascontiguousarray(chrom1, np.int32); chrom2 = np.ascontiguousarray(chrom2, np.int32)
    pos1 = np.ascontiguousarray(pos1, np.int64); pos2 = np.ascontiguousarray(pos2, np.int64)
    support_off = np.ascontiguousarray(support_off, np.int64)
    n = len(chrom1)
    if not (chrom1.shape == chrom2.shape == pos1.shape == pos2.shape == (n,)) or support_off.shape != (n + 1,):
        raise ValueError("one chrom1 / pos1 / chrom2 / pos2 per call and n_calls + 1 support offsets are expected")
    return chrom1, pos1, chrom2, pos2, support_off


def tra_genotype(ctx, chrom1, pos1, chrom2, pos2, support_off, support, contig_len, bias, gt_round, flags=0):
    """csv_aln_tra_genotype: call_gt (cuteSV_resolveTRA.py:258-309) for every call over the context's alignment table ->
    (dr int32[n], status int32[n]): status = count_coverage's answer for the first window, dr = the spanning names that are not
    among the call's supports (-1 where the status is -1).  support: ids as the table holds them, or - with flags =
    FROM_KEPT_REBUILD - the support_sig rows of a result clustered on the context's last kept rebuild_pool_by_name, the table's
    ids being name-pool indices (task_to_pool(aln=True)).  contig_len: one length per chromosome of the table."""
    chrom1, pos1, chrom2, pos2, support_off = _calls(chrom1, pos1, chrom2, pos2, support_off)
    support = np.ascontiguousarray(support)
    if support.dtype != np.int32:
        support = support.astype(np.int64)
    else:
        flags |= _abi.ALN_SUPPORT_I32
    if len(support_off) and int(support_off[-1]) > len(support):
        raise ValueError("support_off names %d supports, %d are given" % (int(support_off[-1]), len(support)))
    contig_len = np.ascontiguousarray(contig_len, np.int64)
    n = len(chrom1)
    dr, status = np.zeros(n, np.int32), np.zeros(n, np.int32)
    ctx._check(lib().csv_aln_tra_genotype(ctx._h, n, *(x.ctypes.data if n else None for x in (chrom1, pos1, chrom2, pos2)), support_off.ctypes.data,
                                          support.ctypes.data if len(support) else None, flags, len(contig_len), contig_len.ctypes.data if len(contig_len) else None,
                                          bias, gt_round, dr.ctypes.data if n else None, status.ctypes.data if n else None))
    return dr, status


def decoded_end(pos, span, flag):
    """the table's end column for records with reference span `span` (0: no CIGAR): pos + max(span, 1), pos + 1 with flag bit 4
    (htslib's bam_endpos), saturating at INT32_MAX"""
    pos = np.asarray(pos, np.int64); span = np.asarray(span, np.int64); flag = np.asarray(flag, np.int64)
    length = np.where(((flag & 4) != 0) | (span < 1), 1, span)
    return np.minimum(pos + length, INT32_MAX).astype(np.int32)


class Table:
    """the table on the host: the columns of `get` plus off (first row per chromosome) - what tra_genotype_host walks"""

    def __init__(self, off, start, end, primary, id):
        self.off = np.asarray(off, np.int64)
        self.start, self.end = np.asarray(start, np.int64), np.asarray(end, np.int64)
        self.primary, self.id = np.asarray(primary, bool), np.asarray(id, np.int64)

    @classmethod
    def from_chroms(cls, per_chrom):
        """per_chrom: one (start, end, primary, id) per chromosome, rows in start order"""
        off = np.r_[0, np.cumsum([len(x[0]) for x in per_chrom])]
        cat = [np.concatenate([np.asarray(x[k]) for x in per_chrom]) if per_chrom else np.zeros(0) for k in range(4)]
        return cls(off, *cat)

    def fetch(self, chrom, s, e):
        """fetch(chrom, s, e) of the stub: the rows with start < e and end > s, in table order (none for an empty window)"""
        if s >= e:
            return
        r0, r1 = int(self.off[chrom]), int(self.off[chrom + 1])
        hi = r0 + int(np.searchsorted(self.start[r0:r1], e, "left"))
        for i in (r0 + np.flatnonzero(self.end[r0:hi] > s)).tolist():
            yield types.SimpleNamespace(flag=0 if self.primary[i] else 2048, reference_start=int(self.start[i]), reference_end=int(self.end[i]),
                                        query_name=int(self.id[i]))


def tra_genotype_host(table, chrom1, pos1, chrom2, pos2, support_off, support, contig_len, bias, gt_round):
    """What csv_aln_tra_genotype computes, on tra_bam.window_status over a stub fetch of `table` (a Table whose ids live in the
    supports' id space) -> (dr, status).  up_bound comes from the number of entries of the call's support list, as in the kernel."""
    chrom1, pos1, chrom2, pos2, support_off = _calls(chrom1, pos1, chrom2, pos2, support_off)
    support = np.asarray(support, np.int64)
    dr, status = np.zeros(len(chrom1), np.int32), np.zeros(len(chrom1), np.int32)
    for c in range(len(chrom1)):
        sup = support[int(support_off[c]):int(support_off[c + 1])]
        reads = set(sup.tolist())
        up_bound = threshold_ref_count(len(sup))
        names = set()
        s, e = max(int(pos1[c]) - bias, 0), min(int(pos1[c]) + bias, int(contig_len[chrom1[c]]))
        st = window_status(table.fetch(int(chrom1[c]), s, e), s, e, names, up_bound, gt_round)
        if st == 0:
            s, e = max(int(pos2[c]) - bias, 0), min(int(pos2[c]) + bias, int(contig_len[chrom2[c]]))
            window_status(table.fetch(int(chrom2[c]), s, e), s, e, names, up_bound, gt_round)
        status[c] = st
        dr[c] = -1 if st == -1 else sum(1 for q in names if q not in reads)
    return dr, status
