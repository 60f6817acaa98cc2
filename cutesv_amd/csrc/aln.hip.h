// aln.hip.h — the alignment table and the TRA genotyping that walks it.
//
// The reference genotypes a TRA call from the BAM itself (call_gt, cuteSV_resolveTRA.py:258-309; count_coverage,
// cuteSV_genotype.py:72-93): EVERY alignment fetch() yields counts towards `iteration` - secondary, supplementary, low-MAPQ
// and placed-unmapped records included - and every record with flag 0 or 16 is primary, whatever its MAPQ.  The reads table
// k_genotype_tra walks holds only the records that passed the extraction gates; this table holds them all:
//   start  pos                                       end  pos + max(reference span, 1); pos + 1 with flag bit 4 (bam_endpos)
//   idp    name id | primary << 31, primary = flag is 0 or 16
// one row per record, grouped by chromosome, in file order (starts ascend inside a chromosome).
//
//   k_aln_keep      one thread per decoded record: cnt = {beg <= pos < end, 0, 0, 0}; the exclusive scan is scan.hip.h's
//                   (scan_counts: k_scan_tiles / k_scan_offsets)
//   k_aln_store     one thread per decoded record: the kept ones become rows behind the table's last row (three int32 stores)
//   k_aln_put       the same for rows that came from host arrays
//   k_aln_check     one thread per NEW row: the order against the row before it (the table's last row for the first one) and
//                   the longest end - start, into a pending pair {flag, longest}
//   k_aln_apply     one thread: the pending longest record into maxlen[chrom] when the flag is clear (atomicMax)
// The rows are written behind the committed count and become part of the table when the host, having read the flag, moves the
// count: a refused append changes nothing a later call reads.
//
//   k_tra_aln       one wavefront per call, tra_window's scheme (kernels.hip.h) over this table: two 64-ary searches bound the
//                   rows of a window (start < e; start + maxlen > s), 64 rows per step, ballots of overlap / primary / span,
//                   popcount prefixes as the running counters, the first stopping lane decides, only lanes up to it commit.
//                   The name set is 4 096 LDS slots seeded with the supports (flag 1; names of the windows: flag 2).  BIG = true:
//                   the calls of big_list, whose set the host gave a slice of global memory (tra_bits_for slots each).
// In rank mode (CSV_ALN_FROM_KEPT_REBUILD) a support is a row of the kept rebuild and its id rid[row], a table row's id is
// rank[name id]: both are looked up where they are used.  Every index is host-checked: chromosomes, supports, name ids.
//
// Includes kernels.hip.h: k_tra_aln calls partition_point_wave, tg_find_or_insert, tra_up_bound and tra_bits_for (and takes
// TG_HASH) from its TRA genotyping section.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wave.hip.h"
#include "kernels.hip.h"

namespace csv {

constexpr int ALN_INT_MAX = 0x7fffffff;

struct AlnCols { int* start; int* end; int* idp; };

struct AlnAppend {
    AlnCols T;
    i64 n0;                         // committed rows: the new ones go behind them
    int prev_same;                  // the table's last row lies on the same chromosome: the first new row is checked against it
    int chrom;
    int* maxlen;                    // per chromosome
    int* pend;                      // {order flag, longest new record, new rows}
};

__global__ __launch_bounds__(256) void k_aln_keep(const i64* pos, i64 n, i64 beg, i64 end, int4* cnt)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) cnt[i] = make_int4(pos[i] >= beg && pos[i] < end ? 1 : 0, 0, 0, 0);
}

// cnt holds the exclusive offsets, tot[0] the number of kept records
__global__ __launch_bounds__(256) void k_aln_store(AlnAppend A, const i64* pos, const i64* ref_end, const int* flag, i64 n, i64 beg, i64 end, int name_base, const int4* cnt,
                                                   const i64* tot)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) A.pend[2] = (int)tot[0];
    if (i >= n) return;
    const i64 p = pos[i];
    if (p < beg || p >= end) return;
    const int f = flag[i];
    i64 len = ref_end[i] - p;
    if ((f & 4) || len < 1) len = 1;
    const i64 e = p + len;
    const i64 r = A.n0 + cnt[i].x;
    A.T.start[r] = (int)p;
    A.T.end[r] = e > ALN_INT_MAX ? ALN_INT_MAX : (int)e;
    A.T.idp[r] = (name_base + (int)i) | ((f == 0 || f == 16) ? (int)0x80000000u : 0);
}

__global__ __launch_bounds__(256) void k_aln_put(AlnAppend A, const int* start, const int* end, const uint8_t* primary, const int* id, i64 n)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) A.pend[2] = (int)n;
    if (i >= n) return;
    A.T.start[A.n0 + i] = start[i];
    A.T.end[A.n0 + i] = end[i];
    A.T.idp[A.n0 + i] = id[i] | (primary[i] ? (int)0x80000000u : 0);
}

// launched over an upper bound of the new rows; pend[2] holds their number
__global__ __launch_bounds__(256) void k_aln_check(AlnAppend A)
{
    const i64 m = A.pend[2];
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    int len = 0, bad = 0;
    if (k < m) {
        const i64 r = A.n0 + k;
        const int s = A.T.start[r];
        len = A.T.end[r] - s;
        if ((k > 0 || A.prev_same) && A.T.start[r - 1] > s) bad = 1;
    }
    for (int d = 32; d; d >>= 1) { const int o = __shfl_xor(len, d); len = o > len ? o : len; }
    if (__ballot(bad) && lane_id() == 0) atomicOr(&A.pend[0], 1);
    if (lane_id() == 0 && len > 0) atomicMax(&A.pend[1], len);
}

__global__ void k_aln_apply(AlnAppend A)
{
    if (threadIdx.x == 0 && blockIdx.x == 0 && A.pend[0] == 0 && A.pend[2] > 0) atomicMax(&A.maxlen[A.chrom], A.pend[1]);
}

// ------------------------------------------------------------------------------------------------ TRA genotyping over the table
struct TraAln {
    const int* start; const int* end; const int* idp;
    const i64* off;                 // n_chrom + 1
    const int* maxlen;              // n_chrom
    const i64* contig_len;          // n_chrom
    const int* rank;                // rank mode: name id -> rank (NameState.rank); else nullptr
    const int* rid;                 // rank mode: row of the kept rebuild -> rank (dev_read_id); else nullptr
    int n_calls;
    const int* chrom1; const int* chrom2;
    const i64* pos1; const i64* pos2;
    const i64* sup_off;             // n_calls + 1
    const int* sup;
    i64 bias, gt_round;
    int* out_dr; int* out_status;
    int* err;                       // a set overflowed (cannot happen: the sets are sized by tra_bits_for)
    // BIG pass
    int n_big;
    const int* big_list;            // calls
    const i64* big_off;             // first int of the call's slice of gset: ids, then flags, 2^bits each
    int* gset;
};

__device__ __forceinline__ int aln_row_id(const TraAln& A, int idp)
{
    const int id = idp & 0x7fffffff;
    return A.rank ? A.rank[id] : id;
}

// one count_coverage() call over the rows of `chrom`; the status (0 / 1 / -1).  nq / dr / filled: wave-uniform running totals
template <bool BIG> __device__ __forceinline__ int aln_window(const TraAln& A, int* ids, int* fl, int bits, int chrom, i64 s, i64 e, i64 up_bound, i64& nq, int& dr,
                                                              int& filled, bool& overflow)
{
    if (s >= e) return 0;
    const i64 limit = (3ll << bits) / 4;
    const i64 r0 = A.off[chrom], r1 = A.off[chrom + 1], maxlen = A.maxlen[chrom];
    if (r1 <= r0) return 0;
    const i64 hi = partition_point_wave(r0, r1, [&](i64 i) { return (i64)A.start[i] < e; });                 // fetch(): start < e ...
    const i64 lo = partition_point_wave(r0, hi, [&](i64 i) { return (i64)A.start[i] + maxlen <= s; });       // ... and end > s (no earlier row is long enough)
    i64 iteration = 0, primary = 0;
    const u64 le = lanemask_lt() | (1ull << lane_id());
    for (i64 base = lo; base < hi; base += 64) {
        if (filled + 64 > limit) { overflow = true; return 0; }
        const i64 i = base + lane_id();
        const bool in = i < hi;
        const i64 ii = in ? i : lo;
        const i64 rs = A.start[ii], re = A.end[ii];
        const int idp = A.idp[ii];
        const bool ov = in && re > s;                                          // GT:76-77
        const bool prim = ov && idp < 0;                                       // GT:78-80
        const bool span = prim && rs < s && re > e;                            // GT:81
        const int id = span ? aln_row_id(A, idp) : 0;
        // a name that occurs twice among the step's spanning rows counts at its first occurrence
        bool dup = false;
        for (u64 m = __ballot(span); m;) {
            const int j = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
            m &= m - 1;
            const int idj = __builtin_amdgcn_readlane(id, j);
            if (span && lane_id() > j && id == idj) dup = true;
        }
        int fresh = 0, slot = 0;
        if (span && !dup) slot = tg_find_or_insert(ids, bits, id, fresh);
        filled += __popcll(__ballot(fresh));
        const int flags = (span && !dup && !fresh) ? fl[slot] : 0;
        const bool isnew = span && !dup && !(flags & 2);
        const u64 m_ov = __ballot(ov), m_pr = __ballot(prim), m_new = __ballot(isnew);
        const i64 it_i = iteration + __popcll(m_ov & le), pn_i = primary + __popcll(m_pr & le), nq_i = nq + __popcll(m_new & le);
        const bool exitA = span && nq_i >= up_bound;                           // GT:83-85
        const bool exitB = prim && it_i >= A.gt_round;                         // GT:86-91
        const u64 stop = __ballot(exitA || exitB);
        const int t = stop ? __builtin_ctzll(stop) : 63;
        const bool commit = isnew && lane_id() <= t;
        if (commit) fl[slot] = flags | 2;
        dr += __popcll(__ballot(commit && !(flags & 1)));
        if (BIG) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");           // the next step's lanes read these flags from global memory
        if (stop) {
            nq = readlane_i64(nq_i, t);
            const int a_t = __builtin_amdgcn_readlane((int)exitA, t);
            const i64 it_t = readlane_i64(it_i, t), pn_t = readlane_i64(pn_i, t);
            if (a_t) return 1;
            return (5 * pn_t <= it_t) ? 1 : -1;                                // float(primary_num / iteration) <= 0.2
        }
        nq += __popcll(m_new); iteration += __popcll(m_ov); primary += __popcll(m_pr);
    }
    return 0;
}

// one call with its set in ids / fl (2^bits slots each)
template <bool BIG> __device__ __forceinline__ void aln_call(const TraAln& A, int c, int* ids, int* fl, int bits)
{
    const i64 T = 1ll << bits, limit = (3ll << bits) / 4;
    for (i64 i = lane_id(); i < T; i += 64) { ids[i] = -1; fl[i] = 0; }
    if (BIG) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    else __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    const i64 s0 = A.sup_off[c], ns = A.sup_off[c + 1] - s0;
    int filled = 0;
    bool overflow = false;
    for (i64 base = 0; base < ns && !overflow; base += 64) {           // read_id_list: flag 1
        if (filled + 64 > limit) { overflow = true; break; }
        const i64 i = base + lane_id();
        int fresh = 0;
        if (i < ns) {
            const int sg = A.sup[s0 + i];
            const int slot = tg_find_or_insert(ids, bits, A.rid ? A.rid[sg] : sg, fresh);
            fl[slot] = 1;
        }
        filled += __popcll(__ballot(fresh));
    }
    if (BIG) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    const i64 up_bound = tra_up_bound(ns);                             // TRA:266
    const int chr1 = A.chrom1[c], chr2 = A.chrom2[c];
    i64 nq = 0;
    int dr = 0, status = 0;
    if (!overflow) {
        i64 s = A.pos1[c] - A.bias, e = A.pos1[c] + A.bias;           // TRA:263-264
        if (s < 0) s = 0;
        if (e > A.contig_len[chr1]) e = A.contig_len[chr1];
        status = aln_window<BIG>(A, ids, fl, bits, chr1, s, e, up_bound, nq, dr, filled, overflow);
        if (status == 0 && !overflow) {                               // TRA:289-299 (status_2 is not looked at)
            s = A.pos2[c] - A.bias; e = A.pos2[c] + A.bias;
            if (s < 0) s = 0;
            if (e > A.contig_len[chr2]) e = A.contig_len[chr2];
            aln_window<BIG>(A, ids, fl, bits, chr2, s, e, up_bound, nq, dr, filled, overflow);
        }
    }
    if (lane_id() == 0) {
        if (overflow) { atomicOr(A.err, 1); status = 0; dr = 0; }
        A.out_dr[c] = status == -1 ? -1 : dr;                          // TRA:276-281
        A.out_status[c] = status;
    }
}

template <bool BIG> __global__ __launch_bounds__(64) void k_tra_aln(TraAln A)
{
    __shared__ int ids[BIG ? 1 : TG_HASH];
    __shared__ int fl[BIG ? 1 : TG_HASH];
    if (BIG) {
        for (int q = blockIdx.x; q < A.n_big; q += gridDim.x) {
            const int c = A.big_list[q];
            const int bits = tra_bits_for(A.sup_off[c + 1] - A.sup_off[c]);
            int* g = A.gset + A.big_off[q];
            aln_call<true>(A, c, g, g + (1ll << bits), bits);
        }
    } else {
        for (int c = blockIdx.x; c < A.n_calls; c += gridDim.x) {
            if (tra_bits_for(A.sup_off[c + 1] - A.sup_off[c]) > 12) continue;      // the BIG pass's
            aln_call<false>(A, c, ids, fl, 12);
        }
    }
}

}  // namespace csv
