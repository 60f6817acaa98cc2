// seqs.hip.h — the INS sequence pool: the inserted bases of every INS pool row, cut out of the reads'
// 4-bit BAM sequences on the GPU, kept beside the signature pool, compared there to settle the rebuild's INS tie groups and
// gathered by pool row.
//
// An INS signature of the reference is (pos, len, read, SEQUENCE) (main script :537, :639-640 for the CIGAR pieces,
// :228 / :244 / :452 for split reads); the rebuild sorts INS rows by (chr, int(pos), len, read, sequence) and drops a row only
// when the whole tuple repeats, the x.5 of a split-read position included (:774-775, :958-969).
//
//   read sequences   SeqReads: the packed image csv_seq_reads_upload checked on the host, read i = (len[i] + 1) / 2 bytes at
//                    off[i], high nibble first; len[i] = -1: not uploaded
//   k_seq_plan_*     one thread per new row: the length of its bases (the pieces / the slice, cut like a Python slice:
//                    py_slice of split.hip.h) - it must equal the pool row's aux - and the reasons a row cannot be cut (no
//                    uploaded read, a negative CIGAR piece); the lengths go through the scan of scan.hip.h (k_scan_tiles / k_scan_offsets)
//   k_seq_gather_*   one wavefront per row: lanes stride over the output, 4 ASCII bytes from 2 (odd start: 3) packed bytes,
//                    one 32-bit store per lane and step; the bytes before the first aligned word and behind the last one are
//                    written one by one.  A split-read slice of the reverse complement is index arithmetic on the stored read.
//   k_seq_tie_order  one wavefront per tie group, rank by counting: order[i] = rows j whose sequence is smaller, or equal with
//                    j < i; drop[i] = the nearest equal row in front of i has the same x.5 flag (rebuild.tie_callback's contract)
//   k_seq_get*       bases by pool row into one blob (csv_seq_pool_get); k_seq_put* attach host-made sequences
// Every loop is bounded by a row's length, its piece count or the group size; every byte read lies inside the range the host
// checked on upload or inside the blob the offsets were made for: a slice c:d goes through py_slice first - a negative bound
// counts from the read's end, both are clamped to [0, len], start >= stop is empty - so that first >= 0 and first + length <= len,
// and the gather reads bases first .. first + length - 1 (reversed: len - 1 - first down to len - first - length) of [0, len).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wave.hip.h"
#include "cigar.hip.h"
#include "split.hip.h"

namespace csv {

struct SeqReads { const uint8_t* bytes; const i64* off; const int* len; i64 n; };
struct SeqPool { uint8_t* blob; i64* off; uint8_t* half; };          // off[pool row] = first byte in blob, -1: the row has no sequence
enum { SEQ_ERR_NO_READ = 1, SEQ_ERR_NEGATIVE = 2 /* a CIGAR piece; a split-read slice may have negative bounds */, SEQ_ERR_LENGTH = 4, SEQ_ERR_TAKEN = 8 };

// "=ACMGRSVTWYHKDBN"[code], or its complement as extract._COMP has it: A <-> T, C <-> G, everything else unchanged
__device__ __forceinline__ unsigned seq_ascii(unsigned code, bool comp)
{
    const u64 lo = comp ? 0x565352434d47543dull : 0x565352474d43413dull;      // "=TGMCRSV" : "=ACMGRSV", the first character in the low byte
    const u64 hi = comp ? 0x4e42444b48595741ull : 0x4e42444b48595754ull;      // "AWYHKDBN" : "TWYHKDBN"
    return (unsigned)(((code & 8u) ? hi : lo) >> (8 * (code & 7u))) & 255u;
}
__device__ __forceinline__ unsigned seq_char(const uint8_t* src, i64 base, bool comp)
{
    const unsigned b = src[base >> 1];
    return seq_ascii((base & 1) ? (b & 15u) : (b >> 4), comp);
}

// L output bytes at dst by one wavefront: byte j = base `start + j` of the read at src, or (rev) the complement of base `start - j`
__device__ __forceinline__ void seq_copy(const uint8_t* src, i64 start, i64 L, bool rev, uint8_t* dst, int lane)
{
    i64 head = (i64)((4 - ((uintptr_t)dst & 3)) & 3);
    head = head < L ? head : L;
    if (lane < head) dst[lane] = (uint8_t)seq_char(src, rev ? start - lane : start + lane, rev);
    const i64 nw = (L - head) >> 2;
    for (i64 w = lane; w < nw; w += 64) {
        const i64 j = head + 4 * w;
        const i64 lo = rev ? start - j - 3 : start + j;             // the lowest of the four bases
        const i64 b = lo >> 1;
        const int odd = (int)(lo & 1);
        unsigned bytes = (unsigned)src[b] | ((unsigned)src[b + 1] << 8);
        if (odd) bytes |= (unsigned)src[b + 2] << 16;
        unsigned word = 0;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int nib = odd + (rev ? 3 - t : t);                 // nibble of base lo + (3 - t | t) in `bytes`, high nibble first
            const unsigned by = (bytes >> (8 * (nib >> 1))) & 255u;
            word |= seq_ascii((nib & 1) ? (by & 15u) : (by >> 4), rev) << (8 * t);
        }
        *(unsigned*)(dst + j) = word;
    }
    const i64 t0 = head + 4 * nw;
    if (lane < L - t0) dst[t0 + lane] = (uint8_t)seq_char(src, rev ? start - (t0 + lane) : start + t0 + lane, rev);
}

// a Python slice [q, e) of a sequence of l >= 0 bases: -> {first, length}
__device__ __forceinline__ i64 seq_clip(i64 q, i64 e, i64 l, i64* first) { return py_slice(q, e, l, first); }

// ------------------------------------------------------------------------------------ the CIGAR scan's INS rows
// cnt[i] = {bytes of row i, 1, 0, 0} (zeros when the row cannot be cut: *err says why)
__global__ __launch_bounds__(256) void k_seq_plan_cigar(SeqReads S, CigarArgs A, i64 n_ins, const int* pool_aux, int4* cnt, int* err)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_ins) return;
    const int r = A.ins_read[i];
    const int l = (r >= 0 && r < S.n) ? S.len[r] : -1;
    int e = 0;
    i64 len = 0;
    if (l < 0) e = SEQ_ERR_NO_READ;
    else {
        const i64 p0 = A.ins_piece0[i];
        for (int k = 0; k < A.ins_npiece[i]; k++) {
            const i64 q = A.piece_qoff[p0 + k], pl = A.piece_len[p0 + k];
            i64 first;
            if (q < 0 || pl < 0) e |= SEQ_ERR_NEGATIVE;
            else len += seq_clip(q, q + pl, l, &first);
        }
    }
    if (!e && len != (i64)pool_aux[i]) e = SEQ_ERR_LENGTH;
    if (e) atomicOr(err, e);
    cnt[i] = e ? make_int4(0, 0, 0, 0) : make_int4((int)len, 1, 0, 0);
}

// one wavefront per row (only launched when the plan found nothing wrong)
__global__ __launch_bounds__(256) void k_seq_gather_cigar(SeqReads S, SeqPool P, CigarArgs A, i64 n_ins, const int4* cnt, i64 pool_base, i64 blob_base)
{
    const i64 k = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n_ins) return;
    const int lane = threadIdx.x & 63;
    const int r = A.ins_read[k];
    const i64 l = S.len[r];
    const uint8_t* src = S.bytes + S.off[r];
    i64 o = blob_base + cnt[k].x;
    if (lane == 0) { P.off[pool_base + k] = o; P.half[pool_base + k] = 0; }
    const i64 p0 = A.ins_piece0[k];
    for (int p = 0; p < A.ins_npiece[k]; p++) {
        const i64 q = A.piece_qoff[p0 + p];
        i64 first;
        const i64 len = seq_clip(q, q + A.piece_len[p0 + p], l, &first);
        if (len > 0) seq_copy(src, first, len, false, P.blob + o, lane);
        o += len;
    }
}

// ------------------------------------------------------------------------------------ the split analysis' INS candidates
// The bases of a kind-1 candidate are q[c:d], q = the read as stored (flag != 16) or its reverse complement (flag == 16),
// reverse-complemented once more when aux bit 0 is set: rev = (flag == 16) ^ (aux & 1) and, for rev, q[x] = comp(read[l - 1 - x]).
struct SeqSplitSrc { const int* read_map; const int* rec_flag; const uint8_t* query_reverse; };      // CSV_SP_FROM_BAM: call -> record, the records' flags; else per read

__global__ __launch_bounds__(256) void k_seq_plan_split(SeqReads S, SplitArgs A, SeqSplitSrc Q, i64 n, const int* pool_aux, int4* cnt, int* err)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (A.kind[i] != 1) { cnt[i] = make_int4(0, 0, 0, 0); return; }
    const int rr = A.read[i], r = Q.read_map ? Q.read_map[rr] : rr;
    const int l = (r >= 0 && r < S.n) ? S.len[r] : -1;
    int e = 0;
    i64 len = 0, first;
    if (l < 0) e = SEQ_ERR_NO_READ;
    else len = seq_clip(A.c[i], A.d[i], l, &first);
    if (!e && len != (i64)pool_aux[i]) e = SEQ_ERR_LENGTH;
    if (e) atomicOr(err, e);
    cnt[i] = e ? make_int4(0, 0, 0, 0) : make_int4((int)len, 1, 0, 0);
}

__global__ __launch_bounds__(256) void k_seq_gather_split(SeqReads S, SeqPool P, SplitArgs A, SeqSplitSrc Q, i64 n, const int4* cnt, i64 pool_base, i64 blob_base)
{
    const i64 k = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n) return;
    const int lane = threadIdx.x & 63;
    if (A.kind[k] != 1) {
        if (lane == 0) { P.off[pool_base + k] = -1; P.half[pool_base + k] = 0; }
        return;
    }
    const int rr = A.read[k], r = Q.read_map ? Q.read_map[rr] : rr, aux = A.aux[k];
    const i64 l = S.len[r];
    const bool stored_reverse = Q.rec_flag ? Q.rec_flag[r] == 16 : (Q.query_reverse && Q.query_reverse[rr] != 0);
    const bool rev = stored_reverse != ((aux & 1) != 0);
    i64 first;
    const i64 len = seq_clip(A.c[k], A.d[k], l, &first);
    const i64 o = blob_base + cnt[k].x;
    if (lane == 0) { P.off[pool_base + k] = o; P.half[pool_base + k] = (uint8_t)(((aux & 2) != 0) && (A.a[k] & 1)); }
    if (len > 0) seq_copy(S.bytes + S.off[r], rev ? l - 1 - first : first, len, rev, P.blob + o, lane);
}

// ------------------------------------------------------------------------------------ by pool row
// len[k] = bytes of row rows[k], -1: the row has no sequence
__global__ __launch_bounds__(256) void k_seq_get_len(const i64* off, const int* aux, const int* rows, i64 n, int* len)
{
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k < n) len[k] = off[rows[k]] >= 0 ? aux[rows[k]] : -1;
}
// one wavefront per requested row: out[out_off[k] ..] = its bases
__global__ __launch_bounds__(256) void k_seq_get(const uint8_t* blob, const i64* off, const int* rows, const i64* out_off, i64 n, uint8_t* out)
{
    const i64 k = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n) return;
    const i64 b = off[rows[k]], o = out_off[k], len = out_off[k + 1] - o;
    for (i64 j = threadIdx.x & 63; j < len; j += 64) out[o + j] = blob[b + j];
}
// csv_seq_pool_put: may row rows[k] take a sequence of len[k] bytes?  Then: off[rows[k]] = at[k], half[rows[k]] = h[k].
__global__ __launch_bounds__(256) void k_seq_put_check(const i64* off, const int* aux, const int* rows, const int* len, i64 n, int* err)
{
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    int e = 0;
    if (off[rows[k]] >= 0) e |= SEQ_ERR_TAKEN;
    if (aux[rows[k]] != len[k]) e |= SEQ_ERR_LENGTH;
    if (e) atomicOr(err, e);
}
__global__ __launch_bounds__(256) void k_seq_put_apply(SeqPool P, const int* rows, const i64* at, const uint8_t* h, i64 n)
{
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k < n) { P.off[rows[k]] = at[k]; P.half[rows[k]] = h[k] ? 1 : 0; }
}

// ------------------------------------------------------------------------------------ INS tie groups
// < 0: x sorts first, 0: equal, > 0: y sorts first (unsigned bytes, a prefix first)
__device__ __forceinline__ int seq_cmp(const uint8_t* x, i64 lx, const uint8_t* y, i64 ly)
{
    const i64 m = lx < ly ? lx : ly;
    for (i64 k = 0; k < m; k++)
        if (x[k] != y[k]) return x[k] < y[k] ? -1 : 1;
    return lx < ly ? -1 : lx > ly ? 1 : 0;
}

// one wavefront per group g = rows [goff[g], goff[g + 1]) of src (pool rows, in the sort's stable order); lanes stride over its rows
__global__ __launch_bounds__(256) void k_seq_tie_order(const uint8_t* blob, const i64* off, const int* aux, const uint8_t* half, const i64* goff, const int* src,
                                                       i64 n_groups, int* order, uint8_t* drop, int* err)
{
    const i64 g = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const i64 g0 = goff[g], g1 = goff[g + 1];
    for (i64 i = g0 + (threadIdx.x & 63); i < g1; i += 64) {
        const int ri = src[i];
        const i64 oi = off[ri], li = aux[ri];
        int rank = 0;
        i64 last = -1;                                              // the nearest row in front of i with the same sequence
        if (oi < 0) atomicOr(err, SEQ_ERR_NO_READ);
        else
            for (i64 j = g0; j < g1; j++) {
                const i64 oj = off[src[j]];
                if (j == i || oj < 0) continue;
                const int cm = seq_cmp(blob + oj, aux[src[j]], blob + oi, li);
                if (cm < 0 || (cm == 0 && j < i)) rank++;
                if (cm == 0 && j < i) last = j;
            }
        order[i] = oi < 0 ? (int)(i - g0) : rank;
        drop[i] = (uint8_t)(last >= 0 && half[src[last]] == half[ri]);
    }
}

}  // namespace csv
