// sa.hip.h — the text of the SA:Z tags of a decoded BAM chunk -> the entry columns of csv_split_in, on the GPU (DESIGN.md
// section 14).  Restates what extract.encode_split_reads does with str.split, int() and a regular expression per entry:
// parse_read's primary_info (cuteSV main script :660-668) and, per "chr,pos,strand,CIGAR,mapq,NM;" entry of the tag,
// organize_split_signal's fields (:493-497) with acquire_clip_pos (:466-481) on the entry's CIGAR text.
//
// Input: what csv_bam_decode left on the device (bam.hip.h: the slim image, sa_off / sa_beg / sa_end and the per-record
// columns), a byte per record `sel`, and the contig names sorted in byte order with the caller's rank for each.
// A CALL is one (selected record, SA tag) pair, in record order and then tag order (the `for tag in sa` of extract._assemble).
//
//   k_sa_mark     one thread per record: the number of its calls (its SA tags when sel[i], else 0)
//   k_sa_scan     one workgroup: counts -> exclusive offsets in place (records -> calls, then calls -> entries)
//   k_sa_calls    one thread per record: call -> (record, SA tag), read_len
//   k_sa_parse<false>   one wavefront per call: parses the value, writes status and the number of entries
//   k_sa_parse<true>    the same walk again, now writing the entry columns at ent_off (a flagged call writes nothing)
//
// A wavefront reads its value 16 bytes per lane (1 KiB per step; the blocks that straddle the value's ends byte by byte,
// so that every byte read lies inside [sa_beg, sa_end), the range the decode checked against the record).  Each lane
// marks the ';' among its bytes; a prefix sum over the lanes numbers them, and the byte behind ';' number k - where entry
// k + 1 begins - goes to LDS.  Then one LANE per entry walks that entry's fields (64 entries per round; longer values
// take more rounds, values beyond 1 KiB more steps).  Text behind the last ';' belongs to no entry: the reference takes
// value.split(";")[:-1].
//
// The grammar is strict - see SA_ST_* - and anything else flags the CALL: it gets no entries here and the Python layer
// sends it through encode_split_reads, so Python's int(), the regular expression's skipping of characters it does not
// match, KeyError and IndexError stay what decides those.  extract.sa_status is the same classifier on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wave.hip.h"

namespace csv {

// status bits of a call (OR over its entries)
constexpr int SA_ST_NUMBER = 1;     // pos / mapq: not 1..18 (mapq: 1..9) ASCII digits
constexpr int SA_ST_STRAND = 2;     // the strand field is not one character
constexpr int SA_ST_CIGAR = 4;      // the CIGAR field is neither "*" nor a run of <1..18 digits><one of MIDNSHP=XB>
constexpr int SA_ST_FIELDS = 8;     // fewer than five fields
constexpr int SA_ST_NAME = 16;      // the contig is not in the name table

struct SaArgs {
    i64 n;                          // records of the chunk
    i64 cap_calls, cap_entries;     // sizes of the per-call / per-entry arrays (writes are checked against them)
    const uint8_t* slim;
    const i64* sa_off; const i64* sa_beg; const i64* sa_end;
    const int* flag; const int* mapq; const int* qlen; const int* clip_l; const int* clip_r; const i64* ref_start; const i64* ref_end;
    const uint8_t* sel;
    int sel_mask;                   // the bits of sel[i] that count: 255, or CSV_GATE_SEL when `sel` is the gates column
    int min_mapq, task_rank;
    const uint8_t* names; const i64* name_off; const int* name_rank; int n_names;      // name k = names[name_off[k] .. name_off[k + 1]), ascending
    i64* call_off;                  // n + 1: calls per record, then exclusive offsets
    int* call_rec; i64* call_sa;    // per call: its record, the index of its tag in sa_beg / sa_end
    i64* ent_off;                   // cap_calls + 1: entries per call, then exclusive offsets
    i64* read_len; uint8_t* status;
    i64* tot;                       // [0] calls, [1] entries, [2] flagged calls
    i64* c0; i64* c1; i64* f0; i64* f1; int* chr; int* emapq; uint8_t* strand; uint8_t* primary;
};

__global__ __launch_bounds__(256) void k_sa_mark(SaArgs A)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < A.n) A.call_off[i] = (A.sel[i] & A.sel_mask) ? A.sa_off[i + 1] - A.sa_off[i] : 0;
}

// v[0 .. n): counts -> exclusive offsets in place, v[n] = *total = their sum; n = *n_dev when given (a count an earlier
// kernel of the stream made), clamped to cap.  One workgroup of 1024: thread t owns a contiguous span (k_bam_scan's shape).
__global__ __launch_bounds__(1024) void k_sa_scan(i64* v, i64 n, const i64* n_dev, i64 cap, i64* total)
{
    __shared__ i64 ws[16];
    const int t = threadIdx.x;
    if (n_dev) n = *n_dev;
    if (n > cap) n = cap;
    const i64 per = (n + 1023) / 1024, b = (i64)t * per < n ? (i64)t * per : n, e = b + per < n ? b + per : n;
    i64 s = 0;
    for (i64 i = b; i < e; i++) s += v[i];
    const i64 inc = wave_incl_scan_i64(s);
    if ((t & 63) == 63) ws[t >> 6] = inc;
    __syncthreads();
    i64 o = inc - s, all = 0;
    for (int q = 0; q < 16; q++) {
        if (q < (t >> 6)) o += ws[q];
        all += ws[q];
    }
    for (i64 i = b; i < e; i++) { const i64 c = v[i]; v[i] = o; o += c; }
    if (t == 0) { v[n] = all; *total = all; }
}

__global__ __launch_bounds__(256) void k_sa_calls(SaArgs A)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    const i64 k0 = A.call_off[i], k1 = A.call_off[i + 1], s0 = A.sa_off[i];
    const i64 ql = A.qlen[i];
    for (i64 k = k0; k < k1 && k < A.cap_calls; k++) { A.call_rec[k] = (int)i; A.call_sa[k] = s0 + (k - k0); A.read_len[k] = ql; }
}

// the ';' among the bytes of the 16-byte block at `blk` that lie inside [beg, end): bit j = byte blk + j
__device__ __forceinline__ unsigned sa_semis(const uint8_t* s, i64 beg, i64 end, i64 blk)
{
    const i64 lo = blk > beg ? blk : beg, hi = blk + 16 < end ? blk + 16 : end;
    unsigned m = 0;
    if (lo >= hi) return 0;
    if (lo == blk && hi == blk + 16) {                       // whole block inside the value: one 16-byte load
        const uint4 v = *(const uint4*)(s + blk);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 16; j++)
            if (((w[j >> 2] >> (8 * (j & 3))) & 255u) == (unsigned)';') m |= 1u << j;
    } else {
        for (i64 q = lo; q < hi; q++)
            if (s[q] == ';') m |= 1u << (int)(q - blk);
    }
    return m;
}

// [b, e) as an unsigned decimal number of 1 .. max_digits ASCII digits: false if it is anything else
__device__ __forceinline__ bool sa_number(const uint8_t* s, i64 b, i64 e, int max_digits, i64& v)
{
    if (e <= b || e - b > max_digits) return false;
    i64 x = 0;
    for (i64 q = b; q < e; q++) {
        const unsigned d = (unsigned)s[q] - (unsigned)'0';
        if (d > 9u) return false;
        x = x * 10 + (i64)d;
    }
    v = x;
    return true;
}

struct SaEnt { i64 c0, c1, f0, f1; int chr, mapq, strand; };

// acquire_clip_pos on the CIGAR text [b, e): leading S, trailing S, span over M D = X (N is not in it, H is no clip here)
__device__ __forceinline__ int sa_cigar(const uint8_t* s, i64 b, i64 e, SaEnt& E)
{
    if (e - b == 1 && s[b] == '*') return 0;
    if (e <= b) return SA_ST_CIGAR;
    i64 span = 0, first_s = 0, last_s = 0;
    bool first = true;
    i64 q = b;
    while (q < e) {
        i64 v = 0;
        int nd = 0;
        while (q < e) {
            const unsigned d = (unsigned)s[q] - (unsigned)'0';
            if (d > 9u) break;
            if (++nd > 18) return SA_ST_CIGAR;
            v = v * 10 + (i64)d;
            q++;
        }
        if (nd == 0 || q >= e) return SA_ST_CIGAR;
        const int c = s[q++];
        if (c == 'M' || c == 'D' || c == '=' || c == 'X') {
            span += v;                                       // (each term < 10^18 < 2^60: the sum is checked before it can wrap)
            if (span > (1ll << 62)) return SA_ST_CIGAR;
        } else if (!(c == 'I' || c == 'N' || c == 'S' || c == 'H' || c == 'P' || c == 'B')) return SA_ST_CIGAR;
        last_s = c == 'S' ? v : 0;
        if (first) { first_s = last_s; first = false; }
    }
    E.c0 = first_s; E.c1 = last_s; E.f1 = span;
    return 0;
}

// rank of the contig named [b, e), or -1: binary search in the sorted name table, bytes compared as unsigned, then lengths
__device__ __forceinline__ int sa_name(const SaArgs& A, i64 b, i64 e)
{
    int lo = 0, hi = A.n_names;
    const i64 len = e - b;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const i64 nb = A.name_off[mid], nl = A.name_off[mid + 1] - nb, m = len < nl ? len : nl;
        int cmp = 0;
        for (i64 k = 0; k < m && cmp == 0; k++) cmp = (int)A.slim[b + k] - (int)A.names[nb + k];
        if (cmp == 0) cmp = len < nl ? -1 : len > nl ? 1 : 0;
        if (cmp == 0) return A.name_rank[mid];
        if (cmp < 0) hi = mid; else lo = mid + 1;
    }
    return -1;
}

// the entry [s, t) (t: its ';'): fields split at ',' like str.split - an empty entry has one empty field
__device__ __forceinline__ int sa_entry(const SaArgs& A, i64 s, i64 t, SaEnt& E)
{
    int st = 0, nf = 0;
    i64 p = s, v = 0;
    E.c0 = E.c1 = E.f0 = E.f1 = 0; E.chr = E.mapq = E.strand = 0;
    while (p <= t && nf < 5) {
        i64 e = p;
        while (e < t && A.slim[e] != ',') e++;
        if (nf == 0) { E.chr = sa_name(A, p, e); if (E.chr < 0) st |= SA_ST_NAME; }
        else if (nf == 1) { if (sa_number(A.slim, p, e, 18, v)) E.f0 = v - 1; else st |= SA_ST_NUMBER; }
        else if (nf == 2) { if (e - p == 1) E.strand = A.slim[p] == '+' ? 0 : 1; else st |= SA_ST_STRAND; }
        else if (nf == 3) st |= sa_cigar(A.slim, p, e, E);
        else { if (sa_number(A.slim, p, e, 9, v)) E.mapq = (int)v; else st |= SA_ST_NUMBER; }
        nf++;
        p = e + 1;
    }
    if (nf < 5) st |= SA_ST_FIELDS;
    return st;
}

// one wavefront per workgroup, one call per wavefront at a time: every loop below runs the same number of times in all
// 64 lanes, so the barriers (and the DPP sums, which need all lanes) are met by the whole workgroup
template <bool EMIT> __global__ __launch_bounds__(64) void k_sa_parse(SaArgs A)
{
    __shared__ unsigned nxt[65];                             // nxt[k]: offset in the value of the byte behind ';' number g - 1 + k
    const int lane = threadIdx.x;
    i64 n_calls = A.tot[0];
    if (n_calls > A.cap_calls) n_calls = A.cap_calls;
    for (i64 call = blockIdx.x; call < n_calls; call += gridDim.x) {
        if (EMIT && A.status[call]) continue;
        const int rec = A.call_rec[call];
        const i64 tag = A.call_sa[call], beg = A.sa_beg[tag], end = A.sa_end[tag];
        const bool prim = A.mapq[rec] >= A.min_mapq;
        const i64 base = beg & ~15ll, nblk = (end - base + 15) >> 4;
        i64 n_semi = 0;
        for (i64 b0 = 0; b0 < nblk; b0 += 64) {
            const unsigned m = b0 + lane < nblk ? sa_semis(A.slim, beg, end, base + (b0 + lane) * 16) : 0u;
            n_semi += wave_sum_i32(__popc(m));
        }
        const i64 o0 = EMIT ? A.ent_off[call] + (prim ? 1 : 0) : 0;
        int st = 0;
        for (i64 g = 0; g < n_semi; g += 64) {
            __syncthreads();                                 // the round before has read nxt
            if (g == 0 && lane == 0) nxt[0] = 0;
            i64 seen = 0;
            for (i64 b0 = 0; b0 < nblk && seen <= g + 63; b0 += 64) {
                const i64 blk = base + (b0 + lane) * 16;
                unsigned m = b0 + lane < nblk ? sa_semis(A.slim, beg, end, blk) : 0u;
                const int c = __popc(m), inc = wave_incl_scan_i32(c);
                i64 k = seen + (inc - c) - (g - 1);          // slot of this lane's first ';'
                while (m) {
                    const int j = __ffs(m) - 1;
                    m &= m - 1;
                    if (k >= 0 && k <= 64) nxt[k] = (unsigned)(blk + j + 1 - beg);
                    k++;
                }
                seen += __builtin_amdgcn_readlane(inc, 63);
            }
            __syncthreads();
            const i64 e = g + lane;
            if (e < n_semi) {
                SaEnt E;
                const int s1 = sa_entry(A, beg + (i64)nxt[lane], beg + (i64)nxt[lane + 1] - 1, E);
                st |= s1;
                const i64 o = o0 + e;
                if (EMIT && o < A.cap_entries) {
                    A.c0[o] = E.c0; A.c1[o] = E.c1; A.f0[o] = E.f0; A.f1[o] = E.f1;
                    A.chr[o] = E.chr; A.emapq[o] = E.mapq; A.strand[o] = (uint8_t)E.strand; A.primary[o] = 0;
                }
            }
        }
        if (!EMIT) {
            int all = 0;
            for (int b = 1; b <= SA_ST_NAME; b <<= 1)
                if (__ballot((st & b) != 0)) all |= b;
            if (lane == 0) {
                A.status[call] = (uint8_t)all;
                A.ent_off[call] = all ? 0 : n_semi + (prim ? 1 : 0);
                if (all) atomicAdd((unsigned long long*)&A.tot[2], 1ull);
            }
        } else if (lane == 0 && prim) {                      // primary_info (:660-668): the clips swap on the reverse strand
            const i64 o = o0 - 1, ql = A.qlen[rec], cl = A.clip_l[rec], cr = A.clip_r[rec];
            const bool fwd = A.flag[rec] == 0;
            if (o < A.cap_entries) {
                A.c0[o] = fwd ? cl : cr; A.c1[o] = ql - (fwd ? cr : cl); A.f0[o] = A.ref_start[rec]; A.f1[o] = A.ref_end[rec];
                A.chr[o] = A.task_rank; A.emapq[o] = 0; A.strand[o] = fwd ? 0 : 1; A.primary[o] = 1;
            }
        }
    }
}

}  // namespace csv
