// bam.hip.h — BAM alignment records -> the columns of the extraction step, on the GPU.
//
// Input: the slim image the host packs while it frames the records (bam_host.cpp): per record the 32 fixed bytes after
// block_size, the CIGAR words and the aux bytes, 16-byte aligned.  Field offsets are the SAM/BAM specification's (4.2):
//   +0 refID  +4 pos  +8 l_read_name  +9 mapq  +10 bin  +12 n_cigar_op  +14 flag  +16 l_seq  +20 next_refID  +24 next_pos  +28 tlen
//
//   k_bam_fixed   one thread per record: fixed fields, flag class, aux walk (SA tags counted, CG:B,I found), the number of
//                 CIGAR operations (the tag's when the record holds the <l_seq>S<n>N placeholder) and where they are
//   k_bam_scan    one workgroup: operation counts -> cig_off, SA counts -> sa_off
//   k_bam_cigar   one wavefront per record (up to BAM_WAVE_MAX operations): copies the words into the packed array - the
//                 packed form IS BAM's oplen << 4 | op - and sums the reference span; 16-byte loads where the source is
//                 aligned (always, outside a CG tag)
//   k_bam_cigar_long   one workgroup per longer record (a list k_bam_fixed appends to)
//   k_bam_sa      one thread per record with SA tags: the walk again, now writing the value ranges
// Every byte a kernel reads lies inside [rec_off, rec_off + rec_len) of its record: the host entry checks those ranges
// against the image, k_bam_fixed checks the CIGAR and every aux value against the record.
//
// At the end of the file, the step in front of all that: k_bgzf_inflate, one wavefront per BGZF block, over the decode core
// of inflate_core.h; and behind it the record framing on the device (frame_core.h):
// k_frame_guess, k_frame_stitch, k_frame_rows find the records of an inflated window that never left the device, k_frame_pack
// builds the slim and the host image from the records the reader selected; and last the index build (index_core.h, DESIGN.md
// section 30): k_index_rows and k_index_runs turn the rows of a framed window into the runs and the linear index of a .bai.  Last of all the
// way back out: k_bgzf_deflate, one wavefront per block over deflate_core.h, and k_deflate_offsets.
// And k_ref_gather: base ranges of a BGZF-compressed FASTA cut out of the blocks k_bgzf_inflate left on the device, one wavefront per
// output tile over ref_core.h; and k_fai_tiles / k_fai_events: the lines of such a text as the event rows its .fai
// is assembled from.  And the coordinate sort of a whole file (sort_core.h): k_sort_keys, k_sort_dst_tiles /
// k_sort_dst_scan and k_sort_gather, the kernel every byte of the file passes through on its way into sorted order.  And the way in from an
// aligner's text (sam_core.h): k_sam_marks, k_sam_plan, k_sam_small and k_sam_bulk turn a window of SAM lines into BAM records.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wave.hip.h"
#include "scan.hip.h"
#include "inflate_core.h"
#include "deflate_core.h"
#include "frame_core.h"
#include "index_core.h"
#include "ref_core.h"
#include "sort_core.h"
#include "sam_core.h"

namespace csv {

constexpr int BAM_WAVE_MAX = 4096;          // operations a wavefront copies (64 steps of 64); longer records get a workgroup
constexpr int BAM_ST_AUX = 1, BAM_ST_CIGAR = 2;

struct BamArgs {
    i64 n;
    const uint8_t* slim;
    const i64* rec_off;
    const unsigned* rec_len;
    i64* ref_start; i64* ref_end; int* flag; int* mapq; int* qlen; int* clip_l; int* clip_r; uint8_t* cls; uint8_t* status;
    i64* cig_off;                   // n + 1: counts (k_bam_fixed), then exclusive offsets (k_bam_scan)
    i64* sa_off;                    // n + 1: likewise, SA tags
    i64* cig_src;                   // byte offset in slim of the record's operation words (the record's own, or the CG tag's)
    i64* cg_beg; i64* cg_end;
    unsigned* cigar;
    i64* sa_beg; i64* sa_end;
    int* long_list;                 // records with more than BAM_WAVE_MAX operations
    int* counters;                  // [0] entries of long_list, [1] records with status != 0
    i64* totals;                    // [0] operations, [1] SA tags
};

struct AuxTag { int k0, k1, type, sub; i64 vbeg, vend; };

// the next tag of the aux area [p, end) of `s`: 1 = read (p moves behind it), 0 = end of the area, -1 = malformed (an
// unknown type byte or a value that does not end inside the area).  Never reads at or beyond `end`.
__device__ __forceinline__ int aux_next(const uint8_t* s, i64& p, const i64 end, AuxTag& t)
{
    if (p >= end) return 0;
    if (end - p < 3) return -1;
    t.k0 = s[p]; t.k1 = s[p + 1]; t.type = s[p + 2]; t.sub = 0;
    p += 3;
    i64 sz = 0;
    switch (t.type) {
    case 'A': case 'c': case 'C': sz = 1; break;
    case 's': case 'S': sz = 2; break;
    case 'i': case 'I': case 'f': sz = 4; break;
    case 'Z': case 'H': {
        i64 q = p;
        while (q < end && s[q]) q++;
        if (q >= end) return -1;                             // no NUL inside the record
        t.vbeg = p; t.vend = q; p = q + 1;
        return 1;
    }
    case 'B': {
        if (end - p < 5) return -1;
        t.sub = s[p];
        const i64 cnt = (i64)s[p + 1] | ((i64)s[p + 2] << 8) | ((i64)s[p + 3] << 16) | ((i64)s[p + 4] << 24);
        i64 es;
        switch (t.sub) {
        case 'c': case 'C': es = 1; break;
        case 's': case 'S': es = 2; break;
        case 'i': case 'I': case 'f': es = 4; break;
        default: return -1;
        }
        p += 5;
        if (cnt > (end - p) / es) return -1;
        t.vbeg = p; t.vend = p + cnt * es; p = t.vend;
        return 1;
    }
    default: return -1;
    }
    if (end - p < sz) return -1;
    t.vbeg = p; t.vend = p + sz; p += sz;
    return 1;
}

__global__ __launch_bounds__(256) void k_bam_fixed(BamArgs A)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    const i64 off = A.rec_off[i], len = A.rec_len[i];       // (host-checked: off % 16 == 0, len >= 32, off + len inside the image)
    const unsigned* w = (const unsigned*)(A.slim + off);
    const i64 pos = (int)w[1];
    const int mapq = (int)((w[2] >> 8) & 255u);
    int n_cig = (int)(w[3] & 0xffffu);
    const int flag = (int)(w[3] >> 16);
    const unsigned l_seq = w[4];
    int st = 0;
    if (32 + 4 * (i64)n_cig > len) { st = BAM_ST_CIGAR; n_cig = 0; }       // the CIGAR leaves the record: treated as empty, reported
    i64 n_ops = n_cig, src = off + 32, cgb = -1, cge = -1;
    int n_sa = 0;
    i64 p = off + 32 + 4 * (i64)n_cig;
    const i64 end = off + len;
    AuxTag t;
    int rc;
    while ((rc = aux_next(A.slim, p, end, t)) == 1) {
        if (t.k0 == 'S' && t.k1 == 'A' && t.type == 'Z') n_sa++;
        else if (t.k0 == 'C' && t.k1 == 'G' && t.type == 'B' && t.sub == 'I' && cgb < 0) { cgb = t.vbeg; cge = t.vend; }
    }
    if (rc < 0) st |= BAM_ST_AUX;
    // more than 65 535 operations: the record holds <l_seq>S<reference length>N and the real CIGAR is the CG array (SAM spec 4.2.2)
    if (n_cig == 2 && cgb >= 0 && (w[8] & 15u) == 4u && (w[8] >> 4) == l_seq && (w[9] & 15u) == 3u) { n_ops = (cge - cgb) >> 2; src = cgb; }
    A.ref_start[i] = pos; A.flag[i] = flag; A.mapq[i] = mapq; A.qlen[i] = (int)l_seq;
    A.cls[i] = (flag == 256 || flag == 272) ? 0 : (flag == 0 || flag == 16) ? 1 : 2;
    A.status[i] = (uint8_t)st;
    A.cig_off[i] = n_ops; A.sa_off[i] = n_sa; A.cig_src[i] = src; A.cg_beg[i] = cgb; A.cg_end[i] = cge;
    if (n_ops > BAM_WAVE_MAX) A.long_list[atomicAdd(&A.counters[0], 1)] = (int)i;
    if (st) atomicAdd(&A.counters[1], 1);
}

// counts -> exclusive offsets, both columns, in place; one workgroup of 1024: thread t owns a contiguous span of records
__global__ __launch_bounds__(1024) void k_bam_scan(BamArgs A)
{
    __shared__ i64 ws[2][16];
    const int t = threadIdx.x;
    const i64 per = (A.n + 1023) / 1024, b = (i64)t * per < A.n ? (i64)t * per : A.n, e = b + per < A.n ? b + per : A.n;
    i64 s0 = 0, s1 = 0;
    for (i64 i = b; i < e; i++) { s0 += A.cig_off[i]; s1 += A.sa_off[i]; }
    const i64 i0 = wave_incl_scan_i64(s0), i1 = wave_incl_scan_i64(s1);
    if ((t & 63) == 63) { ws[0][t >> 6] = i0; ws[1][t >> 6] = i1; }
    __syncthreads();
    i64 o0 = i0 - s0, o1 = i1 - s1, tot0 = 0, tot1 = 0;
    for (int q = 0; q < 16; q++) {
        if (q < (t >> 6)) { o0 += ws[0][q]; o1 += ws[1][q]; }
        tot0 += ws[0][q]; tot1 += ws[1][q];
    }
    for (i64 i = b; i < e; i++) {
        const i64 c0 = A.cig_off[i], c1 = A.sa_off[i];
        A.cig_off[i] = o0; A.sa_off[i] = o1;
        o0 += c0; o1 += c1;
    }
    if (t == 0) { A.cig_off[A.n] = tot0; A.sa_off[A.n] = tot1; A.totals[0] = tot0; A.totals[1] = tot1; }
}

__device__ __forceinline__ i64 ref_len_of(unsigned w)
{
    const unsigned op = w & 15u;
    return (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) ? (i64)(w >> 4) : 0;     // M D N = X
}

__device__ __forceinline__ unsigned load_op(const uint8_t* s, i64 at)          // an operation word at any byte alignment
{
    if ((at & 3) == 0) return *(const unsigned*)(s + at);
    return (unsigned)s[at] | ((unsigned)s[at + 1] << 8) | ((unsigned)s[at + 2] << 16) | ((unsigned)s[at + 3] << 24);
}

// threads t of nt copy the n operation words at byte `src` of the image to dst; returns this thread's share of the reference span
__device__ __forceinline__ i64 copy_ops(const uint8_t* slim, i64 src, unsigned* dst, i64 n, int t, int nt)
{
    i64 span = 0;
    if ((src & 15) == 0) {                                   // 16 bytes per lane: a wavefront moves 1 KiB per step
        const uint4* s4 = (const uint4*)(slim + src);
        const i64 n4 = n >> 2;
        for (i64 k = t; k < n4; k += nt) {
            const uint4 v = s4[k];
            dst[4 * k] = v.x; dst[4 * k + 1] = v.y; dst[4 * k + 2] = v.z; dst[4 * k + 3] = v.w;
            span += ref_len_of(v.x) + ref_len_of(v.y) + ref_len_of(v.z) + ref_len_of(v.w);
        }
        const unsigned* s1 = (const unsigned*)(slim + src);
        for (i64 k = 4 * n4 + t; k < n; k += nt) { const unsigned v = s1[k]; dst[k] = v; span += ref_len_of(v); }
    } else {                                                 // a CG array sits wherever the tags before it end
        for (i64 k = t; k < n; k += nt) { const unsigned v = load_op(slim, src + 4 * k); dst[k] = v; span += ref_len_of(v); }
    }
    return span;
}

__device__ __forceinline__ void bam_finish(const BamArgs& A, i64 r, i64 n_ops, i64 src, i64 span)
{
    int cl = 0, cr = 0;
    if (n_ops > 0) {
        const unsigned f = load_op(A.slim, src), l = load_op(A.slim, src + 4 * (n_ops - 1));
        if ((f & 15u) == 4u || (f & 15u) == 5u) cl = (int)(f >> 4);            // S, or the H that replaces it
        if ((l & 15u) == 4u || (l & 15u) == 5u) cr = (int)(l >> 4);
    }
    A.ref_end[r] = A.ref_start[r] + span; A.clip_l[r] = cl; A.clip_r[r] = cr;
}

__global__ __launch_bounds__(256) void k_bam_cigar(BamArgs A)
{
    const i64 wave = ((i64)blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = ((i64)gridDim.x * 256) >> 6;
    const int lane = lane_id();
    for (i64 r = wave; r < A.n; r += nwaves) {
        const i64 c0 = A.cig_off[r], n_ops = A.cig_off[r + 1] - c0;
        if (n_ops > BAM_WAVE_MAX) continue;                  // k_bam_cigar_long's
        const i64 src = A.cig_src[r];
        const i64 span = wave_sum_i64(copy_ops(A.slim, src, A.cigar + c0, n_ops, lane, 64));
        if (lane == 0) bam_finish(A, r, n_ops, src, span);
    }
}

__global__ __launch_bounds__(256) void k_bam_cigar_long(BamArgs A)
{
    __shared__ i64 sh[4];
    const i64 r = A.long_list[blockIdx.x];
    const i64 c0 = A.cig_off[r], n_ops = A.cig_off[r + 1] - c0, src = A.cig_src[r];
    const i64 part = wave_sum_i64(copy_ops(A.slim, src, A.cigar + c0, n_ops, (int)threadIdx.x, 256));
    if (lane_id() == 0) sh[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) bam_finish(A, r, n_ops, src, sh[0] + sh[1] + sh[2] + sh[3]);
}

__global__ __launch_bounds__(256) void k_bam_sa(BamArgs A)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    i64 o = A.sa_off[i];
    const i64 o_end = A.sa_off[i + 1];
    if (o_end <= o) return;
    const i64 off = A.rec_off[i], end = off + A.rec_len[i];
    const unsigned* w = (const unsigned*)(A.slim + off);
    i64 p = off + 32 + 4 * (i64)(w[3] & 0xffffu);           // (the CIGAR fits: a record where it does not has no SA count)
    if (A.status[i] & BAM_ST_CIGAR) p = off + 32;
    AuxTag t;
    while (o < o_end && aux_next(A.slim, p, end, t) == 1)
        if (t.k0 == 'S' && t.k1 == 'A' && t.type == 'Z') { A.sa_beg[o] = t.vbeg; A.sa_end[o] = t.vend; o++; }
}

// ------------------------------------------------------------------------------------ BGZF inflate
// The 64-lane form of inflate_core.h's Lanes.  uni: v_readfirstlane, so whatever the decode core decides on lives in scalar
// registers and every branch on it is a scalar branch: all 64 lanes leave a block together, none waits at a shuffle the others
// skipped.  sync: a wavefront's LDS and global accesses are issued in order, so a fence of wavefront scope - an ordering for the
// compiler, no instruction - is all a lane needs to see what another lane of its wave wrote.
struct InfWave {
    __device__ __forceinline__ int lane() const { return lane_id(); }
    __device__ __forceinline__ int width() const { return WAVE; }
    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ __forceinline__ void sync() const
    {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    // a * b in GF(2)[x] modulo the CRC32 polynomial, reflected: bit 31 is x^0
    static __device__ __forceinline__ uint32_t mul(uint32_t a, uint32_t b)
    {
        uint32_t p = 0;
        for (int k = 0; k < 32; k++) {
            if (a & (0x80000000u >> k)) p ^= b;
            b = (b >> 1) ^ ((b & 1u) ? 0xEDB88320u : 0u);
        }
        return p;
    }
    // CRC32 of out[0 .. len), len >= 1: the bytes are cut into 64 pieces of c = ceil(len / 64) - as if 64 c - len zero bytes stood
    // in front, which leave a register of zero as it is; the lane that holds byte 0 starts from 0xffffffff there.  Lane l's
    // register r_l then counts for r_l * x^(8 c (63 - l)): six rounds of "left half times x^(8 c s), plus right half".
    __device__ __forceinline__ uint32_t crc(const uint8_t* out, int32_t len, const uint32_t* table) const
    {
        const int c = (len + 63) >> 6, l = lane_id();
        int lo = l * c - (64 * c - len);
        const int hi = lo + c;                                    // (hi <= len: lane 63 ends at 64 c - (64 c - len))
        uint32_t r = 0;
        if (hi > 0) {
            if (lo <= 0) { r = 0xffffffffu; lo = 0; }
            for (int i = lo; i < hi; i++) r = table[(r ^ out[i]) & 255u] ^ (r >> 8);
        }
        uint32_t q = 0x80000000u;                                 // x^0 -> x^(8 c): c zero bytes through the register
        for (int i = 0; i < c; i++) q = table[q & 255u] ^ (q >> 8);
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t right = (uint32_t)__shfl_down((int)r, s);
            if ((l & (2 * s - 1)) == 0) r = mul(r, q) ^ right;
            q = mul(q, q);
        }
        return uni(r) ^ 0xffffffffu;
    }
};

struct InflateArgs {
    int n;                          // BGZF blocks
    const uint8_t* comp;            // block k's raw-deflate payload: comp[in_off[k] .. + in_len[k])
    const i64* in_off; const int* in_len;
    const i64* out_off; const int* out_len;     // its bytes: out[out_off[k] .. + out_len[k]), host-checked: inside `out`, disjoint, at most 65536
    const unsigned* crc;
    uint8_t* out;
    uint8_t* status;
};

constexpr int INF_WAVES = 4;        // wavefronts (BGZF blocks in flight) per workgroup

// One wavefront per BGZF block, a grid-stride loop over the blocks.  No workgroup barrier behind the first: the four waves of a
// workgroup share nothing but the CRC table.  LDS: 4 * sizeof(InfWork) + 1 KiB = 10 KiB per workgroup.
__global__ __launch_bounds__(64 * INF_WAVES) void k_bgzf_inflate(InflateArgs A)
{
    __shared__ InfWork work[INF_WAVES];
    __shared__ uint32_t crc_table[256];
    crc_table[threadIdx.x] = inf_crc_entry(threadIdx.x);
    __syncthreads();
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const InfWave L;
    for (i64 k = (i64)blockIdx.x * INF_WAVES + w; k < A.n; k += (i64)gridDim.x * INF_WAVES) {
        const int out_len = A.out_len[k];
        int st = 0;
        if (out_len > 0) st = inf_block(L, work[w], A.comp + A.in_off[k], A.in_len[k], A.out + A.out_off[k], out_len, A.crc[k], crc_table);
        if (L.lane() == 0) A.status[k] = (uint8_t)st;
    }
}

// ------------------------------------------------------------------------------------ record framing
// The 64-lane form of frame_core.h's Lanes.  first / sum are called where the wavefront has converged: fr_guess evaluates the
// test of every lane before the call, fr_row leaves its strided loop before it.
struct FrWave {
    __device__ __forceinline__ int lane() const { return lane_id(); }
    __device__ __forceinline__ int width() const { return WAVE; }
    __device__ __forceinline__ int first(bool p) const
    {
        const u64 m = __ballot(p ? 1 : 0);
        return m ? __ffsll((long long)m) - 1 : -1;
    }
    __device__ __forceinline__ fr_i64 sum(fr_i64 v) const { return wave_sum_i64(v); }
};

struct FrameArgs {
    FrWin W;                        // the window (device memory) and the file's n_ref
    int n_blocks;                   // BGZF blocks of the window, in stream order
    i64 c;                          // the cursor: a true record start
    const i64* blk_off; const int* blk_len;     // host-checked: contiguous from 0, inside [0, W.n], at most 65536 each
    const i64* slot_off;            // block s's slot in `starts`: fr_slot_size(blk_len[s]) entries
    i64* g; i64* ex; int* cnt;      // per block: the guess, where its chain landed, the starts it met
    i64* starts;
    int* used;                      // per block: the starts that are the true chain's (k_frame_stitch)
    int4* scan;                     // per block: used -> exclusive row offsets (scan_counts)
    FrStitch* res;
    FrRow* rows;
};

constexpr int FRAME_WAVES = 4;

// one wavefront per BGZF block: the guess (64 offsets a round), then lane 0 chases the chain through the block
__global__ __launch_bounds__(64 * FRAME_WAVES) void k_frame_guess(FrameArgs A)
{
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const FrWave L;
    for (i64 s = (i64)blockIdx.x * FRAME_WAVES + w; s < A.n_blocks; s += (i64)gridDim.x * FRAME_WAVES) {
        const i64 b = A.blk_off[s], e = b + A.blk_len[s];
        i64 g = -1, ex = -1;
        int cnt = 0;
        if (e > A.c) {                                           // (a block in front of the cursor is never landed in)
            g = b <= A.c ? A.c : fr_guess(L, A.W, b, e);
            if (g >= 0 && L.lane() == 0) ex = fr_chase(A.W, g, e, A.starts + A.slot_off[s], fr_slot_size(A.blk_len[s]), &cnt);
        }
        if (L.lane() == 0) { A.g[s] = g; A.ex[s] = ex; A.cnt[s] = cnt; }
    }
}

// one wavefront: lane 0 walks from the cursor block by block (fr_stitch), then the lanes lay out the counts for the scan
__global__ __launch_bounds__(64) void k_frame_stitch(FrameArgs A)
{
    if (threadIdx.x == 0) fr_stitch(A.W, A.n_blocks, A.blk_off, A.blk_len, A.slot_off, A.g, A.ex, A.cnt, A.starts, A.used, A.c, A.res);
    __syncthreads();
    for (int s = threadIdx.x; s < A.n_blocks; s += 64) A.scan[s] = make_int4(A.used[s], 0, 0, 0);
}

// one wavefront per block: the rows of its records (the lanes share a record's CIGAR sum); scan[s].x = the block's first row
__global__ __launch_bounds__(64 * FRAME_WAVES) void k_frame_rows(FrameArgs A, i64 n_rows)
{
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const FrWave L;
    for (i64 s = (i64)blockIdx.x * FRAME_WAVES + w; s < A.n_blocks; s += (i64)gridDim.x * FRAME_WAVES) {
        const int n = __builtin_amdgcn_readfirstlane(A.used[s]);
        const i64 base = A.scan[s].x, slot = A.slot_off[s];
        for (int j = 0; j < n; j++) {
            const i64 o = A.starts[slot + j];
            FrRow r = fr_row(L, A.W, o);
            if (L.lane() == 0 && base + j < n_rows) A.rows[base + j] = r;
        }
    }
}

// L bytes from src to dst with the lanes of a wavefront: aligned words of dst between a byte head and a byte tail
__device__ __forceinline__ void frame_copy(const uint8_t* src, i64 L, uint8_t* dst, int lane)
{
    i64 head = (i64)((4 - ((uintptr_t)dst & 3)) & 3);
    head = head < L ? head : L;
    if (lane < head) dst[lane] = src[lane];
    const i64 nw = (L - head) >> 2;
    for (i64 w = lane; w < nw; w += 64) {
        const i64 j = head + 4 * w;
        *(unsigned*)(dst + j) = (unsigned)src[j] | ((unsigned)src[j + 1] << 8) | ((unsigned)src[j + 2] << 16) | ((unsigned)src[j + 3] << 24);
    }
    const i64 t0 = head + 4 * nw;
    if (lane < L - t0) dst[t0 + lane] = src[t0 + lane];
}

// one wavefront per selected record: fixed fields, CIGAR words and aux bytes into the slim image (padded with zeros to 16
// bytes), name and 4-bit sequence into the host image - the layout bam_host.cpp packs on the host route
__global__ __launch_bounds__(256) void k_frame_pack(const uint8_t* win, const FrPack* P, i64 n, uint8_t* slim, uint8_t* host)
{
    const int lane = lane_id();
    for (i64 r = ((i64)blockIdx.x * 256 + threadIdx.x) >> 6; r < n; r += ((i64)gridDim.x * 256) >> 6) {
        const FrPack p = P[r];
        const i64 l_name = p.l_name, cig = 4 * (i64)p.n_cig, seq = ((i64)p.l_seq + 1) / 2;
        const i64 fixed_to_aux = 32 + l_name + cig + seq + (i64)p.l_seq, aux_len = (i64)p.bs - fixed_to_aux, slim_len = 32 + cig + aux_len;
        const uint8_t* s = win + p.src + 4;
        uint8_t* d = slim + p.rec_off;
        frame_copy(s, 32, d, lane);
        frame_copy(s + 32 + l_name, cig, d + 32, lane);
        frame_copy(s + fixed_to_aux, aux_len, d + 32 + cig, lane);
        const i64 pad = (slim_len + 15) / 16 * 16 - slim_len;
        if (lane < pad) d[slim_len + lane] = 0;
        uint8_t* h = host + p.host_off;
        frame_copy(s + 32, l_name, h, lane);
        frame_copy(s + 32 + l_name + cig, seq, h + l_name, lane);
    }
}

// one wavefront per item: len[i] bytes at src + src_off[i] -> dst + dst_off[i] (host-checked ranges); the names and the 4-bit
// sequences of a device chunk on their way into the name pool and the read sequences
__global__ __launch_bounds__(256) void k_frame_gather(const uint8_t* src, const i64* src_off, const int* len, i64 n, uint8_t* dst, const i64* dst_off)
{
    const int lane = lane_id();
    for (i64 r = ((i64)blockIdx.x * 256 + threadIdx.x) >> 6; r < n; r += ((i64)gridDim.x * 256) >> 6)
        if (len[r] > 0) frame_copy(src + src_off[r], len[r], dst + dst_off[r], lane);
}

// ------------------------------------------------------------------------------------ index build
// The rows k_frame_rows left in device memory -> the work of a BAM index (index_core.h), window by window: k_index_rows, one thread
// per record, scan_counts over the head flags, k_index_runs.  What the kernels trust is host-checked: n rows, the tables' sizes.
struct IxAux { u64 vbeg, vend; int ref; unsigned bin; int pos; int head; };       // per record, between the two kernels (32 bytes)

struct IndexArgs {
    const uint8_t* win; i64 win_n;  // the window (device memory): the flag of a record is read there
    i64 win_u0;                     // the stream offset of the window's first byte
    const FrRow* rows; i64 n;       // the framed records of the window, in file order
    i64 ordinal0;                   // the ordinal of rows[0] in the file
    IxCarry carry;                  // the record in front of rows[0]
    IxBlocks blocks;                // the whole-file block table
    int n_ref; const i64* l_ref; const i64* lin_off;
    IxFormat fmt;                   // the binning scheme: BAI's, or a CSI index's own
    u64* lin;                       // the linear arrays of the whole build: IX_NONE or the smallest virtual offset so far
    u64* counts;                    // mapped, unmapped per reference; then the records without coordinates
    IxAux* aux; int4* scan; const i64* totals;
    IxVerdict* verdict; IxRun* runs;
};

// one thread per record: bin, windows, both virtual offsets, the head flag against the predecessor, the refusals, the linear index
// (a 64-bit atomicMin per touched window: the first IX_LANE_WINDOWS by the record's lane, the rest by the whole wavefront), the
// counts (one atomic per wavefront and reference).  No lane leaves before the end: the ballots see the whole wavefront.
__global__ __launch_bounds__(256) void k_index_rows(IndexArgs A)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < A.n;
    const int lane = lane_id();
    IxAux x;
    x.vbeg = 0; x.vend = 0; x.ref = -1; x.bin = 0; x.pos = 0; x.head = 0;
    IxRec r = ix_record(0, 0, A.fmt);
    bool ok = false, unmapped = false;
    if (live) {
        const FrRow w = A.rows[i];
        IxCarry prev = A.carry;
        if (i > 0) {
            const FrRow q = A.rows[i - 1];
            prev.valid = 1; prev.ref = q.refid; prev.pos = q.pos; prev.bin = ix_record(q.pos, q.span, A.fmt).bin;
        }
        r = ix_record(w.pos, w.span, A.fmt);
        x.ref = w.refid; x.pos = w.pos; x.bin = r.bin;
        const int why = ix_refuse(w.refid, w.pos, r, A.n_ref, A.l_ref, prev, A.fmt);
        if (why != IX_OK) atomicMin((u64*)&A.verdict->bad, ((u64)(A.ordinal0 + i) << 3) | (u64)why);
        ok = why == IX_OK;
        const i64 u = A.win_u0 + w.off;
        x.vbeg = ix_voff(A.blocks, u); x.vend = ix_voff(A.blocks, u + 4 + (i64)w.block_size);
        if (w.off >= 0 && w.off + 20 <= A.win_n) unmapped = ((fr_u32(A.win, w.off + 16) >> 16) & 4u) != 0;      // flag_nc: flag << 16 | n_cigar_op
        x.head = ok && w.refid >= 0 && (!prev.valid || prev.ref != w.refid || prev.bin != r.bin) ? 1 : 0;
        if (!ok) x.ref = -1;                                     // (a refused record belongs to no run: the build fails anyway)
        A.aux[i] = x;
        A.scan[i] = make_int4(x.head, 0, 0, 0);
    }
    const bool mapped_ref = ok && x.ref >= 0;
    // the linear index: every window of [w0, w1] lies inside the reference's entries (ix_refuse: end <= max(l_ref, 1), end <= max_pos)
    u64* io = A.lin + (mapped_ref ? A.lin_off[x.ref] : 0);
    const int nw = mapped_ref ? r.w1 - r.w0 + 1 : 0;
    for (int k = 0; k < IX_LANE_WINDOWS; k++) if (k < nw) atomicMin(io + r.w0 + k, x.vbeg);
    u64 wide = __ballot(nw > IX_LANE_WINDOWS ? 1 : 0);
    while (wide) {
        const int src = __ffsll((long long)wide) - 1;
        wide &= wide - 1;
        const int ref = __shfl(x.ref, src), w0 = __shfl(r.w0, src) + IX_LANE_WINDOWS, w1 = __shfl(r.w1, src);
        const u64 v = (u64)shfl_i64((i64)x.vbeg, src);
        u64* row = A.lin + A.lin_off[ref];
        for (int w = w0 + lane; w <= w1; w += WAVE) atomicMin(row + w, v);
    }
    // the counts: the file is sorted, so a wavefront is almost always of one reference
    u64 todo = __ballot(ok ? 1 : 0);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        const int ref = __shfl(x.ref, src);
        const u64 same = __ballot(ok && x.ref == ref ? 1 : 0), un = __ballot(ok && x.ref == ref && unmapped ? 1 : 0);
        if (lane == src) {
            if (ref < 0) atomicAdd(A.counts + 2 * (i64)A.n_ref, (u64)__popcll(same));
            else {
                if (same & ~un) atomicAdd(A.counts + 2 * (i64)ref, (u64)__popcll(same & ~un));
                if (un) atomicAdd(A.counts + 2 * (i64)ref + 1, (u64)__popcll(un));
            }
        }
        todo &= ~same;
    }
}

// one thread per record, behind the scan of the head flags (scan[i].x: the heads in front of record i).  The head of run r writes
// beg, ref and bin, the run's last record writes end and the record count (the head's row is found in the scan by bisection).  A
// window whose first record is no head opens with a `continues` row.  Record n - 1 leaves the carry, record 0 the number of rows.
__global__ __launch_bounds__(256) void k_index_runs(IndexArgs A)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    const IxAux x = A.aux[i];
    const IxAux x0 = A.aux[0];
    const int cont = x0.ref >= 0 && !x0.head ? 1 : 0;
    if (i == 0) A.verdict->n_runs = A.totals[0] + cont;
    if (i == A.n - 1) {
        const FrRow w = A.rows[i];                               // (the record as it is in the file, refused or not)
        A.verdict->last = IxCarry{1, w.refid, w.pos, ix_record(w.pos, w.span, A.fmt).bin};
    }
    if (x.ref < 0) return;
    const i64 heads = (i64)A.scan[i].x + x.head;                 // heads up to and including this record
    const i64 run = heads - 1 + cont;
    if (run < 0 || run >= A.n) return;                           // (cannot happen: a record without a head in front of it is under `cont`)
    if (x.head || i == 0) {
        IxRun* R = A.runs + run;
        R->beg = x.vbeg; R->ref = x.ref; R->bin = x.bin; R->continues = x.head ? 0u : 1u;
    }
    bool last = i == A.n - 1;
    if (!last) { const IxAux y = A.aux[i + 1]; last = y.ref < 0 || y.head; }
    if (last) {
        i64 lo = 0;                                              // the run's first record: 0, or the row where scan.x reaches heads - 1 last
        if (heads > 0) {
            i64 hi = i + 1;                                      // the largest j <= i with scan[j].x == heads - 1
            lo = 0;
            while (hi - lo > 1) { const i64 m = (lo + hi) / 2; if ((i64)A.scan[m].x <= heads - 1) lo = m; else hi = m; }
        }
        IxRun* R = A.runs + run;
        R->end = x.vend; R->n_records = (unsigned)(i - lo + 1);
    }
}

// The loffset of a CSI bin: the filled linear entry at the bin's first window, bot - the first touched entry from
// there on, as empty windows are filled from the next touched one.  One wavefront per (ref, bin) pair reads the reference's array from
// lin[at[k]] on, 64 entries a step, up to lin + end[k] (the end of the reference's entries), and the lowest lane of the ballot that
// holds a touched entry writes it; IX_NONE when there is none (the host refuses that: a bin that holds records has a touched window
// inside its span).  The host checked at[k] <= end[k] <= the array's size.  8 bytes per bin, no dependency between wavefronts.
struct IndexLoffArgs { const u64* lin; const i64* at; const i64* end; u64* loff; i64 n; };

__global__ __launch_bounds__(256) void k_index_loff(IndexLoffArgs A)
{
    const int lane = lane_id();
    for (i64 k = ((i64)blockIdx.x * 256 + threadIdx.x) >> 6; k < A.n; k += ((i64)gridDim.x * 256) >> 6) {
        const i64 e = A.end[k];
        u64 found = IX_NONE;
        for (i64 w = A.at[k]; w < e; w += WAVE) {                // (k, w and e are the wavefront's: every lane makes the same turns)
            const u64 v = w + lane < e ? A.lin[w + lane] : IX_NONE;
            const u64 hit = __ballot(v != IX_NONE ? 1 : 0);
            if (hit) { found = (u64)shfl_i64((i64)v, __ffsll((long long)hit) - 1); break; }
        }
        if (lane == 0) A.loff[k] = found;
    }
}

// ------------------------------------------------------------------------------------ BGZF deflate
// The 64-lane form of deflate_core.h's Lanes, over InfWave.  amax / add / or32: LDS atomics on results that do not depend on the
// order of arrival; ballot_nz and scan64 are called where the wavefront has converged (the tile loops of the core).
struct DflWave : InfWave {
    __device__ __forceinline__ void amax(uint32_t* p, uint32_t v) const { atomicMax(p, v); }
    __device__ __forceinline__ void add(uint32_t* p, uint32_t v) const { atomicAdd(p, v); }
    __device__ __forceinline__ void or32(uint32_t* p, uint32_t v) const { atomicOr(p, v); }
    __device__ __forceinline__ uint64_t ballot_nz(const uint16_t* a) const { return __ballot(a[lane_id()] != 0 ? 1 : 0); }
    __device__ __forceinline__ uint32_t scan64(uint32_t* a) const
    {
        const int v = (int)a[lane_id()], inc = wave_incl_scan_i32(v);
        a[lane_id()] = (uint32_t)(inc - v);
        return (uint32_t)__builtin_amdgcn_readlane(inc, 63);
    }
};

struct DeflateArgs {
    int n;                          // input blocks
    const uint8_t* in;              // block k: in[in_off[k] .. + in_len[k]), host-checked: inside `in`, at most DFL_MAX_IN bytes
    const i64* in_off; const int* in_len;
    uint8_t* slots;                 // block k's BGZF block: slots[k * DFL_SLOT ..)
    uint32_t* tok;                  // DFL_MAX_IN words per wavefront of the grid
    int* size;                      // per block: the size of its BGZF block
};

constexpr int DFL_WAVES = 2;        // wavefronts per workgroup: 2 * sizeof(DflWork) + 1 KiB = 45 KiB of LDS, three workgroups on a CU

// One wavefront per input block, a grid-stride loop over the blocks.  No workgroup barrier behind the first.
__global__ __launch_bounds__(64 * DFL_WAVES) void k_bgzf_deflate(DeflateArgs A)
{
    __shared__ DflWork work[DFL_WAVES];
    __shared__ uint32_t crc_table[256];
    for (int i = threadIdx.x; i < 256; i += 64 * DFL_WAVES) crc_table[i] = inf_crc_entry((uint32_t)i);
    __syncthreads();
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const DflWave L;
    uint32_t* tok = A.tok + ((i64)blockIdx.x * DFL_WAVES + w) * DFL_MAX_IN;
    for (i64 k = (i64)blockIdx.x * DFL_WAVES + w; k < A.n; k += (i64)gridDim.x * DFL_WAVES) {
        const int size = dfl_block(L, work[w], A.in + A.in_off[k], A.in_len[k], tok, A.slots + k * DFL_SLOT, crc_table, nullptr);
        if (L.lane() == 0) A.size[k] = size;
    }
}

// one workgroup: the sizes -> where each block starts in the file image (dst_off, and n entries of slot offsets for k_frame_gather);
// total[0] = the image's size.  Thread t sums a run of ceil(n / 256) blocks, thread 0 scans the 256 sums.
__global__ __launch_bounds__(256) void k_deflate_offsets(const int* size, i64 n, i64* src_off, i64* dst_off, i64* total)
{
    __shared__ i64 part[256];
    const i64 per = (n + 255) / 256, b = (i64)threadIdx.x * per, e = b + per < n ? b + per : n;
    i64 s = 0;
    for (i64 k = b; k < e; k++) s += size[k];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        i64 run = 0;
        for (int t = 0; t < 256; t++) { const i64 v = part[t]; part[t] = run; run += v; }
        total[0] = run;
    }
    __syncthreads();
    s = part[threadIdx.x];
    for (i64 k = b; k < e; k++) { src_off[k] = k * DFL_SLOT; dst_off[k] = s; s += size[k]; }
}

// ------------------------------------------------------------------------------------ reference gather
// The 64-lane form of ref_core.h's Lanes.
struct RefWave {
    __device__ __forceinline__ int lane() const { return lane_id(); }
    __device__ __forceinline__ int width() const { return WAVE; }
};

struct RefGatherArgs {
    RefBlocks B;                    // the touched blocks, inflated back to back in device memory (k_bgzf_inflate wrote them)
    i64 n_ranges, n_tiles;
    const i64* tile_first;          // n_ranges + 1: the tiles in front of a range
    const i64* out_off;             // n_ranges + 1: where a range's bases start in `out`
    const i64* base_off; const int* lb; const int* lw; const i64* beg;     // host-checked: every source byte lies in a block
    uint8_t* out;
};

// One wavefront per output tile of REF_TILE bases, a grid-stride loop over the tiles: the tile's range and the block of its first
// source byte by binary search, then base by base with the line arithmetic (ref_core.h).  No LDS, no barrier.
__global__ __launch_bounds__(256) void k_ref_gather(RefGatherArgs A)
{
    const RefWave L;
    for (i64 t = ((i64)blockIdx.x * 256 + threadIdx.x) >> 6; t < A.n_tiles; t += ((i64)gridDim.x * 256) >> 6)
        ref_gather_tile(L, A.B, A.n_ranges, A.tile_first, A.out_off, A.base_off, A.lb, A.lw, A.beg, t, A.out);
}

// ------------------------------------------------------------------------------------ .fai event rows
// The line breaks of a window of FASTA text that k_bgzf_inflate left on the device, as ref_core.h's event rows.  A workgroup takes a
// tile of FAI_TILE bytes, each of its four wavefronts a quarter of it, 64 bytes a step: one ballot per step says where the line
// breaks are, and the line break before a lane's own (and the one before that: the row rule compares a line with the line before) is
// a bit of the same ballot or the wavefront's running pair.  What runs into a wavefront from the left - the running "previous line
// break" - is the maximum over everything before it: k_fai_tiles leaves the last two line breaks of every tile, and a tile folds the
// tiles before it with wave_incl_max_i64 and its own wavefronts' pairs through LDS.  Three launches over the window: k_fai_tiles,
// k_fai_events<false> (rows per wavefront -> cnt), k_fai_events<true> (cnt summed by block_prefix_of -> where a wavefront's rows go).
// Bounds: a byte is read at 0 <= i < n only (fai_row reads a line's first and last byte, both inside [0, e)); a row is written at
// an index below row_cap only; cnt has 4 and top 2 entries per tile.
constexpr int FAI_TILE = 32768, FAI_WAVE_BYTES = FAI_TILE / 4;

struct FaiOut { i64 n_rows; FaiCarry tail; };

struct FaiArgs {
    const uint8_t* d; i64 n, base;  // the window: n > 0 bytes whose first has absolute offset base
    FaiCarry c;
    int n_tiles;
    i64* top;                       // 2 per tile: its last line break and the one before, window-relative (FAI_NONE: none)
    int* cnt;                       // 4 per tile: the rows of each wavefront
    FaiRow* rows; i64 row_cap;
    FaiOut* out;
};

// the pair (m1 > m2) after the line breaks `mask` of the 64 bytes at p0
__device__ __forceinline__ void fai_push(u64 mask, i64 p0, i64& m1, i64& m2)
{
    if (!mask) return;
    const int hi = 63 - __builtin_clzll(mask);
    const u64 rest = mask & ~(1ull << hi);
    m2 = rest ? p0 + (63 - __builtin_clzll(rest)) : m1;
    m1 = p0 + hi;
}

// the last two line breaks of bytes [lo, hi) (a wavefront's share): wave-uniform
__device__ __forceinline__ void fai_wave_top2(const uint8_t* d, i64 lo, i64 hi, i64& m1, i64& m2)
{
    m1 = m2 = FAI_NONE;
    for (i64 p0 = lo; p0 < hi; p0 += WAVE) {
        const i64 i = p0 + lane_id();
        fai_push(__ballot(i < hi && d[i] == '\n' ? 1 : 0), p0, m1, m2);
    }
}

// the four wavefronts' pairs in sh[2 w], sh[2 w + 1] (in order of position) on top of (m1, m2): the pair after wavefronts [0, upto)
__device__ __forceinline__ void fai_fold(const i64* sh, int upto, i64& m1, i64& m2)
{
    for (int w = 0; w < upto; w++) {
        const i64 a = sh[2 * w], b = sh[2 * w + 1];
        if (a == FAI_NONE) continue;
        m2 = b != FAI_NONE ? b : m1;
        m1 = a;
    }
}

__global__ __launch_bounds__(256) void k_fai_tiles(FaiArgs A)
{
    __shared__ i64 sh[8];
    const int w = threadIdx.x >> 6;
    const i64 t0 = (i64)blockIdx.x * FAI_TILE, lo = t0 + (i64)w * FAI_WAVE_BYTES, hi = lo + FAI_WAVE_BYTES < A.n ? lo + FAI_WAVE_BYTES : A.n;
    i64 m1, m2;
    fai_wave_top2(A.d, lo, hi, m1, m2);
    if (lane_id() == 0) { sh[2 * w] = m1; sh[2 * w + 1] = m2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        i64 a = FAI_NONE, b = FAI_NONE;
        fai_fold(sh, 4, a, b);
        A.top[2 * (i64)blockIdx.x] = a; A.top[2 * (i64)blockIdx.x + 1] = b;
    }
}

// the maximum of v over the workgroup; every thread gets it (sh: 4 values)
__device__ __forceinline__ i64 fai_block_max(i64 v, i64* sh)
{
    v = lane63_i64(wave_incl_max_i64(v));
    if (lane_id() == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    i64 m = sh[0];
    for (int k = 1; k < 4; k++) m = sh[k] > m ? sh[k] : m;
    __syncthreads();
    return m;
}

template <bool WRITE> __global__ __launch_bounds__(256) void k_fai_events(FaiArgs A)
{
    __shared__ i64 sh[8], red[4];
    const int t = blockIdx.x, w = threadIdx.x >> 6;
    // the last two line breaks in front of this tile: the largest, then the largest below it (FAI_NONE is below every position)
    i64 v = FAI_NONE;
    for (int k = threadIdx.x; k < t; k += 256) { const i64 a = A.top[2 * (i64)k]; v = a > v ? a : v; }
    const i64 in1 = fai_block_max(v, red);
    v = FAI_NONE;
    for (int k = threadIdx.x; k < 2 * t; k += 256) { const i64 a = A.top[k]; if (a < in1 && a > v) v = a; }
    const i64 in2 = fai_block_max(v, red);
    // the wavefronts' own pairs, so that each knows what runs into it
    const i64 t0 = (i64)t * FAI_TILE, lo = t0 + (i64)w * FAI_WAVE_BYTES, hi = lo + FAI_WAVE_BYTES < A.n ? lo + FAI_WAVE_BYTES : A.n;
    i64 m1, m2;
    fai_wave_top2(A.d, lo, hi, m1, m2);
    if (lane_id() == 0) { sh[2 * w] = m1; sh[2 * w + 1] = m2; }
    __syncthreads();
    i64 q1 = in1, q2 = in2;                                        // the running pair: wave-uniform
    fai_fold(sh, w, q1, q2);
    i64 at = 0;                                                    // where this wavefront's rows go
    if (WRITE) {
        at = block_prefix_of(A.cnt, 4 * t, red);
        for (int k = 0; k < w; k++) at += A.cnt[4 * (i64)t + k];
    }
    int rows = 0;
    for (i64 p0 = lo; p0 < hi; p0 += WAVE) {
        const i64 e = p0 + lane_id();
        const bool nl = e < hi && A.d[e] == '\n';
        const u64 mask = __ballot(nl ? 1 : 0);
        if (!mask) continue;
        bool hit = false;
        FaiRow r{0, 0, 0};
        if (nl) {
            // the line breaks before this lane's: bits of the ballot below it, then the running pair
            const u64 below = mask & lanemask_lt();
            i64 a = q1, b = q2;
            fai_push(below, p0, a, b);
            hit = fai_event(A.d, A.base, A.c, e, a, b, &r);
        }
        const u64 hits = __ballot(hit ? 1 : 0);
        if (WRITE && hit) {
            const i64 k = at + rows + __popcll(hits & lanemask_lt());
            if (k < A.row_cap) A.rows[k] = r;
        }
        rows += __popcll(hits);
        fai_push(mask, p0, q1, q2);
    }
    if (!WRITE && lane_id() == 0) A.cnt[4 * (i64)t + w] = rows;
    if (WRITE && t == (int)gridDim.x - 1) {
        // the last tile: the rows of the whole window, and the line in progress behind its last line break
        __syncthreads();
        if (lane_id() == 63) red[w] = at + rows;                   // (the last wavefront's is the total)
        __syncthreads();
        if (threadIdx.x == 0) {
            i64 a = in1, b = in2;
            fai_fold(sh, 4, a, b);
            A.out->n_rows = red[3];
            A.out->tail = fai_tail(A.d, A.n, A.base, A.c, a);
        }
    }
}

// ------------------------------------------------------------------------------------ the coordinate sort
// The kernels of the coordinate sort of a BAM file; sort_core.h holds the rules.  The whole
// inflated stream lies in one arena in device memory; `starts` names its records.
//   k_sort_keys      one thread per record: key and length out of the record's bytes; the first refused record by a 64-bit atomicMin of
//                    ordinal << 3 | why; the adjacent inversions (key[i] < key[i - 1]); the OR of all keys, from which the host names the
//                    8-bit digits the radix passes have to look at
//   (the permutation comes from sort.hip.h's k_sort_* passes over the key column: there is no second radix sort)
//   k_sort_dst_tiles / k_sort_dst_scan   the lengths gathered through the permutation and their exclusive 64-bit prefix sums: dst
//   k_sort_gather    the hot path: every byte of the file passes through it once.  Output-driven: a wavefront owns SORT_GATHER_TILE
//                    bytes of the slice buffer and every lane writes aligned 16-byte pieces of it, so the time does not depend on the mix
//                    of record lengths - 40-byte records and a 300 KB read cost the same per byte, and no wavefront copies a long record
//                    alone.  Two wave-uniform binary searches over dst bracket the records that feed the tile; a lane searches only that
//                    bracket (at most tile / 36 + 2 entries, hot in the cache).  A piece that lies inside one record is read as five
//                    aligned dwords funnel-shifted to the source's alignment; a piece that crosses a record boundary, the header's end or
//                    the stream's end is assembled byte by byte by sort_core.h's piece rule.  All offsets are 64-bit.
// Bounds.  The host has checked the chain: every start lies in [first record, arena end), whole records only, so key fields (36
// bytes) and every source byte are inside the arena; the aligned dword reads reach at most 3 bytes in front of a source (never in
// front of the arena: the header precedes the first record) and 7 bytes behind it (the arena has 32 bytes of slack).  A lane stores
// only inside [0, round_up(len, 16)) of the slice buffer, which has that room.

// Bytes of the slice buffer per wavefront: 64 lanes x 16 bytes x 4 rounds.  Chosen, not measured: 4 rounds amortise the two bracket
// searches (2 x ~25 dependent loads for 16 M records) over 256 stores, and a 16 MiB slice still gives 4096 wavefronts, 4 per SIMD.
constexpr int SORT_GATHER_TILE = 4096;

struct SortKeyArgs {
    const uint8_t* arena; i64 arena_bytes; const i64* starts; i64 n; int n_ref;
    u64* key; i64* len;
    u64* verdict;                   // [0] min of ordinal << 3 | why (SORT_NONE: none), [1] inversions, [2] OR of the keys
};

__global__ __launch_bounds__(256) void k_sort_keys(SortKeyArgs A)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const bool in = i < A.n;
    u64 key = 0;
    int inv = 0;
    if (in) {
        const SortFields f = sort_fields(A.arena + A.starts[i]);
        int why = sort_refuse(f, A.n_ref);
        if (f.len < 36 || f.len > A.arena_bytes - A.starts[i]) why = SORT_WHY_CHAIN;   // (not the bytes the reader stepped over: nothing may be gathered)
        if (why) atomicMin((unsigned long long*)&A.verdict[0], (unsigned long long)((u64)i << 3 | (u64)why));
        else key = sort_key(f, A.n_ref);
        A.key[i] = key; A.len[i] = f.len;
        if (i > 0) {                                              // (the neighbour's key again from its bytes: no second launch, no barrier)
            const SortFields g = sort_fields(A.arena + A.starts[i - 1]);
            inv = !why && !sort_refuse(g, A.n_ref) && key < sort_key(g, A.n_ref);
        }
    }
    const u64 votes = __ballot(inv);
    u64 any = key;
    for (int m = 1; m < 64; m <<= 1) any |= (u64)shfl_xor_i64((i64)any, m);
    if (lane_id() == 0) {
        if (votes) atomicAdd((unsigned long long*)&A.verdict[1], (unsigned long long)__popcll(votes));
        if (any) atomicOr((unsigned long long*)&A.verdict[2], (unsigned long long)any);
    }
}

// dst: per tile of 1024 sorted records the sum of their lengths, then every tile its carry and its own exclusive scan
constexpr int SORT_DST_TILE = 1024;
struct SortDstArgs { const i64* len; const int* perm; i64 n; i64* dst; i64* tile_sum; };      // perm NULL: the identity; dst: n + 1

__global__ __launch_bounds__(256) void k_sort_dst_tiles(SortDstArgs A)
{
    __shared__ i64 sh[4];
    const i64 base = (i64)blockIdx.x * SORT_DST_TILE;
    i64 s = 0;
    for (int k = threadIdx.x; k < SORT_DST_TILE; k += 256) {
        const i64 r = base + k;
        if (r < A.n) s += A.len[A.perm ? A.perm[r] : r];
    }
    s = wave_sum_i64(s);
    if (lane_id() == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) A.tile_sum[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ __launch_bounds__(256) void k_sort_dst_scan(SortDstArgs A)
{
    __shared__ i64 sh[4], ws[4];
    __shared__ i64 carry;
    const i64 before = block_prefix_of64(A.tile_sum, (int)blockIdx.x, sh);
    if (threadIdx.x == 0) carry = before;
    __syncthreads();
    const i64 base = (i64)blockIdx.x * SORT_DST_TILE;
    for (int b0 = 0; b0 < SORT_DST_TILE; b0 += 256) {
        const i64 r = base + b0 + threadIdx.x;
        const i64 v = r < A.n ? A.len[A.perm ? A.perm[r] : r] : 0;
        const i64 inc = wave_incl_scan_i64(v);
        if (lane_id() == 63) ws[threadIdx.x >> 6] = inc;
        __syncthreads();
        i64 off = carry;
        for (int q = 0; q < (int)(threadIdx.x >> 6); q++) off += ws[q];
        off += inc - v;
        if (r < A.n) A.dst[r] = off;
        if (r == A.n - 1) A.dst[A.n] = off + v;
        __syncthreads();
        if (threadIdx.x == 255) carry = off + v;
        __syncthreads();
    }
}

struct SortGatherArgs {
    const uint8_t* arena; const uint8_t* hdr; i64 H;
    const i64* starts; const int* perm; const i64* dst; i64 n;     // perm NULL: the identity; dst: n + 1 (unused when n == 0)
    i64 s0, len;                    // the slice: bytes [s0, s0 + len) of the sorted stream; s0 is a multiple of 16
    uint8_t* out;                   // the slice buffer: round_up(len, 16) bytes are written, 16-byte aligned
};

// 16 bytes at any alignment as five aligned dwords, funnel-shifted
__device__ __forceinline__ uint4 sort_ld16(const uint8_t* p)
{
    const uintptr_t a = (uintptr_t)p;
    const uint32_t* w = (const uint32_t*)(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(a & 3) * 8;
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
    return make_uint4(__builtin_amdgcn_alignbit(w1, w0, sh), __builtin_amdgcn_alignbit(w2, w1, sh), __builtin_amdgcn_alignbit(w3, w2, sh), __builtin_amdgcn_alignbit(w4, w3, sh));
}

__global__ __launch_bounds__(256) void k_sort_gather(SortGatherArgs A)
{
    const i64 tile = ((i64)blockIdx.x * 256 + threadIdx.x) >> 6;
    const i64 t0 = tile * SORT_GATHER_TILE;                       // in the slice
    if (t0 >= A.len) return;
    const i64 t1 = t0 + SORT_GATHER_TILE < A.len ? t0 + SORT_GATHER_TILE : A.len;
    const i64 end = A.s0 + A.len;                                 // of the slice, in the stream
    // the records that feed the tile: [lo, hi] (wave-uniform)
    i64 lo = 0, hi = 0;
    if (A.n > 0 && A.s0 + t1 > A.H) {
        const i64 ra = A.s0 + t0 > A.H ? A.s0 + t0 - A.H : 0;
        lo = sort_first_record(A.dst, 0, A.n - 1, ra);
        hi = sort_first_record(A.dst, lo, A.n - 1, A.s0 + t1 - 1 - A.H);
    }
    for (int q = 0; q < SORT_GATHER_TILE / (64 * 16); q++) {
        const i64 at = t0 + ((i64)q * 64 + lane_id()) * 16;      // in the slice
        if (at >= t1) break;
        const i64 o = A.s0 + at;                                  // in the stream
        uint4 v;
        if (o + 16 <= A.H) v = *(const uint4*)(A.hdr + o);
        else {
            i64 r = o >= A.H ? sort_first_record(A.dst, lo, hi, o - A.H) : 0;
            if (o >= A.H && o + 16 <= end && o + 16 - A.H <= A.dst[r + 1])
                v = sort_ld16(A.arena + A.starts[A.perm ? A.perm[r] : r] + (o - A.H - A.dst[r]));
            else {                                                // a boundary inside the piece: sort_tile_fill's rule, byte by byte
                uint32_t w[4] = {0, 0, 0, 0};
                i64 src = -1, left = 0;                           // the running source, and its bytes still inside the record
                for (int j = 0; j < 16; j++) {
                    const i64 p = o + j;
                    if (p >= end) break;                          // (behind the stream's end the piece stays zero)
                    uint32_t b;
                    if (p < A.H) b = A.hdr[p];
                    else {
                        if (left == 0) {
                            if (src >= 0) r++;
                            const i64 in_rec = p - A.H - A.dst[r];
                            src = A.starts[A.perm ? A.perm[r] : r] + in_rec;
                            left = A.dst[r + 1] - A.dst[r] - in_rec;
                        }
                        b = A.arena[src]; src++; left--;
                    }
                    w[j >> 2] |= b << (8 * (j & 3));
                }
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        *(uint4*)(A.out + at) = v;
    }
}

// ------------------------------------------------------------------------------------ SAM text to BAM records
// A window of SAM text - whole alignment lines, the last byte a line break - lies in device memory; sam_core.h holds the rules.
//   k_sam_marks<false / true>   the line breaks and the tabs of the window as two sorted position lists.  A workgroup takes SAM_TILE bytes,
//                    a wavefront a quarter, a lane 16 bytes a step (one aligned load); a lane's marks are a 16-bit mask, their places the
//                    wave scan of the popcounts over the wavefront's running count; the count pass leaves the wavefronts' counts, the write
//                    pass sums those in front (block_prefix_of).  A 4 MB line and a 200-byte line cost the same per byte.
//   k_sam_plan       one wavefront per line: its fields are cuts of the tab list (two wave-uniform searches), every number is read a digit
//                    per lane (sam_wave_int / sam_wave_float), the CIGAR and the tags lanes striding with ballots.  Out: the row (what the
//                    write pass needs again) and the record's size - or the mark "host item": every line outside the strict grammar,
//                    which means every line that may be refused, and B:f arrays.  The host runs sam_core.h's serial rule on those lines.
//   (one exclusive 64-bit scan of the sizes - k_sort_dst_tiles / k_sort_dst_scan, the sort's - gives dst)
//   k_sam_small      one wavefront per record: block_size, the fixed fields, the name, the CIGAR words (or the placeholder and the
//                    CG:B:I tag) and the tags; a float outside the fast path leaves a patch row
//   k_sam_bulk       the hot path, output-driven as k_sort_gather is: a wavefront owns SAM_BULK_TILE bytes of the stream buffer, brackets
//                    the records that feed it with two searches over dst, and every lane writes aligned 16-byte pieces of SEQ (32 text
//                    bytes -> 16) and QUAL (16 -> 16, a byte below 33 reported by atomicMin of the line's ordinal); a piece that holds a
//                    region's edge is written byte by byte, and only the bytes that belong to SEQ or QUAL
//   k_sam_items / k_sam_item_len / k_sam_patch   the host's records copied into their places, their sizes, the patched floats
// Bounds.  Text is read at [0, n) only, except sort_ld16's aligned dwords (at most 3 bytes in front of a SEQ or QUAL field, which
// never begins a window, and 19 behind its last piece: the text buffer has 64 bytes of slack).  A record's bytes are written inside
// [base + dst[r], base + dst[r + 1]) only: plan and write pass call the same functions on the same text, so sizes and bytes agree.
constexpr int SAM_TILE = 32768, SAM_WAVE_BYTES = SAM_TILE / 4;
// Bytes of the stream buffer per wavefront of k_sam_bulk: 64 lanes x 16 bytes x 4 rounds, k_sort_gather's choice for its reasons
// (two bracket searches amortised over 256 stores); chosen, not measured.
constexpr int SAM_BULK_TILE = 4096;
constexpr int SAM_ROW_HOST = 1, SAM_ROW_CG = 2, SAM_ROW_QSTAR = 4;

struct SamRow { i64 seq_text, qual_text, ref_len; int n_ops, l_seq, seq_out, flags; i64 tab0; int ntab, pad; };
struct SamPatch { i64 out_off, text_off; int len, pad; };

struct SamArgs {
    const uint8_t* t; i64 n;        // the window: n > 0 bytes, the last a line break
    int* cnt_nl; int* cnt_tab;      // 4 per tile of SAM_TILE bytes
    i64* nl; i64* tab; i64 n_lines, n_tabs;
    SamNames names;
    SamRow* rows; i64* len; const i64* dst;
    int* items; int* counters;      // the host items' lines (n_lines entries); [0] their count, [1] the patch rows, [2] the CG records
    u64* verdict;                   // the lowest line ordinal (in the window) with a QUAL byte below 33; ~0: none
    uint8_t* out; i64 base, total;  // the stream buffer; the records begin at base and take total bytes
    SamPatch* patches; i64 patch_cap;
};

template <bool WRITE> __global__ __launch_bounds__(256) void k_sam_marks(SamArgs A)
{
    __shared__ i64 red[4];
    const int t = blockIdx.x, w = threadIdx.x >> 6;
    const i64 lo = (i64)t * SAM_TILE + (i64)w * SAM_WAVE_BYTES, hi = lo + SAM_WAVE_BYTES < A.n ? lo + SAM_WAVE_BYTES : A.n;
    i64 at_nl = 0, at_tab = 0;
    if (WRITE) {
        at_nl = block_prefix_of(A.cnt_nl, 4 * t, red);
        at_tab = block_prefix_of(A.cnt_tab, 4 * t, red);
        for (int k = 0; k < w; k++) { at_nl += A.cnt_nl[4 * (i64)t + k]; at_tab += A.cnt_tab[4 * (i64)t + k]; }
    }
    for (i64 p0 = lo; p0 < hi; p0 += 64 * 16) {
        const i64 p = p0 + (i64)lane_id() * 16;
        uint32_t m_nl = 0, m_tab = 0;
        if (p < hi) {
            const uint4 v = *(const uint4*)(A.t + p);           // (aligned: the buffer and every p are multiples of 16; the buffer has slack)
            const uint32_t x[4] = {v.x, v.y, v.z, v.w};
            for (int j = 0; j < 16; j++) {
                const uint32_t c = (x[j >> 2] >> (8 * (j & 3))) & 255u;
                if (p + j < hi) { m_nl |= (uint32_t)(c == '\n') << j; m_tab |= (uint32_t)(c == '\t') << j; }
            }
        }
        const int c_nl = __popc(m_nl), c_tab = __popc(m_tab);
        const int i_nl = wave_incl_scan_i32(c_nl), i_tab = wave_incl_scan_i32(c_tab);
        if (WRITE) {
            i64 k = at_nl + i_nl - c_nl;
            for (uint32_t m = m_nl; m; m &= m - 1, k++) if (k < A.n_lines) A.nl[k] = p + __builtin_ctz(m);
            k = at_tab + i_tab - c_tab;
            for (uint32_t m = m_tab; m; m &= m - 1, k++) if (k < A.n_tabs) A.tab[k] = p + __builtin_ctz(m);
        }
        at_nl += __builtin_amdgcn_readlane(i_nl, 63); at_tab += __builtin_amdgcn_readlane(i_tab, 63);
    }
    if (!WRITE && lane_id() == 0) { A.cnt_nl[4 * (i64)t + w] = (int)at_nl; A.cnt_tab[4 * (i64)t + w] = (int)at_tab; }
}

__device__ __forceinline__ u64 sam_bits(int a, int b) { return a >= b ? 0ull : (b >= 64 ? ~0ull : (1ull << b) - 1ull) & ~((1ull << a) - 1ull); }     // lanes [a, b), a < 64

// the first index in [0, n) with a[index] >= x (n: none); wave-uniform
__device__ __forceinline__ i64 sam_lower(const i64* a, i64 n, i64 x)
{
    i64 lo = 0, hi = n;
    while (lo < hi) {
        const i64 m = lo + (hi - lo) / 2;
        if (a[m] < x) lo = m + 1; else hi = m;
    }
    return lo;
}

// sam_int_text, a digit per lane
__device__ __forceinline__ bool sam_wave_int(const uint8_t* t, i64 b, i64 e, bool sign_ok, i64* v)
{
    const i64 n = e - b;
    if (n < 1 || n > 19) return false;
    const uint32_t c0 = t[b];
    const bool sg = sign_ok && (c0 == '-' || c0 == '+');
    const int s = sg ? 1 : 0, nd = (int)n - s, l = lane_id();
    if (nd < 1 || nd > 18) return false;
    const uint32_t c = l < n ? t[b + l] : 0u;
    const bool isd = l >= s && l < n && sam_digit(c);
    if (__popcll(__ballot(isd ? 1 : 0)) != nd) return false;
    const i64 sum = wave_sum_i64(isd ? (i64)((u64)(c - '0') * sam_pow10((int)n - 1 - l)) : 0);
    *v = sg && c0 == '-' ? -sum : sum;
    return true;
}

// sam_float_text, a byte per lane: 0 not the grammar, 1 slow, 2 fast
__device__ __forceinline__ int sam_wave_float(const uint8_t* t, i64 b, i64 e, float* f)
{
    const i64 n64 = e - b;
    if (n64 < 1 || n64 > SAM_NUM_MAX) return 0;
    const int n = (int)n64, l = lane_id();
    const bool in = l < n;
    const uint32_t c = in ? t[b + l] : 0u;
    const u64 dig = __ballot(in && sam_digit(c) ? 1 : 0), dot = __ballot(in && c == '.' ? 1 : 0), ee = __ballot(in && (c == 'e' || c == 'E') ? 1 : 0);
    const u64 sg = __ballot(in && (c == '-' || c == '+') ? 1 : 0), minus = __ballot(in && c == '-' ? 1 : 0);
    const int s = (int)(sg & 1ull);
    if (__popcll(ee) > 1) return 0;
    const int E = ee ? __builtin_ctzll(ee) : n;
    if (E <= s) return 0;
    const u64 mm = sam_bits(s, E), md = dig & mm, mdot = dot & mm;
    if (__popcll(mdot) > 1 || (md | mdot) != mm) return 0;
    int nfrac = 0;
    if (mdot) {
        const int d = __builtin_ctzll(mdot);
        if (d == s || d == E - 1) return 0;
        nfrac = E - 1 - d;
    }
    SamFloat q{(int)(minus & 1ull), 0, 0, 0, 0};
    i64 expv = 0;
    bool eneg = false;
    if (ee) {
        int x0 = E + 1;
        if (x0 < n && ((sg >> x0) & 1ull)) { eneg = (minus >> x0) & 1ull; x0++; }
        if (x0 >= n) return 0;
        const u64 xm = sam_bits(x0, n);
        if ((dig & xm) != xm) return 0;
        q.nexp = n - x0;
        if (q.nexp <= 4) expv = wave_sum_i64(((xm >> l) & 1ull) ? (i64)((u64)(c - '0') * sam_pow10(n - 1 - l)) : 0);
    }
    const u64 nz = __ballot(((md >> l) & 1ull) && c != '0' ? 1 : 0);
    if (nz) {
        const u64 sig = md & ~((1ull << __builtin_ctzll(nz)) - 1ull);
        q.nsig = __popcll(sig);
        if (q.nsig <= 15) {
            const int r = __popcll(sig & (l >= 63 ? 0ull : ~0ull << (l + 1)));
            q.mant = (u64)wave_sum_i64(((sig >> l) & 1ull) ? (i64)((u64)(c - '0') * sam_pow10(r)) : 0);
        }
    }
    q.exp10 = (eneg ? -expv : expv) - nfrac;
    return sam_float_class(q, f);
}

// sam_name_find, 64 bytes a comparison step
__device__ __forceinline__ int sam_wave_name(const SamNames& N, const uint8_t* t, i64 b, i64 e)
{
    const i64 qn = e - b;
    int lo = 0, hi = N.n - 1;
    while (lo <= hi) {
        const int m = lo + (hi - lo) / 2;
        const i64 nb = N.off[m], nn = N.off[m + 1] - nb, mn = qn < nn ? qn : nn;
        int cmp = 0;
        for (i64 k = 0; k < mn && !cmp; k += 64) {
            const i64 j = k + lane_id();
            const int a = j < mn ? t[b + j] : 0, c = j < mn ? N.blob[nb + j] : 0;
            const u64 diff = __ballot(a != c ? 1 : 0);
            if (diff) {
                const int d = __builtin_ctzll(diff);
                cmp = __shfl(a, d) < __shfl(c, d) ? -1 : 1;
            }
        }
        if (!cmp) cmp = qn < nn ? -1 : qn > nn ? 1 : 0;
        if (cmp == 0) return N.id[m];
        if (cmp < 0) hi = m - 1; else lo = m + 1;
    }
    return -2;
}

// the CIGAR text t[b, e), lanes striding: its operations counted (and, out != NULL, written as BAM words at out, which has their room),
// the reference bases they span.  false: not a CIGAR.  A lane that stands on an operation reads its own length backwards, 10 bytes at most
__device__ __forceinline__ bool sam_wave_cigar(const uint8_t* t, i64 b, i64 e, uint8_t* out, i64* n_ops, i64* ref_len)
{
    *n_ops = 0; *ref_len = 0;
    if (e - b == 1 && t[b] == '*') return true;
    if (e <= b || sam_digit(t[e - 1])) return false;
    i64 ops = 0, rl = 0;
    bool ok = true;
    for (i64 p0 = b; p0 < e; p0 += 64) {
        const i64 i = p0 + lane_id();
        const bool in = i < e;
        const uint32_t c = in ? t[i] : (uint32_t)'0';
        const int op = sam_digit(c) ? -1 : sam_cigar_op(c);
        bool bad = in && !sam_digit(c) && op < 0, is_op = in && op >= 0;
        i64 len = 0;
        if (is_op) {
            int nd = 0;
            i64 mul = 1;
            for (i64 j = i - 1; j >= b && nd < 10 && sam_digit(t[j]); j--, nd++, mul *= 10) len += (i64)(t[j] - '0') * mul;
            if (nd == 0 || nd > 9 || len >= (1ll << 28)) { bad = true; is_op = false; }
        }
        const u64 m = __ballot(is_op ? 1 : 0);
        if (out && is_op) sam_put32(out + 4 * (ops + __popcll(m & lanemask_lt())), (uint32_t)len << 4 | (uint32_t)op);
        rl += wave_sum_i64(is_op && sam_op_on_ref(op) ? len : 0);
        ops += __popcll(m);
        if (__ballot(bad ? 1 : 0)) ok = false;
    }
    *n_ops = ops; *ref_len = rl;
    return ok;
}

// One optional field t[b, e) as a BAM tag: its bytes, or -1 when the text is outside the device's grammar (the line becomes a host item).
// WRITE: the tag is written at o (offset o_abs of the stream buffer); a slow float leaves zeros and a patch row
template <bool WRITE> __device__ __forceinline__ i64 sam_wave_tag(const SamArgs& A, i64 b, i64 e, uint8_t* o, i64 o_abs)
{
    const uint8_t* t = A.t;
    const i64 n = e - b;
    const int l = lane_id();
    if (n < 5 || t[b + 2] != ':' || t[b + 4] != ':') return -1;
    const uint32_t type = t[b + 3];
    const i64 vb = b + 5, vn = n - 5;
    if (WRITE && l < 2) o[l] = t[b + l];
    switch (type) {
    case 'A':
        if (vn != 1) return -1;
        if (WRITE && l == 0) { o[2] = 'A'; o[3] = t[vb]; }
        return 4;
    case 'i': {
        i64 x;
        int w;
        if (!sam_wave_int(t, vb, e, true, &x)) return -1;
        const int ty = sam_int_type(x, &w);
        if (!ty) return -1;
        if (WRITE) { if (l == 0) o[2] = (uint8_t)ty; if (l < w) o[3 + l] = (uint8_t)((u64)x >> (8 * l)); }
        return 3 + w;
    }
    case 'f': {
        float f = 0;
        const int cls = sam_wave_float(t, vb, e, &f);
        if (cls == 0) return -1;
        if (WRITE) {
            if (l == 0) o[2] = 'f';
            if (l < 4) o[3 + l] = cls == 2 ? (uint8_t)(__float_as_uint(f) >> (8 * l)) : (uint8_t)0;
            if (cls == 1 && l == 0) {
                const int k = atomicAdd(&A.counters[1], 1);
                if (k < A.patch_cap) A.patches[k] = SamPatch{o_abs + 3, vb, (int)vn, 0};
            }
        }
        return 7;
    }
    case 'H': {
        if (vn & 1) return -1;
        bool bad = false;
        for (i64 k = l; k < vn; k += 64) {
            const uint32_t c = t[vb + k];
            if (!(sam_digit(c) || (c >= 'A' && c <= 'F') || (c >= 'a' && c <= 'f'))) bad = true;
        }
        if (__ballot(bad ? 1 : 0)) return -1;
    }
    /* fall through */
    case 'Z':
        if (WRITE) {
            if (l == 0) { o[2] = (uint8_t)type; o[3 + vn] = 0; }
            for (i64 k = l; k < vn; k += 64) o[3 + k] = t[vb + k];
        }
        return 4 + vn;
    case 'B': {
        if (vn < 1 || (vn > 1 && t[vb + 1] != ',')) return -1;
        const uint32_t sub = t[vb];
        i64 lo, hi;
        const int w = sam_sub_width(sub, &lo, &hi);
        if (!w || sub == 'f') return -1;                          // (B:f: a host item)
        i64 count = 0;
        bool ok = true;
        for (i64 p0 = vb + 1; p0 < e; p0 += 64) {
            const i64 i = p0 + l;
            const bool comma = i < e && t[i] == ',';
            const u64 m = __ballot(comma ? 1 : 0);
            bool bad = false;
            if (comma) {                                          // the element behind this lane's comma: 19 bytes at most
                i64 q = i + 1, x = 0;
                while (q < e && t[q] != ',' && q - i <= 20) q++;
                if ((q < e && t[q] != ',') || !sam_int_text(t + i + 1, q - i - 1, true, &x) || x < lo || x > hi) bad = true;
                else if (WRITE) {
                    uint8_t* d = o + 8 + (count + __popcll(m & lanemask_lt())) * w;
                    for (int k = 0; k < w; k++) d[k] = (uint8_t)((u64)x >> (8 * k));
                }
            }
            if (__ballot(bad ? 1 : 0)) ok = false;
            count += __popcll(m);
        }
        if (!ok || count > 0xffffffffll) return -1;
        if (WRITE && l == 0) { o[2] = 'B'; o[3] = (uint8_t)sub; sam_put32(o + 4, (uint32_t)count); }
        return 8 + count * w;
    }
    default: return -1;
    }
}

// the line's first 11 fields as cuts of the tab list: false when it has fewer.  fb / fe: their begins and ends
__device__ __forceinline__ bool sam_fields(const SamArgs& A, i64 line, i64& beg, i64& end, i64& tab0, i64& ntab, i64* fb, i64* fe)
{
    beg = line == 0 ? 0 : A.nl[line - 1] + 1; end = A.nl[line];
    tab0 = sam_lower(A.tab, A.n_tabs, beg);
    ntab = sam_lower(A.tab, A.n_tabs, end) - tab0;
    if (ntab < 10) return false;
    for (int k = 0; k < 11; k++) {
        fb[k] = k == 0 ? beg : A.tab[tab0 + k - 1] + 1;
        fe[k] = k < ntab ? A.tab[tab0 + k] : end;
    }
    return true;
}

__global__ __launch_bounds__(256) void k_sam_plan(SamArgs A)
{
    const i64 line = ((i64)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (line >= A.n_lines) return;
    const uint8_t* t = A.t;
    SamRow R{0, 0, 0, 0, 0, 0, SAM_ROW_HOST, 0, 0, 0};
    i64 size = 0;
    i64 beg, end, tab0, ntab, fb[11], fe[11];
    do {                                                          // (left by `break` where the line becomes a host item; wave-uniform)
        if (!sam_fields(A, line, beg, end, tab0, ntab, fb, fe)) break;
        if (t[end - 1] == '\r' || t[beg] == '@') break;
        bool empty = false;
        for (int k = 0; k < 11; k++) empty |= fe[k] <= fb[k];
        if (empty) break;
        const i64 l_name = fe[0] - fb[0];
        if (l_name > SAM_QNAME_MAX) break;
        i64 v;
        if (!sam_wave_int(t, fb[1], fe[1], false, &v) || v > 65535) break;
        if (!sam_wave_int(t, fb[3], fe[3], false, &v) || v > 2147483647) break;
        if (!sam_wave_int(t, fb[4], fe[4], false, &v) || v > 255) break;
        if (!sam_wave_int(t, fb[7], fe[7], false, &v) || v > 2147483647) break;
        if (!sam_wave_int(t, fb[8], fe[8], true, &v) || v > 2147483647 || v < -2147483647) break;
        if (!(fe[2] - fb[2] == 1 && t[fb[2]] == '*') && sam_wave_name(A.names, t, fb[2], fe[2]) == -2) break;
        if (!(fe[6] - fb[6] == 1 && (t[fb[6]] == '*' || t[fb[6]] == '=')) && sam_wave_name(A.names, t, fb[6], fe[6]) == -2) break;
        i64 n_ops, ref_len;
        if (!sam_wave_cigar(t, fb[5], fe[5], nullptr, &n_ops, &ref_len)) break;
        const i64 l_seq = fe[9] - fb[9] == 1 && t[fb[9]] == '*' ? 0 : fe[9] - fb[9];
        const bool qstar = fe[10] - fb[10] == 1 && t[fb[10]] == '*';
        if (!qstar && fe[10] - fb[10] != l_seq) break;
        i64 tags = 0;
        bool ok = true;
        for (i64 k = 11; k <= ntab && ok; k++) {
            const i64 b = A.tab[tab0 + k - 1] + 1, e = k < ntab ? A.tab[tab0 + k] : end;
            const i64 sz = sam_wave_tag<false>(A, b, e, nullptr, 0);
            if (sz < 0) ok = false; else tags += sz;
        }
        if (!ok) break;
        const bool cg = n_ops > SAM_MAX_OPS;
        const i64 seq_out = 36 + l_name + 1 + 4 * (cg ? 2 : n_ops);
        size = seq_out + (l_seq + 1) / 2 + l_seq + tags + (cg ? 8 + 4 * n_ops : 0);
        if (size - 4 > 2147483647ll) { size = 0; break; }
        R = SamRow{fb[9], fb[10], ref_len, (int)n_ops, (int)l_seq, (int)seq_out, (cg ? SAM_ROW_CG : 0) | (qstar ? SAM_ROW_QSTAR : 0), tab0, (int)ntab, 0};
    } while (false);
    if (lane_id() == 0) {
        A.rows[line] = R; A.len[line] = size;
        if (R.flags & SAM_ROW_HOST) A.items[atomicAdd(&A.counters[0], 1)] = (int)line;
        if (R.flags & SAM_ROW_CG) atomicAdd(&A.counters[2], 1);
    }
}

__global__ __launch_bounds__(256) void k_sam_small(SamArgs A)
{
    const i64 line = ((i64)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (line >= A.n_lines) return;
    const SamRow R = A.rows[line];
    if (R.flags & SAM_ROW_HOST) return;
    const uint8_t* t = A.t;
    const int l = lane_id();
    i64 beg, end, tab0, ntab, fb[11], fe[11];
    if (!sam_fields(A, line, beg, end, tab0, ntab, fb, fe)) return;
    const i64 o_rec = A.base + A.dst[line], size = A.dst[line + 1] - A.dst[line];
    uint8_t* rec = A.out + o_rec;
    SamFixed x{};
    i64 v = 0;
    sam_wave_int(t, fb[1], fe[1], false, &v); x.flag = (uint32_t)v;
    sam_wave_int(t, fb[3], fe[3], false, &v); x.pos = (int32_t)(v - 1);
    sam_wave_int(t, fb[4], fe[4], false, &v); x.mapq = (uint32_t)v;
    sam_wave_int(t, fb[7], fe[7], false, &v); x.next_pos = (int32_t)(v - 1);
    sam_wave_int(t, fb[8], fe[8], true, &v); x.tlen = (int32_t)v;
    x.refid = fe[2] - fb[2] == 1 && t[fb[2]] == '*' ? -1 : sam_wave_name(A.names, t, fb[2], fe[2]);
    if (fe[6] - fb[6] == 1 && t[fb[6]] == '*') x.next_refid = -1;
    else if (fe[6] - fb[6] == 1 && t[fb[6]] == '=') x.next_refid = x.refid;
    else x.next_refid = sam_wave_name(A.names, t, fb[6], fe[6]);
    const i64 l_name = fe[0] - fb[0];
    const bool cg = R.flags & SAM_ROW_CG;
    x.l_name = (uint32_t)l_name + 1; x.n_cigar = cg ? 2u : (uint32_t)R.n_ops; x.l_seq = (uint32_t)R.l_seq; x.bin = sam_bin(x.pos, R.ref_len);
    if (l == 0) { sam_put32(rec, (uint32_t)(size - 4)); sam_put_fixed(rec + 4, x); rec[36 + l_name] = 0; }
    for (i64 k = l; k < l_name; k += 64) rec[36 + k] = t[fb[0] + k];
    uint8_t* oc = rec + 36 + l_name + 1;
    i64 n_ops, ref_len;
    if (cg) { if (l == 0) { sam_put32(oc, (uint32_t)R.l_seq << 4 | 4u); sam_put32(oc + 4, (uint32_t)R.ref_len << 4 | 3u); } }
    else sam_wave_cigar(t, fb[5], fe[5], oc, &n_ops, &ref_len);
    i64 ot = R.seq_out + (R.l_seq + 1) / 2 + R.l_seq;             // in the record
    for (i64 k = 11; k <= ntab; k++) {
        const i64 b = A.tab[tab0 + k - 1] + 1, e = k < ntab ? A.tab[tab0 + k] : end;
        const i64 sz = sam_wave_tag<true>(A, b, e, rec + ot, o_rec + ot);
        if (sz < 0) return;                                       // (the plan took this tag: never)
        ot += sz;
    }
    if (cg) {
        if (l == 0) { rec[ot] = 'C'; rec[ot + 1] = 'G'; rec[ot + 2] = 'B'; rec[ot + 3] = 'I'; sam_put32(rec + ot + 4, (uint32_t)R.n_ops); }
        sam_wave_cigar(t, fb[5], fe[5], rec + ot + 8, &n_ops, &ref_len);
    }
}

// the byte at in_rec of record r when it belongs to SEQ or QUAL (true), read from the text
__device__ __forceinline__ bool sam_bulk_byte(const SamArgs& A, const SamRow& R, i64 r, i64 in_rec, uint32_t* b)
{
    const i64 s0 = R.seq_out, s1 = s0 + (R.l_seq + 1) / 2, q1 = s1 + R.l_seq;
    if ((R.flags & SAM_ROW_HOST) || in_rec < s0 || in_rec >= q1) return false;
    if (in_rec < s1) {
        const i64 k = 2 * (in_rec - s0);
        *b = sam_base_code(A.t[R.seq_text + k]) << 4 | (k + 1 < R.l_seq ? sam_base_code(A.t[R.seq_text + k + 1]) : 0u);
        return true;
    }
    if (R.flags & SAM_ROW_QSTAR) { *b = 0xffu; return true; }
    const uint32_t c = A.t[R.qual_text + (in_rec - s1)];
    if (c < 33) atomicMin((unsigned long long*)A.verdict, (unsigned long long)r);
    *b = (c - 33) & 255u;
    return true;
}

__global__ __launch_bounds__(256) void k_sam_bulk(SamArgs A)
{
    const i64 tile = ((i64)blockIdx.x * 256 + threadIdx.x) >> 6;
    const i64 end = A.base + A.total;
    i64 t0 = tile * SAM_BULK_TILE, t1 = t0 + SAM_BULK_TILE < end ? t0 + SAM_BULK_TILE : end;
    if (t0 >= end || t1 <= A.base || A.n_lines <= 0) return;
    const i64 n = A.n_lines;
    const i64 lo = sort_first_record(A.dst, 0, n - 1, (t0 > A.base ? t0 : A.base) - A.base), hi = sort_first_record(A.dst, lo, n - 1, t1 - 1 - A.base);
    for (int q = 0; q < SAM_BULK_TILE / (64 * 16); q++) {
        const i64 o = t0 + ((i64)q * 64 + lane_id()) * 16;       // in the stream buffer
        if (o >= t1) break;
        if (o + 16 <= A.base) continue;
        i64 r = sort_first_record(A.dst, lo, hi, (o > A.base ? o : A.base) - A.base);
        const SamRow R = A.rows[r];
        const i64 in_rec = o - A.base - A.dst[r];
        const i64 s0 = R.seq_out, s1 = s0 + (R.l_seq + 1) / 2, q1 = s1 + R.l_seq;
        if (o >= A.base && !(R.flags & SAM_ROW_HOST) && in_rec >= s0 && in_rec + 16 <= s0 + R.l_seq / 2) {
            // 16 bytes of SEQ out of 32 bases
            const uint8_t* src = A.t + R.seq_text + 2 * (in_rec - s0);
            const uint4 a = sort_ld16(src), b = sort_ld16(src + 16);
            const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            uint32_t v[4];
            for (int k = 0; k < 4; k++) {
                const uint32_t x = w[2 * k], y = w[2 * k + 1];
                v[k] = (sam_base_code(x & 255u) << 4 | sam_base_code((x >> 8) & 255u)) | (sam_base_code((x >> 16) & 255u) << 4 | sam_base_code(x >> 24)) << 8
                     | (sam_base_code(y & 255u) << 4 | sam_base_code((y >> 8) & 255u)) << 16 | (sam_base_code((y >> 16) & 255u) << 4 | sam_base_code(y >> 24)) << 24;
            }
            *(uint4*)(A.out + o) = make_uint4(v[0], v[1], v[2], v[3]);
        } else if (o >= A.base && !(R.flags & SAM_ROW_HOST) && in_rec >= s1 && in_rec + 16 <= q1) {
            uint4 a = make_uint4(~0u, ~0u, ~0u, ~0u);
            if (!(R.flags & SAM_ROW_QSTAR)) {
                a = sort_ld16(A.t + R.qual_text + (in_rec - s1));
                uint32_t w[4] = {a.x, a.y, a.z, a.w};
                bool bad = false;
                for (int k = 0; k < 4; k++) {
                    uint32_t y = 0;
                    for (int j = 0; j < 32; j += 8) { const uint32_t c = (w[k] >> j) & 255u; bad |= c < 33; y |= ((c - 33) & 255u) << j; }
                    w[k] = y;
                }
                if (bad) atomicMin((unsigned long long*)A.verdict, (unsigned long long)r);
                a = make_uint4(w[0], w[1], w[2], w[3]);
            }
            *(uint4*)(A.out + o) = a;
        } else {
            // a piece with an edge in it: byte by byte, and only the bytes of SEQ and QUAL
            SamRow Q = R;
            for (int j = 0; j < 16; j++) {
                const i64 p = o + j;
                if (p < A.base) continue;
                if (p >= end) break;
                while (p - A.base >= A.dst[r + 1]) { r++; Q = A.rows[r]; }
                uint32_t b;
                if (sam_bulk_byte(A, Q, r, p - A.base - A.dst[r], &b)) A.out[p] = (uint8_t)b;
            }
        }
    }
}

struct SamItemArgs { const int* line; const i64* src_off; const i64* size; i64 n; const uint8_t* src; i64* len; const i64* dst; uint8_t* out; i64 base; };

__global__ __launch_bounds__(256) void k_sam_item_len(SamItemArgs A)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < A.n) A.len[A.line[i]] = A.size[i];
}

// one wavefront per host item: its record into its place
__global__ __launch_bounds__(256) void k_sam_items(SamItemArgs A)
{
    const i64 i = ((i64)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (i >= A.n) return;
    const uint8_t* s = A.src + A.src_off[i];
    uint8_t* d = A.out + A.base + A.dst[A.line[i]];
    for (i64 k = lane_id(); k < A.size[i]; k += 64) d[k] = s[k];
}

__global__ __launch_bounds__(256) void k_sam_patch(const SamPatch* P, const uint32_t* bits, i64 n, uint8_t* out)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) sam_put32(out + P[i].out_off, bits[i]);
}

}  // namespace csv
