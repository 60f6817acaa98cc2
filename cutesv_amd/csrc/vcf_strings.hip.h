// vcf_strings.hip.h — the two strings a VCF record takes from the pools, gathered where the pools are:
//   ALT of an INS call   bases(pool row src_row[seq_pick])[: SVLEN]                      (cuteSV_resolveINDEL.py:402)
//   RNAMES of a call     ",".join(name(first[read_id[s]]) for s in the call's supports)   (cuteSV_genotype.py:263-458)
// Both read the sorted columns a kept pool rebuild left on the device (src_row, read_id, aux) and produce the CSR blobs
// csv_vcf_in takes (ins_alt / ins_alt_off, rnames / rnames_off).
//
//   k_alt_plan      one thread per pick: length = min(aux, clip), status (the row has no sequence)
//   k_join_plan     one thread per support: length of its name + 1 (the comma, or the slot the last name of a call leaves
//                   unused), status (a rank outside the name pool's)
//   scan            the lengths go through the scan of scan.hip.h (k_scan_tiles / k_scan_offsets), as seqs.hip.h's do
//   k_vs_offsets    the scanned lengths as the caller's 64-bit offsets;  k_join_call_off  the same per call: byte position
//                   of support j of call c = P[j] - (non-empty calls in front of c), P = the exclusive scan of len + 1
//   k_alt_copy      one wavefront per pick, lanes stride over the output: single bytes up to the first aligned word and behind
//                   the last one, one 32-bit store per lane and step in between (seq_copy's layout in seqs.hip.h)
//   k_join_copy     one wavefront per support: a name is at most 255 bytes, four steps of 64 lanes (k_name_gather), then the comma
// Every kernel walks its entries with a grid-stride loop (the host caps the grid).  Every byte read lies inside the row's
// [seq_off, seq_off + aux) resp. inside the name's [off[i], off[i + 1]); picks and supports were range-checked on the host.
// The same columns and pools also give the lines of cuteSV's <TYPE>.sigs files (k_sigs_plan / k_sigs_write, at the end of this file).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wave.hip.h"
#include "names.hip.h"
#include "vcf_core.h"

namespace csv {

enum { VS_ERR_NO_SEQ = 1, VS_ERR_RANK = 2 };

struct VsRows { const int* src_row; const int* read_id; const int* aux; };      // the kept rebuild's sorted columns

// cnt[k] = {bytes of entry k, 0, 0, 0}
__global__ __launch_bounds__(256) void k_alt_plan(VsRows R, const i64* seq_off, const int* pick, const int* clip, i64 n, int4* cnt, int* err)
{
    for (i64 k = (i64)blockIdx.x * 256 + threadIdx.x; k < n; k += (i64)gridDim.x * 256) {
        const int row = pick[k];
        int len = 0;
        if (seq_off[R.src_row[row]] < 0) atomicOr(err, VS_ERR_NO_SEQ);
        else {
            const int aux = R.aux[row];
            len = aux < clip[k] ? aux : clip[k];
            len = len > 0 ? len : 0;
        }
        cnt[k] = make_int4(len, 0, 0, 0);
    }
}

__global__ __launch_bounds__(256) void k_vs_offsets(const int4* cnt, const i64* tot, i64 n, i64* off)
{
    for (i64 k = (i64)blockIdx.x * 256 + threadIdx.x; k <= n; k += (i64)gridDim.x * 256) off[k] = k < n ? (i64)cnt[k].x : tot[0];
}

// L bytes from src to dst by one wavefront
__device__ __forceinline__ void vs_copy(const uint8_t* src, i64 L, uint8_t* dst, int lane)
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

// one wavefront per pick (only launched when the plan found nothing wrong); cnt holds the exclusive offsets
__global__ __launch_bounds__(256) void k_alt_copy(VsRows R, const uint8_t* blob, const i64* seq_off, const int* pick, const int* clip, i64 n, const int4* cnt, uint8_t* out)
{
    const int lane = threadIdx.x & 63;
    for (i64 k = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); k < n; k += (i64)gridDim.x * 4) {
        const int row = pick[k], aux = R.aux[row];
        const int len = aux < clip[k] ? aux : clip[k];
        if (len > 0) vs_copy(blob + seq_off[R.src_row[row]], len, out + cnt[k].x, lane);
    }
}

// ------------------------------------------------------------------------------------ RNAMES
struct VsNames { const uint8_t* blob; const i64* off; const int* first; i64 n_distinct; };

__global__ __launch_bounds__(256) void k_join_plan(VsRows R, VsNames N, const int* sup, i64 n_sup, int4* cnt, int* err)
{
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j < n_sup; j += (i64)gridDim.x * 256) {
        const int rk = R.read_id[sup[j]];
        int len = 0;
        if (rk < 0 || rk >= N.n_distinct) atomicOr(err, VS_ERR_RANK);
        else {
            const int i = N.first[rk];
            len = (int)(N.off[i + 1] - N.off[i]);
        }
        cnt[j] = make_int4(len + 1, 0, 0, 0);
    }
}

// out_off[c] = first byte of call c, c in [0, n_calls]; before[c] = non-empty calls in front of call c
__global__ __launch_bounds__(256) void k_join_call_off(const int4* cnt, const i64* tot, const i64* support_off, const i64* before, i64 n_calls, i64 n_sup, i64* out_off)
{
    for (i64 c = (i64)blockIdx.x * 256 + threadIdx.x; c <= n_calls; c += (i64)gridDim.x * 256) {
        const i64 s = support_off[c];
        out_off[c] = (s < n_sup ? (i64)cnt[s].x : tot[0]) - before[c];
    }
}

// one wavefront per support; adj[j] = non-empty calls in front of its call << 1 | the support is the last of its call
__global__ __launch_bounds__(256) void k_join_copy(VsRows R, VsNames N, const int* sup, const int* adj, i64 n_sup, const int4* cnt, uint8_t* out)
{
    const int lane = threadIdx.x & 63;
    for (i64 j = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); j < n_sup; j += (i64)gridDim.x * 4) {
        const int i = N.first[R.read_id[sup[j]]];
        const i64 b = N.off[i], len = N.off[i + 1] - b, o = (i64)cnt[j].x - (adj[j] >> 1);
        for (int s = 0; s < (NAME_MAX_LEN + 63) / 64; s++) {
            const int x = s * 64 + lane;
            if (x < len) out[o + x] = N.blob[b + x];
        }
        if (lane == 0 && !(adj[j] & 1)) out[o + len] = (uint8_t)',';
    }
}


// ------------------------------------------------------------------------------------ the text signature files
// The legacy text signature files of cuteSV's --write_old_sigs (main script :763-808), made where the rebuilt
// signatures are: rows [row_begin, row_begin + n) of a kept pool rebuild become one text line each
//   DEL / DUP   TYPE \t chr \t a \t b \t read \n                       INS   TYPE \t chr \t a \t b \t read \t bases \n
//   INV         TYPE \t chr \t strand \t a \t b \t read \n             TRA   TYPE \t chr \t A|B|C|D \t a \t chr2 \t b \t read \n
// with segment s = type TYPES[s / n_chrom] on chromosome s % n_chrom (rebuild._segments), read = name(first[read_id]), bases = the
// sequence-pool entry of the row's pool row (aux bytes), strand = strands[aux], TRA: type = aux & 7, chr2 = chromosome aux >> 3.
//
//   k_sigs_plan     one thread per row: the line's length into cnt[k].x, and a status bit for what the entry refuses
//   scan            the lengths go through the scan of scan.hip.h (k_scan_tiles / k_scan_offsets)
//   k_sigs_write    one wavefront per row: lanes write the fixed pieces, one lane per decimal digit, the name in four steps of 64
//                   lanes (k_join_copy), the chromosome names in steps of 64, the bases with vs_copy's aligned words
// Both kernels walk their rows with a grid-stride loop (the host caps the grid).  Every byte read lies inside the row's own name
// [off[i], off[i + 1]), its own sequence [seq_off, seq_off + aux) or a chromosome name of the caller's table; the write kernel is
// launched only when the plan found nothing wrong, so it repeats none of the plan's checks.

enum { ST_ERR_COORD = 1, ST_ERR_RANK = 2, ST_ERR_NO_SEQ = 4, ST_ERR_TRA = 8, ST_ERR_STRAND = 16, ST_ERR_SEG = 32 };
enum { ST_DEL = 0, ST_INS = 1, ST_INV = 2, ST_DUP = 3, ST_TRA = 4 };          // columns.TYPES
constexpr i64 ST_COORD_END = 1ll << 42;                                        // coordinates live in [0, 2^42)
constexpr int ST_STRAND_MAX = 15;

struct StRows { const int* seg; const i64* a; const i64* b; const int* rid; const int* aux; const int* src; };
struct StTables {
    const uint8_t* chrom; const int* chrom_off; int n_chrom;                   // chromosome names in name-rank order: blob + n_chrom + 1 offsets
    const uint8_t* seq_blob; const i64* seq_off;                               // the sequence pool by pool row (seq_off NULL: the context holds none)
    uint8_t strand[2][ST_STRAND_MAX + 1]; int strand_len[2];
};

__device__ __forceinline__ u64 st_pow10(int k)
{
    static const u64 P[14] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull, 1000000000ull, 10000000000ull,
                              100000000000ull, 1000000000000ull, 10000000000000ull};
    return P[k];
}
// decimal digits of v in [0, 2^42): 1 .. 13
__device__ __forceinline__ int st_digits(i64 v)
{
    int d = 1;
    while (d < 13 && (u64)v >= st_pow10(d)) d++;
    return d;
}

__global__ __launch_bounds__(256) void k_sigs_plan(StRows R, VsNames N, StTables T, i64 row0, i64 n, int4* cnt, int* err)
{
    for (i64 k = (i64)blockIdx.x * 256 + threadIdx.x; k < n; k += (i64)gridDim.x * 256) {
        const i64 r = row0 + k;
        const int seg = R.seg[r], aux = R.aux[r], rk = R.rid[r];
        const i64 a = R.a[r], b = R.b[r];
        int bad = 0, len = 0;
        if (seg < 0 || seg >= 5 * T.n_chrom) bad |= ST_ERR_SEG;
        if (a < 0 || a >= ST_COORD_END || b < 0 || b >= ST_COORD_END) bad |= ST_ERR_COORD;
        if (rk < 0 || rk >= N.n_distinct) bad |= ST_ERR_RANK;
        if (!bad) {
            const int type = seg / T.n_chrom, ch = seg - type * T.n_chrom;
            const int i = N.first[rk];
            // "TYP\t" chr "\t" a "\t" b "\t" read "\n"
            len = 4 + (T.chrom_off[ch + 1] - T.chrom_off[ch]) + 1 + st_digits(a) + 1 + st_digits(b) + 1 + (int)(N.off[i + 1] - N.off[i]) + 1;
            if (type == ST_INS) {
                if (!T.seq_off || aux < 0 || T.seq_off[R.src[r]] < 0) bad |= ST_ERR_NO_SEQ;
                else len += 1 + aux;
            } else if (type == ST_INV) {
                if (aux < 0 || aux > 1) bad |= ST_ERR_STRAND;
                else len += T.strand_len[aux] + 1;
            } else if (type == ST_TRA) {
                const int c2 = aux >> 3;
                if (aux < 0 || (aux & 7) > 3 || c2 >= T.n_chrom) bad |= ST_ERR_TRA;
                else len += 2 + (T.chrom_off[c2 + 1] - T.chrom_off[c2]) + 1;
            }
        }
        if (bad) atomicOr(err, bad);
        cnt[k] = make_int4(bad ? 0 : len, 0, 0, 0);
    }
}

// the pieces of a line, each written by the whole wavefront at o; every one returns the position behind it
__device__ __forceinline__ i64 st_put_byte(uint8_t* out, i64 o, int lane, uint8_t ch)
{
    if (lane == 0) out[o] = ch;
    return o + 1;
}
__device__ __forceinline__ i64 st_put_bytes(uint8_t* out, i64 o, int lane, const uint8_t* src, int len)
{
    for (int x = lane; x < len; x += 64) out[o + x] = src[x];
    return o + len;
}
// v in [0, 2^42) in decimal, one lane per digit (the quotient by a power of ten in 32 bits where the value has them)
__device__ __forceinline__ i64 st_put_number(uint8_t* out, i64 o, int lane, i64 v)
{
    const int nd = st_digits(v);
    if (lane < nd) {
        const u64 p = st_pow10(nd - 1 - lane);
        const unsigned q = (u64)v < (1ull << 32) ? (unsigned)v / (unsigned)p : (unsigned)(((u64)v / p) % 10ull);
        out[o + lane] = (uint8_t)('0' + q % 10u);
    }
    return o + nd;
}

// one wavefront per row (only launched when the plan found nothing wrong); cnt holds the exclusive offsets
__global__ __launch_bounds__(256) void k_sigs_write(StRows R, VsNames N, StTables T, i64 row0, i64 n, const int4* cnt, uint8_t* out)
{
    const int lane = threadIdx.x & 63;
    for (i64 k = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); k < n; k += (i64)gridDim.x * 4) {
        const i64 r = row0 + k;
        const int seg = R.seg[r], aux = R.aux[r];
        const int type = seg / T.n_chrom, ch = seg - type * T.n_chrom;
        i64 o = (i64)cnt[k].x;
        // "DEL\t" .. "TRA\t" as little-endian words
        const unsigned tag = type == ST_DEL ? 0x094c4544u : type == ST_INS ? 0x09534e49u : type == ST_INV ? 0x09564e49u : type == ST_DUP ? 0x09505544u : 0x09415254u;
        if (lane < 4) out[o + lane] = (uint8_t)(tag >> (8 * lane));
        o += 4;
        o = st_put_bytes(out, o, lane, T.chrom + T.chrom_off[ch], T.chrom_off[ch + 1] - T.chrom_off[ch]);
        o = st_put_byte(out, o, lane, '\t');
        if (type == ST_INV) {
            o = st_put_bytes(out, o, lane, T.strand[aux], T.strand_len[aux]);
            o = st_put_byte(out, o, lane, '\t');
        } else if (type == ST_TRA) {
            if (lane == 0) { out[o] = (uint8_t)('A' + (aux & 7)); out[o + 1] = '\t'; }
            o += 2;
        }
        o = st_put_number(out, o, lane, R.a[r]);
        o = st_put_byte(out, o, lane, '\t');
        if (type == ST_TRA) {
            const int c2 = aux >> 3;
            o = st_put_bytes(out, o, lane, T.chrom + T.chrom_off[c2], T.chrom_off[c2 + 1] - T.chrom_off[c2]);
            o = st_put_byte(out, o, lane, '\t');
        }
        o = st_put_number(out, o, lane, R.b[r]);
        o = st_put_byte(out, o, lane, '\t');
        const int i = N.first[R.rid[r]];
        const i64 nb = N.off[i];
        const int nlen = (int)(N.off[i + 1] - nb);
        for (int s = 0; s < (NAME_MAX_LEN + 63) / 64; s++) {
            const int x = s * 64 + lane;
            if (x < nlen) out[o + x] = N.blob[nb + x];
        }
        o += nlen;
        if (type == ST_INS) {
            o = st_put_byte(out, o, lane, '\t');
            if (aux > 0) vs_copy(T.seq_blob + T.seq_off[R.src[r]], aux, out + o, lane);
            o += aux;
        }
        st_put_byte(out, o, lane, '\n');
    }
}

// ------------------------------------------------------------------------------------ the VCF records
// The record text itself: the calls of a batch, as the flat view of vcf_core.h, become the lines of the VCF body
// in emission order (`order`: slot q writes call order[q]).  The record of a call is vcf_core.h's vcf_record, the one source the host
// form runs with one lane.
//   k_vcf_plan      one thread per slot: the emitted id (-1: a size filter drops the call) as the six counts {INS, DEL, BND} / {DUP, INV,
//                   emitted}.  A record's length depends on the digits of its SVID, and the SVID is the count of emitted records of its
//                   type in front of it: so the counts go through the scan of scan.hip.h first ...
//   k_vcf_len       ... then one thread per slot computes the record's length (vcf_record_len: a sink that only counts), and the lengths
//                   are scanned
//   k_vcf_write     one wavefront per slot: every piece of the record is stored by the 64 lanes, neighbouring lanes neighbouring bytes - the
//                   REF bases through the IUPAC table, a number as one digit per lane - looping over long pieces (a DEL's REF may be 100
//                   kb); lane 0 writes the record's row {chromosome, beg, end, offset of the record in the text}
// All three walk their slots with a grid-stride loop (the host caps the grid).  Bounds: the view was judged on the host before anything
// is launched (vcf_host_prepare): every index lies inside its table, every call's bytes inside its blob.  A record is written to
// out[prefix + off .. prefix + off + len) with off, len from the same vcf_record that writes it, inside the prefix + total bytes the host
// reserved; its row to rows[4 r .. 4 r + 4), r = the emitted records in front of it < their total.
struct VeArgs { VcfView V; const i64* order; i64 n; i64 sv_ins, sv_del, sv_bnd, sv_dup, sv_inv; i64 prefix; };

__global__ __launch_bounds__(256) void k_vcf_plan(VeArgs A, int4* cnt_a, int4* cnt_b)
{
    for (i64 q = (i64)blockIdx.x * 256 + threadIdx.x; q < A.n; q += (i64)gridDim.x * 256) {
        const int id = vcf_call_id(A.V, A.order[q]);
        cnt_a[q] = make_int4(id == VCF_ID_INS, id == VCF_ID_DEL, id == VCF_ID_BND, 0);
        cnt_b[q] = make_int4(id == VCF_ID_DUP, id == VCF_ID_INV, id >= 0, 0);
    }
}

// the SVID of slot q's record: the caller's counter of its type plus the records of that type in front of it (cnt_a / cnt_b scanned)
__device__ __forceinline__ i64 ve_svid(const VeArgs& A, const int4* cnt_a, const int4* cnt_b, i64 q, int id)
{
    const int4 a = cnt_a[q], b = cnt_b[q];
    return id == VCF_ID_INS ? A.sv_ins + a.x : id == VCF_ID_DEL ? A.sv_del + a.y : id == VCF_ID_BND ? A.sv_bnd + a.z : id == VCF_ID_DUP ? A.sv_dup + b.x : A.sv_inv + b.y;
}

__global__ __launch_bounds__(256) void k_vcf_len(VeArgs A, const int4* cnt_a, const int4* cnt_b, int4* cnt_c)
{
    for (i64 q = (i64)blockIdx.x * 256 + threadIdx.x; q < A.n; q += (i64)gridDim.x * 256) {
        const i64 c = A.order[q];
        const int id = vcf_call_id(A.V, c);
        cnt_c[q] = make_int4(id < 0 ? 0 : (int)vcf_record_len(A.V, c, id, ve_svid(A, cnt_a, cnt_b, q, id)), 0, 0, 0);
    }
}

// one wavefront per slot (launched only when the text fits 31 bits); cnt_a / cnt_b / cnt_c hold the exclusive prefixes
__global__ __launch_bounds__(256) void k_vcf_write(VeArgs A, const int4* cnt_a, const int4* cnt_b, const int4* cnt_c, uint8_t* out, i64* rows)
{
    const int lane = threadIdx.x & 63;
    for (i64 q = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); q < A.n; q += (i64)gridDim.x * 4) {
        const i64 c = A.order[q];
        const int id = vcf_call_id(A.V, c);
        if (id < 0) continue;
        const i64 o = A.prefix + (i64)cnt_c[q].x;
        VcfRow row;
        vcf_record_write(A.V, c, id, ve_svid(A, cnt_a, cnt_b, q, id), out, o, lane, 64, &row);
        if (lane < 4) rows[4 * (i64)cnt_b[q].z + lane] = lane == 0 ? (i64)row.chrom : lane == 1 ? row.beg : lane == 2 ? row.end : o;
    }
}

}  // namespace csv
