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
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wave.hip.h"
#include "names.hip.h"

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

}  // namespace csv
