// scan.hip.h — the "count -> offsets" step of the extraction stages: one exclusive scan over three int columns at once.
//
// Contract: the counts in cnt[i].x / .y / .z (i < n) become their exclusive prefix sums in place and cnt[i].w is zeroed;
// totals[0..2] receive the three sums, written by the last tile; tile_sum is work space of three i64 per tile of SCAN_TILE
// entries (scan_tile_bytes(n) bytes).  Offsets are stored as int: a batch whose sums leave 31 bits is rejected by the host.
// Two launches of scan_tiles(n) workgroups: k_scan_tiles (the tiles' sums), k_scan_offsets (every tile recomputes its carry
// from the tile sums - a few thousand values - and scans its own entries).  scan_counts() launches both; n > 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "wave.hip.h"

namespace csv {

struct ScanArgs {
    i64 n;
    int4* cnt;
    i64* tile_sum;                  // 3 per tile of SCAN_TILE entries
    i64* totals;                    // 3
};

constexpr int SCAN_TILE = 1024;     // entries per scan tile

// per tile of SCAN_TILE entries: sums of the three counts
__global__ __launch_bounds__(256) void k_scan_tiles(ScanArgs A)
{
    const i64 base = (i64)blockIdx.x * SCAN_TILE;
    i64 s0 = 0, s1 = 0, s2 = 0;
    for (int i = threadIdx.x; i < SCAN_TILE; i += 256) {
        const i64 r = base + i;
        if (r < A.n) { const int4 c = A.cnt[r]; s0 += c.x; s1 += c.y; s2 += c.z; }
    }
    s0 = wave_sum_i64(s0); s1 = wave_sum_i64(s1); s2 = wave_sum_i64(s2);
    __shared__ i64 sh[12];
    if (lane_id() == 0) { sh[(threadIdx.x >> 6)] = s0; sh[4 + (threadIdx.x >> 6)] = s1; sh[8 + (threadIdx.x >> 6)] = s2; }
    __syncthreads();
    if (threadIdx.x < 3) A.tile_sum[(i64)blockIdx.x * 3 + threadIdx.x] = sh[4 * threadIdx.x] + sh[4 * threadIdx.x + 1] + sh[4 * threadIdx.x + 2] + sh[4 * threadIdx.x + 3];
}

// counts -> exclusive offsets, in place (the tile's prefix is recomputed from the tile sums: a few thousand values)
__global__ __launch_bounds__(256) void k_scan_offsets(ScanArgs A)
{
    __shared__ i64 sh[12], carry[3];
    __shared__ i64 ws[3][4];
    i64 p[3] = {0, 0, 0};
    for (int t = threadIdx.x; t < (int)blockIdx.x; t += 256)
        for (int k = 0; k < 3; k++) p[k] += A.tile_sum[(i64)t * 3 + k];
    for (int k = 0; k < 3; k++) { p[k] = wave_sum_i64(p[k]); if (lane_id() == 0) sh[4 * k + (threadIdx.x >> 6)] = p[k]; }
    __syncthreads();
    if (threadIdx.x < 3) carry[threadIdx.x] = sh[4 * threadIdx.x] + sh[4 * threadIdx.x + 1] + sh[4 * threadIdx.x + 2] + sh[4 * threadIdx.x + 3];
    __syncthreads();
    const i64 base = (i64)blockIdx.x * SCAN_TILE;
    for (int b0 = 0; b0 < SCAN_TILE; b0 += 256) {
        const i64 r = base + b0 + threadIdx.x;
        int4 c = make_int4(0, 0, 0, 0);
        if (r < A.n) c = A.cnt[r];
        const i64 v[3] = {c.x, c.y, c.z};
        i64 inc[3];
        for (int k = 0; k < 3; k++) { inc[k] = wave_incl_scan_i64(v[k]); if (lane_id() == 63) ws[k][threadIdx.x >> 6] = inc[k]; }
        __syncthreads();
        i64 off[3];
        for (int k = 0; k < 3; k++) {
            off[k] = carry[k];
            for (int q = 0; q < (int)(threadIdx.x >> 6); q++) off[k] += ws[k][q];
            off[k] += inc[k] - v[k];
        }
        // offsets can exceed 32 bits only beyond 2^31 signatures per batch: rejected by the host
        if (r < A.n) A.cnt[r] = make_int4((int)off[0], (int)off[1], (int)off[2], 0);
        __syncthreads();
        if (threadIdx.x == 255) for (int k = 0; k < 3; k++) carry[k] = off[k] + v[k];
        __syncthreads();
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) for (int k = 0; k < 3; k++) A.totals[k] = carry[k];
}

// host side: tiles of n entries, the bytes of their sums, and the two launches
inline int scan_tiles(i64 n) { return (int)((n + SCAN_TILE - 1) / SCAN_TILE); }
inline size_t scan_tile_bytes(i64 n) { return (size_t)scan_tiles(n) * 3 * sizeof(i64); }
inline void scan_counts(hipStream_t st, const ScanArgs& A)
{
    const int ntile = scan_tiles(A.n);
    hipLaunchKernelGGL(k_scan_tiles, dim3(ntile), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_scan_offsets, dim3(ntile), dim3(256), 0, st, A);
}

}  // namespace csv
