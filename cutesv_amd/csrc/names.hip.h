// names.hip.h — read names ranked on the GPU: the context's name pool (a blob plus offsets) -> for every
// name its index in sorted(set(names)), the names compared as unsigned bytes, a prefix before its extensions.
//
// The reference's order contract ends in the read NAME (main script :764-802: ties on (pos, len) order by name; :958-969:
// equal rows are rows with equal names), so the rebuild's read-id column must be an integer whose order is the names' string
// order.  Here that integer is made where the rows already are:
//   k_name_pack    the blob -> a column-major matrix of big-endian 64-bit words, W = ceil(max_len / 8) columns, zero padded
//                  (integer order of the word tuple == byte order of the name; NUL cannot occur inside a BAM name, so the
//                  padding orders a prefix first), and per column the OR of word ^ word of name 0: the bytes that vary
//   sort           the permutation sort of sort.hip.h (k_sort_hist / k_sort_rowsum / k_sort_rowscan / k_sort_scatter) over the
//                  word columns, one pass per byte position that differs anywhere - the host plans them from the W OR words,
//                  so the number of passes is bounded by the varying positions (<= 255) and never depends on the data inside
//                  a pass
//   k_name_count / k_name_apply   in sorted order: flag = the name differs from its predecessor (word by word, early exit,
//                  bounded by W), prefix sum, rank[perm[i]] = sum - 1, first[rank] = perm[i] where flagged (the sort is
//                  stable: that is the smallest index holding the name)
//   k_name_gather  names by index into one blob (csv_name_pool_get)
// Every loop is bounded by W, n or the tile; every byte read lies inside the arena (the host checked the ranges on append).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wave.hip.h"

namespace csv {

constexpr int NAME_MAX_LEN = 255;
constexpr int NAME_MAX_WORDS = 32;
constexpr int NAME_TILE = 2048;              // names per workgroup in the pack and rank kernels

// word w of name i: bytes [8 w, 8 w + 8) of the name, the first byte most significant, zero behind the name's end
__device__ __forceinline__ u64 name_word(const uint8_t* blob, const i64* off, i64 i, int w)
{
    const i64 b = off[i] + 8 * (i64)w, e = off[i + 1];
    u64 v = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) v = (v << 8) | (u64)(b + k < e ? blob[b + k] : 0);
    return v;
}

// grid (tiles of NAME_TILE names, W): words[w * n + i], vary[w] |= word ^ word of name 0
__global__ __launch_bounds__(256) void k_name_pack(const uint8_t* blob, const i64* off, i64 n, u64* words, unsigned long long* vary)
{
    __shared__ u64 sh[4];
    const int w = blockIdx.y;
    const u64 w0 = name_word(blob, off, 0, w);
    u64 acc = 0;
    const i64 base = (i64)blockIdx.x * NAME_TILE;
    for (int r = 0; r < NAME_TILE / 256; r++) {
        const i64 i = base + r * 256 + threadIdx.x;
        if (i < n) {
            const u64 v = name_word(blob, off, i, w);
            words[(i64)w * n + i] = v;
            acc |= v ^ w0;
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)(acc & 0xffffffffull), d), hi = __shfl_xor((unsigned)(acc >> 32), d);
        acc |= ((u64)hi << 32) | lo;
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 v = sh[0] | sh[1] | sh[2] | sh[3];
        if (v) atomicOr(&vary[w], (unsigned long long)v);
    }
}

struct NameRank {
    i64 n;
    int W;
    const u64* words;       // [W][n]
    const int* perm;        // sorted order (nullptr: identity - no byte varies, every name is equal)
    uint8_t* flag;          // per sorted position: the name differs from its predecessor (position 0: 1)
    int* partial;           // per tile of NAME_TILE positions: flags set
    int* rank;              // per name
    int* first;             // per rank: smallest index holding the name
    int* n_distinct;
};

__device__ __forceinline__ int name_head(const NameRank& R, i64 i)
{
    if (i >= R.n) return 0;
    if (i == 0) return 1;
    const i64 p = R.perm ? R.perm[i] : i, q = R.perm ? R.perm[i - 1] : i - 1;
    for (int w = 0; w < R.W; w++)
        if (R.words[(i64)w * R.n + p] != R.words[(i64)w * R.n + q]) return 1;
    return 0;
}

__global__ __launch_bounds__(256) void k_name_count(NameRank R)
{
    const i64 base = (i64)blockIdx.x * NAME_TILE + (threadIdx.x >> 6) * 512;
    int cnt = 0;
    for (int r = 0; r < 8; r++) {
        const i64 i = base + r * 64 + (threadIdx.x & 63);
        const int h = name_head(R, i);
        if (i < R.n) R.flag[i] = (uint8_t)h;
        cnt += __popcll(__ballot(h));
    }
    __shared__ int s[4];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) R.partial[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}

__global__ __launch_bounds__(256) void k_name_apply(NameRank R)
{
    __shared__ i64 sh[4];
    __shared__ int s[4];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const i64 base = (i64)blockIdx.x * NAME_TILE + wv * 512;
    u64 masks[8]; int cnt = 0;
    for (int r = 0; r < 8; r++) {
        const i64 i = base + r * 64 + lane;
        masks[r] = __ballot(i < R.n && R.flag[i]);
        cnt += __popcll(masks[r]);
    }
    int run = (int)block_prefix_of(R.partial, blockIdx.x, sh);        // heads in front of this tile
    if (lane == 0) s[wv] = cnt;
    __syncthreads();
    for (int k = 0; k < wv; k++) run += s[k];
    for (int r = 0; r < 8; r++) {
        const i64 i = base + r * 64 + lane;
        const u64 m = masks[r];
        if (i < R.n) {
            const int rk = run + __popcll(m & ((2ull << lane) - 1ull)) - 1;     // heads up to and including position i, minus one
            const int p = R.perm ? R.perm[i] : (int)i;
            R.rank[p] = rk;
            if ((m >> lane) & 1) R.first[rk] = p;
        }
        run += __popcll(m);
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 255) *R.n_distinct = run;
}

// one wavefront per requested name: out[out_off[k] ..] = the bytes of name index[k] (at most 255: four steps of 64 lanes)
__global__ __launch_bounds__(256) void k_name_gather(const uint8_t* blob, const i64* off, const int* index, const i64* out_off, i64 n_get, uint8_t* out)
{
    const i64 k = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n_get) return;
    const int lane = threadIdx.x & 63;
    const i64 b = off[index[k]], len = off[index[k] + 1] - b, o = out_off[k];
    for (int s = 0; s < (NAME_MAX_LEN + 63) / 64; s++) {
        const int j = s * 64 + lane;
        if (j < len) out[o + j] = blob[b + j];
    }
}

}  // namespace csv
