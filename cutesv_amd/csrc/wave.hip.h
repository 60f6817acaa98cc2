// wave.hip.h — the wavefront and workgroup primitives every device header of libcutesv_hip.so builds on (gfx950 / CDNA4 only,
// wave64): the 64-bit typedefs, lane helpers, 64-bit shuffles and v_readlane, the DPP scans and reductions, and the sum of an
// array over a workgroup of 256 threads.  No kernel lives here; a device header that uses any of this includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define CSV_LIKELY(x) __builtin_expect(!!(x), 1)
#define CSV_UNLIKELY(x) __builtin_expect(!!(x), 0)

namespace csv {

typedef unsigned long long u64;
typedef long long i64;

constexpr int WAVE = 64;

// ------------------------------------------------------------------------------------ small helpers
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ u64 lanemask_lt() { return (1ull << lane_id()) - 1ull; }

__device__ __forceinline__ i64 shfl_i64(i64 v, int src)
{
    int lo = __shfl((int)(v & 0xffffffffll), src), hi = __shfl((int)(v >> 32), src);
    return ((i64)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ i64 shfl_up_i64(i64 v, int d)
{
    int lo = __shfl_up((int)(v & 0xffffffffll), d), hi = __shfl_up((int)(v >> 32), d);
    return ((i64)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ i64 shfl_xor_i64(i64 v, int m)
{
    int lo = __shfl_xor((int)(v & 0xffffffffll), m), hi = __shfl_xor((int)(v >> 32), m);
    return ((i64)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ double shfl_xor_f64(double v, int m) { return __longlong_as_double(shfl_xor_i64(__double_as_longlong(v), m)); }
// value of lane l (wave-uniform index): a wave-uniform (SGPR) result
__device__ __forceinline__ i64 readlane_i64(i64 v, int l)
{
    const int lo = __builtin_amdgcn_readlane((int)(v & 0xffffffffll), l);
    const int hi = __builtin_amdgcn_readlane((int)(v >> 32), l);
    return ((i64)hi << 32) | (unsigned)lo;
}
// ---- wave64 scans / reductions on DPP (data-parallel primitives: row_shr inside rows of 16 lanes, then
// row_bcast:15 / row_bcast:31 across rows): 6 VALU moves per 32-bit word, no LDS round trips, no waitcnt.
template <int CTRL, int RM> __device__ __forceinline__ int dpp_i32(int old, int v)
{
    return __builtin_amdgcn_update_dpp(old, v, CTRL, RM, 0xf, false);       // lanes without a source keep `old`
}
template <int CTRL, int RM> __device__ __forceinline__ i64 dpp_i64(i64 old, i64 v)
{
    const int lo = dpp_i32<CTRL, RM>((int)(old & 0xffffffffll), (int)(v & 0xffffffffll));
    const int hi = dpp_i32<CTRL, RM>((int)(old >> 32), (int)(v >> 32));
    return ((i64)hi << 32) | (unsigned)lo;
}
// One step of a 64-bit DPP scan: v + (v moved by the pattern; lanes without a source and rows outside the mask add nothing),
// as the carry pair the hardware has for it - v_add_co_u32_dpp / v_addc_co_u32_dpp.  Written through dpp_i64 the compiler
// builds the moved value as two 64-bit numbers (lo | 0 and 0 | hi), each from a zeroed register and a v_mov_b32_dpp, and adds
// them with two v_lshl_add_u64: seven vector instructions a step where two do - and these kernels run at 60 - 86 % of the vector
// ALUs' issue rate (profiles/r04_cfg3_insts.txt), so the count is the time.  s_nop 4: a DPP read needs two wait states after
// the VALU write of its source and FIVE after a VALU write of EXEC (v_cmpx), and the hazard recogniser does not look inside an
// asm block: the wait covers the longer of the two whatever precedes the block.
template <int CTRL, int RM> __device__ __forceinline__ i64 dpp_add_i64(i64 v);
#define CSV_DPP_ADD64(CTRL, RM, TXT)                                                                                              \
    template <> __device__ __forceinline__ i64 dpp_add_i64<CTRL, RM>(i64 v)                                                       \
    {                                                                                                                             \
        unsigned lo = (unsigned)((u64)v & 0xffffffffull), hi = (unsigned)((u64)v >> 32);                                          \
        asm volatile("s_nop 4\n\tv_add_co_u32_dpp %0, vcc, %0, %0 " TXT "\n\tv_addc_co_u32_dpp %1, vcc, %1, %1, vcc " TXT         \
                     : "+v"(lo), "+v"(hi) : : "vcc");                                                                             \
        return (i64)(((u64)hi << 32) | lo);                                                                                       \
    }
CSV_DPP_ADD64(0x111, 0xf, "row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1")
CSV_DPP_ADD64(0x112, 0xf, "row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1")
CSV_DPP_ADD64(0x114, 0xf, "row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1")
CSV_DPP_ADD64(0x118, 0xf, "row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1")
CSV_DPP_ADD64(0x142, 0xa, "row_bcast:15 row_mask:0xa bank_mask:0xf")
CSV_DPP_ADD64(0x143, 0xc, "row_bcast:31 row_mask:0xc bank_mask:0xf")
#undef CSV_DPP_ADD64
__device__ __forceinline__ i64 wave_incl_scan_i64(i64 v)
{
    v = dpp_add_i64<0x111, 0xf>(v);     // row_shr:1
    v = dpp_add_i64<0x112, 0xf>(v);     // row_shr:2
    v = dpp_add_i64<0x114, 0xf>(v);     // row_shr:4
    v = dpp_add_i64<0x118, 0xf>(v);     // row_shr:8
    v = dpp_add_i64<0x142, 0xa>(v);     // row_bcast:15 into rows 1 and 3
    v = dpp_add_i64<0x143, 0xc>(v);     // row_bcast:31 into rows 2 and 3
    return v;
}
__device__ __forceinline__ int wave_incl_scan_i32(int v)
{
    v += dpp_i32<0x111, 0xf>(0, v);
    v += dpp_i32<0x112, 0xf>(0, v);
    v += dpp_i32<0x114, 0xf>(0, v);
    v += dpp_i32<0x118, 0xf>(0, v);
    v += dpp_i32<0x142, 0xa>(0, v);
    v += dpp_i32<0x143, 0xc>(0, v);
    return v;
}
__device__ __forceinline__ i64 wave_incl_max_i64(i64 v)
{
    i64 t;
    t = dpp_i64<0x111, 0xf>(INT64_MIN, v); v = t > v ? t : v;
    t = dpp_i64<0x112, 0xf>(INT64_MIN, v); v = t > v ? t : v;
    t = dpp_i64<0x114, 0xf>(INT64_MIN, v); v = t > v ? t : v;
    t = dpp_i64<0x118, 0xf>(INT64_MIN, v); v = t > v ? t : v;
    t = dpp_i64<0x142, 0xa>(INT64_MIN, v); v = t > v ? t : v;
    t = dpp_i64<0x143, 0xc>(INT64_MIN, v); v = t > v ? t : v;
    return v;
}
// totals come back through v_readlane of lane 63: wave-uniform (SGPR) results
__device__ __forceinline__ i64 lane63_i64(i64 v) { return readlane_i64(v, 63); }
__device__ __forceinline__ i64 wave_sum_i64(i64 v) { return lane63_i64(wave_incl_scan_i64(v)); }
__device__ __forceinline__ int wave_sum_i32(int v)
{
    return __builtin_amdgcn_readlane(wave_incl_scan_i32(v), 63);
}
// value of the lane to the left (lane 0 gets 0): DPP wave_shr:1
__device__ __forceinline__ i64 wave_shr1_i64(i64 v) { return dpp_i64<0x138, 0xf>(0, v); }

// sum of p[0 .. n) over the workgroup (256 threads); every thread gets the result
__device__ __forceinline__ i64 block_prefix_of(const int* p, int n, i64* sh)
{
    i64 v = 0;
    for (int i = threadIdx.x; i < n; i += 256) v += p[i];
    v = wave_sum_i64(v);
    if (lane_id() == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const i64 t = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return t;
}
__device__ __forceinline__ i64 block_prefix_of64(const i64* p, int n, i64* sh)
{
    i64 v = 0;
    for (int i = threadIdx.x; i < n; i += 256) v += p[i];
    v = wave_sum_i64(v);
    if (lane_id() == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const i64 t = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return t;
}

}  // namespace csv
