// gs_device_utils.h -- wave64 / workgroup primitives for gfx950.  Wave width is hard-coded to 64.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gs {

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ int wave_id() { return threadIdx.x >> 6; }

// number of set bits of `mask` below this lane (v_mbcnt_lo/hi)
__device__ __forceinline__ uint32_t mbcnt(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                     __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__device__ __forceinline__ uint32_t wave_reduce_add(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v; // every lane holds the sum
}

// Inclusive prefix sum over the wave with six DPP adds (row_shr 1/2/4/8, row_bcast 15/31): lane l gets
// x_0 + ... + x_l, so lane 63 holds the wave total.  Pure VALU (no LDS crossbar traffic, unlike
// __shfl_up / __shfl_xor).  Every lane of the wave must be active at the call.
__device__ __forceinline__ uint32_t wave_sum_to_lane63(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xe, false);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xc, false);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31
    return v;
}

// Inclusive prefix maximum (unsigned) over the wave, same six DPP steps with max; 0 is the identity.
__device__ __forceinline__ uint32_t wave_inclusive_max(uint32_t v) {
    auto mx = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xe, false));   // row_shr:4
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xc, false));   // row_shr:8
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));   // row_bcast:15
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));   // row_bcast:31
    return v;
}

// inclusive prefix sum inside each row of 16 lanes (DPP row_shr 1/2/4/8; lanes shifted in from outside the row add 0)
__device__ __forceinline__ uint32_t row16_inclusive_scan(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xe, false);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xc, false);   // row_shr:8
    return v;
}

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {   // all 64 lanes active
    return wave_sum_to_lane63(v);
}

__device__ __forceinline__ uint64_t wave_inclusive_scan64(uint64_t v) {
    const int lane = lane_id();
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        uint32_t lo = __shfl_up((uint32_t)v, off, 64);
        uint32_t hi = __shfl_up((uint32_t)(v >> 32), off, 64);
        uint64_t t = ((uint64_t)hi << 32) | lo;
        if (lane >= off) v += t;
    }
    return v;
}

// The value of another lane of the row of 16 by DPP (pure VALU, no LDS crossbar); every lane of the wave must be active
template <int CTRL>
__device__ __forceinline__ float row_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

// A six-level butterfly over the wave, lanes 2 k and 2 k + 1 first, then adjacent pair results: lane l combines with lane
// l ^ 1, ^ 2, ^ 4, ^ 8 by DPP -- quad_perm [1,0,3,2] and [2,3,0,1], then row_half_mirror and row_mirror: once the lanes of a
// group of 4 (8) hold the same bits, the mirrored lane holds those of the group l ^ 4 (l ^ 8) lies in -- and with l ^ 16,
// ^ 32 by shuffles.  Both operands of every level are the same two values in either order, so with a commutative op every
// lane ends with the same bits.
template <class Op>
__device__ __forceinline__ float wave_tree(float v, Op op) {
    v = op(v, row_dpp<0xB1>(v));
    v = op(v, row_dpp<0x4E>(v));
    v = op(v, row_dpp<0x141>(v));
    v = op(v, row_dpp<0x140>(v));
    v = op(v, __shfl_xor(v, 16, 64));
    return op(v, __shfl_xor(v, 32, 64));
}

// GLSL clamp(x, lo, hi) = min(max(x, lo), hi) with the comparison forms the oracle uses.
__device__ __forceinline__ float clampf(float x, float lo, float hi) {
    float t = x > lo ? x : lo;
    return t < hi ? t : hi;
}
__device__ __forceinline__ float maxf(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ int clampi(int x, int lo, int hi) {
    return x < lo ? lo : (x > hi ? hi : x);
}

// GLSL int(float) / uint(float): truncate, saturate, NaN -> 0 (what v_cvt_i32_f32 / v_cvt_u32_f32 do;
// written out so the result does not depend on the compiler's treatment of out-of-range casts).
__device__ __forceinline__ int f2i_sat(float x) {
    if (x != x) return 0;
    if (x >= 2147483648.0f) return 2147483647;
    if (x <= -2147483648.0f) return (-2147483647 - 1);
    return (int)x;
}
__device__ __forceinline__ uint32_t f2u_sat(float x) {
    if (x != x) return 0u;
    if (x >= 4294967296.0f) return 0xFFFFFFFFu;
    if (x <= 0.0f) return 0u;
    return (uint32_t)x;
}

// pinned exp: identical operation sequence to gso_exp() in oracle/gs_oracle.c, for every float: both clamps, so positive
// arguments are served too (t = +-126 at the ends; a NaN fails `t > -126` and goes to the lower clamp, 2^-126)
__device__ __forceinline__ float exp_pinned(float x) {
    float t = x * 0x1.715476p+0f;
    t = t > -126.0f ? t : -126.0f;
    t = t < 126.0f ? t : 126.0f;
    const float n = __builtin_rintf(t);
    const float r = t - n;
    float p = 0x1.42059ap-13f;
    p = __builtin_fmaf(p, r, 0x1.5f3e12p-10f);
    p = __builtin_fmaf(p, r, 0x1.3b2d40p-7f);
    p = __builtin_fmaf(p, r, 0x1.c6aeeap-5f);
    p = __builtin_fmaf(p, r, 0x1.ebfbdcp-3f);
    p = __builtin_fmaf(p, r, 0x1.62e430p-1f);
    p = __builtin_fmaf(p, r, 1.0f);
    return __builtin_ldexpf(p, (int)n);
}

// exp_pinned_live of gs_render.hip (its scalar form, shared with the blend backward of gs_backward.hip): the pinned exp of
// oracle/gs_oracle.h, bit for bit, for every x <= 0 (see exp_pinned2_live in gs_render.hip)
__device__ __forceinline__ float exp_pinned_live(float x) {            // the scalar form of exp_pinned2_live
    const float t = __builtin_fmaxf(x * 0x1.715476p+0f, -126.0f);
    const float tn = t + 12582912.0f;
    const float r = t - (tn - 12582912.0f);
    float p = 0x1.42059ap-13f;
    p = __builtin_fmaf(p, r, 0x1.5f3e12p-10f);
    p = __builtin_fmaf(p, r, 0x1.3b2d40p-7f);
    p = __builtin_fmaf(p, r, 0x1.c6aeeap-5f);
    p = __builtin_fmaf(p, r, 0x1.ebfbdcp-3f);
    p = __builtin_fmaf(p, r, 0x1.62e430p-1f);
    p = __builtin_fmaf(p, r, 1.0f);
    return __uint_as_float(__float_as_uint(p) + (__float_as_uint(tn) << 23));
}

} // namespace gs
