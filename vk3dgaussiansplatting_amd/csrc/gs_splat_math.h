// gs_splat_math.h -- the per-splat expressions more than one kernel file evaluates, each written once (device).  Every
// .hip file is built with -ffp-contract=off and correctly rounded division and square root, so an expression of this header
// gives the same floats wherever it is compiled: the frame (gs_project.hip), its backward (gs_backward.hip), the upload
// (gs_upload.hip), density control (gs_densify.hip), the raw space (gs_raw.hip) and MCMC (gs_mcmc.hip) agree bit for bit
// because they call the same function.
#pragma once

#include <float.h>

#include "gs_device_utils.h"
#include "gs_internal.h"

namespace gs {

struct Mat3 { float m[3][3]; }; // column-major m[col][row], like GLSL mat3x3

// GLSL `M * v`, M column-major: ((M[0]*v.x + M[1]*v.y) + M[2]*v.z) + M[3]*v.w
__device__ __forceinline__ void mat4_mul_vec4(const float* m, float vx, float vy, float vz,
                                              float vw, float out[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float acc = m[0 * 4 + r] * vx;
        acc = acc + m[1 * 4 + r] * vy;
        acc = acc + m[2 * 4 + r] * vz;
        acc = acc + m[3 * 4 + r] * vw;
        out[r] = acc;
    }
}

// Common/Common.glsl:17-30 (column-major constructor: col0, col1, col2); R[row][col] = m[col][row]
__device__ __forceinline__ Mat3 get_rot_mat(float r, float x, float y, float z) {
    Mat3 m;
    m.m[0][0] = 1.0f - 2.0f * y * y - 2.0f * z * z;
    m.m[0][1] = 2.0f * x * y - 2.0f * r * z;
    m.m[0][2] = 2.0f * x * z + 2.0f * r * y;
    m.m[1][0] = 2.0f * x * y + 2.0f * r * z;
    m.m[1][1] = 1.0f - 2.0f * x * x - 2.0f * z * z;
    m.m[1][2] = 2.0f * y * z - 2.0f * r * x;
    m.m[2][0] = 2.0f * x * z - 2.0f * r * y;
    m.m[2][1] = 2.0f * y * z + 2.0f * r * x;
    m.m[2][2] = 1.0f - 2.0f * x * x - 2.0f * y * y;
    return m;
}

// The radius of getGaussianTileExtents (InitSortList.comp:47-68) from the 2-D covariance (cx, cy; cy, cz):
// ceil(3 sqrt(largest eigenvalue))
__device__ __forceinline__ float tile_extent_radius(float cx, float cy, float cz) {
    const float det = cx * cz - cy * cy;
    const float m = (cx + cz) * 0.5f;
    const float lambda0 = m + sqrtf(maxf(m * m - det, 0.0f));
    const float lambda1 = m - sqrtf(maxf(m * m - det, 0.0f));
    return ceilf(3.0f * sqrtf(maxf(lambda0, lambda1)));
}

// ---- the counter-based random words of gs_densify.hip and gs_mcmc.hip (the header's mix)

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// The standard normal of (seed, g, child, axis): Box-Muller on two counter-based words
__device__ __forceinline__ float densify_normal(uint32_t h, uint32_t child, uint32_t axis) {
    const uint32_t w0 = mix32(h + (child * 6u + axis * 2u + 1u) * 0x9E3779B9u);
    const uint32_t w1 = mix32(h + (child * 6u + axis * 2u + 2u) * 0x9E3779B9u);
    const float u1 = (float)((w0 >> 8) + 1u) * 0x1p-24f;         // (0, 1]
    const float u2 = (float)(w1 >> 8) * 0x1p-24f;                // [0, 1)
    return sqrtf(-2.0f * logf(u1)) * cosf(6.2831855f * u2);
}

// ---- the raw parameter space of gs_raw.hip and gs_mcmc.hip: act() of the header and its inverse

constexpr uint32_t kQuadScale = kRecScale / 4u, kQuadRot = kRecRot / 4u, kQuadDc = kRecSh / 4u;   // the quads act() changes
static_assert(kRecOpacity == kQuadDc * 4u + 3u, "the opacity is the w of the SH-DC quad");

// 1 / |q| in the association of the loader (gs_ply.cpp convert_row, glm::normalize)
__device__ __forceinline__ float inv_length4(float x, float y, float z, float w) {
    const float t0 = x * x, t1 = y * y, t2 = z * z, t3 = w * w;
    return 1.0f / sqrtf((t0 + t1) + (t2 + t3));
}

__device__ __forceinline__ float sigmoid_pinned(float x) { return 1.0f / (1.0f + exp_pinned(-x)); }

// act(raw) on one leading quad, in place: the header's expressions in the header's order
__device__ __forceinline__ void act_quad(uint32_t quad, float3& p, float& w) {
    if (quad == kQuadScale) {
        p.x = exp_pinned(p.x); p.y = exp_pinned(p.y); p.z = exp_pinned(p.z);
    } else if (quad == kQuadRot) {
        const float inv = inv_length4(p.x, p.y, p.z, w);
        p.x = p.x * inv; p.y = p.y * inv; p.z = p.z * inv; w = w * inv;
    } else if (quad == kQuadDc) {
        w = sigmoid_pinned(w);
    }
}

// the inverse, with the device's logf and the two clamps of the header
__device__ __forceinline__ float log_scale(float s) { return logf(s < FLT_MIN ? FLT_MIN : s); }
__device__ __forceinline__ float logit_opacity(float o) {
    const float c = o < 0x1p-24f ? 0x1p-24f : (o > 0x1.fffffep-1f ? 0x1.fffffep-1f : o);
    return logf(c / (1.0f - c));
}

// The first COLS columns of splat g's rows (BackwardBuffers::rows) summed in slot order, from 0.0f, over the slots below the
// capacity; zero for a splat that emits nothing in this frame (SplatCounts::of).  Only the summed columns are read.
// STRIDE: the floats of a row -- kRowFloats, or kAbsRowFloats for the pairs of BackwardBuffers::abs_rows.
template <int STRIDE = kRowFloats, int COLS>
__device__ __forceinline__ void splat_row_sum(const SplatCounts& counts, const uint32_t* __restrict__ offsets,
                                              const float* __restrict__ rows, uint32_t g, uint32_t capacity,
                                              float (&acc)[COLS]) {
#pragma unroll
    for (int k = 0; k < COLS; ++k) acc[k] = 0.0f;
    const uint64_t o = offsets[g];
    const uint64_t e = o + counts.of(g);
    const uint64_t stop = e < capacity ? e : capacity;
    for (uint64_t s = o; s < stop; ++s) {
        const float* r = rows + s * STRIDE;
#pragma unroll
        for (int k = 0; k < COLS; ++k) acc[k] += r[k];
    }
}

} // namespace gs
