// gs_densify.hip -- adaptive density control on the device (include/gsplat.h, no reference counterpart):
//   gs_densify_stats_device : k_densify_stats, per listed splat of the frame the screen-gradient norm, a visit count and the
//                   largest screen radius, accumulated into the caller's arrays;
//   gs_densify_device       : the rule per input splat (pruned / kept / clone / split) evaluated three times instead of stored --
//                   k_dens_block_sums + k_dens_scan_blocks + k_dens_offsets give o(g), the exclusive scan of the number of
//                   outputs k(g) (the trio of gs_backward.hip with four sums per block: outputs, cloned, split, pruned), and
//                   k_dens_write moves the records: a lane per (input splat, group of four floats), so a wave reads 1 KiB of
//                   consecutive bytes of records, m and v and writes the outputs of g next to those of g - 1 -- the children
//                   sit beside their parent, and the storage order keeps its locality.
// No float atomics, nothing read back by the host: both calls are bitwise reproducible.  Built with -ffp-contract=off and
// correctly rounded division and square root, like gs_adam.hip.
#include "gs_device_utils.h"
#include "gs_internal.h"

namespace gs {

namespace {

constexpr uint32_t kRowFloats = 10;      // a row of BackwardBuffers::rows (gs_backward.hip): sx, sy first
constexpr uint32_t kRecordQuads = 21;    // a record is 21 groups of four floats

// The rule of the header: 0 pruned, 1 kept, 2 clone, 3 split.  Every comparison as the header writes it: a NaN compares false.
__device__ __forceinline__ uint32_t densify_kind(float s0, float s1, float s2, float op, float accum, uint32_t seen,
                                                 float radius, const DensifyRule& r) {
    const float smax = maxf(maxf(s0, s1), s2);
    const bool pruned = op < r.prune_opacity || smax > r.prune_scale || radius > r.prune_radius;
    const float mean = seen ? accum / (float)seen : 0.0f;
    const bool grow = !pruned && mean >= r.grad_threshold;
    const bool split = grow && smax > r.split_scale;
    return pruned ? 0u : (!grow ? 1u : (split ? 3u : 2u));
}

__device__ __forceinline__ uint32_t densify_kind_of(const float* __restrict__ records, const float* __restrict__ grad_accum,
                                                    const uint32_t* __restrict__ seen, const float* __restrict__ max_radius,
                                                    uint32_t g, const DensifyRule& r) {
    const float4 sc = *reinterpret_cast<const float4*>(records + (size_t)g * 84u + 4u);
    return densify_kind(sc.x, sc.y, sc.z, records[(size_t)g * 84u + 15u], grad_accum[g], seen[g], max_radius[g], r);
}

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

}  // namespace

// ---- statistics of one step ---------------------------------------------------------------------------------------

// Thread i < min(*count, max_rows) handles g = ids[i] (an id >= n is skipped).  The splat's rows are summed as bwd_row_sum of
// gs_backward.hip sums them -- slot order, clamped at the capacity, from 0.0f -- for columns 0 and 1: the bits
// bwd_chain_record consumed as dsx, dsy.  The radius is that of k_project (gs_project.hip, getGaussianTileExtents) on the
// covariance the frame stored in the raster record.
__global__ __launch_bounds__(256) void k_densify_stats(const DensifyStatsArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t listed = *a.count, rows = listed < a.max_rows ? listed : a.max_rows;
    if (i >= rows) return;
    const uint32_t g = a.ids[i];
    if (g >= a.n) return;
    float dsx = 0.0f, dsy = 0.0f;
    const uint64_t o = a.offsets[g];
    const uint64_t e = o + a.touched[g];
    const uint64_t stop = e < a.capacity ? e : a.capacity;
    for (uint64_t s = o; s < stop; ++s) {
        const float* r = a.rows + s * kRowFloats;
        dsx += r[0];
        dsy += r[1];
    }
    const float gx = dsx * 0.5f * (float)a.width, gy = dsy * 0.5f * (float)a.height;
    const float norm = sqrtf(gx * gx + gy * gy);
    a.grad_accum[g] = a.grad_accum[g] + norm;
    a.seen[g] += 1u;

    const SplatRaster* rec = a.raster + g;
    const float cx = rec->cx, cy = rec->cy, cz = rec->cz;
    const float det = cx * cz - cy * cy;
    const float m = (cx + cz) * 0.5f;
    const float lambda0 = m + sqrtf(maxf(m * m - det, 0.0f));
    const float lambda1 = m - sqrtf(maxf(m * m - det, 0.0f));
    const float radius = ceilf(3.0f * sqrtf(maxf(lambda0, lambda1)));
    const float old = a.max_radius[g];
    a.max_radius[g] = radius > old ? radius : old;
}

void launch_densify_stats(const DensifyStatsArgs& a, hipStream_t stream) {
    if (a.max_rows == 0) return;
    hipLaunchKernelGGL(k_densify_stats, dim3(backward_blocks(a.max_rows)), dim3(256), 0, stream, a);
}

// ---- the new cloud ------------------------------------------------------------------------------------------------

// block_sums: [4][blocks] -- outputs, cloned, split, pruned of the block's 256 splats
__global__ __launch_bounds__(256) void k_dens_block_sums(const DensifyArgs a, uint32_t blocks) {
    __shared__ uint32_t s_w[4][4];
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    const uint32_t kind = g < a.n ? densify_kind_of(a.records, a.grad_accum, a.seen, a.max_radius, g, a.rule) : 4u;
    const uint32_t clones = (uint32_t)__popcll(__ballot(kind == 2u)), splits = (uint32_t)__popcll(__ballot(kind == 3u));
    const uint32_t kept = (uint32_t)__popcll(__ballot(kind == 1u)), pruned = (uint32_t)__popcll(__ballot(kind == 0u));
    if (lane_id() == 0) {
        s_w[0][wave_id()] = kept + 2u * (clones + splits);
        s_w[1][wave_id()] = clones;
        s_w[2][wave_id()] = splits;
        s_w[3][wave_id()] = pruned;
    }
    __syncthreads();
    if (threadIdx.x < 4u) {
        const uint32_t q = threadIdx.x;
        a.block_sums[(size_t)q * blocks + blockIdx.x] = s_w[q][0] + s_w[q][1] + s_w[q][2] + s_w[q][3];
    }
}

// One workgroup: the exclusive scan of the blocks' output counts, every thread owning `per` consecutive blocks, and the four
// totals into counts_out.  n < 2^31 (the host refuses more), so no total passes 2^32 - 2.
__global__ __launch_bounds__(256) void k_dens_scan_blocks(const uint32_t* __restrict__ block_sums, uint32_t blocks,
                                                           uint32_t* __restrict__ block_offsets,
                                                           uint32_t* __restrict__ counts_out) {
    __shared__ uint32_t s_w[4][4];
    const uint32_t per = (blocks + 255u) / 256u;
    const uint32_t b0 = threadIdx.x * per;
    uint32_t mine[4] = {0u, 0u, 0u, 0u};
    for (uint32_t k = 0; k < per; ++k) {
        if (b0 + k < blocks) {
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q) mine[q] += block_sums[(size_t)q * blocks + b0 + k];
        }
    }
    uint32_t inc[4];
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) inc[q] = wave_inclusive_scan(mine[q]);
    if (lane_id() == 63) {
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) s_w[q][wave_id()] = inc[q];
    }
    __syncthreads();
    uint32_t run = inc[0] - mine[0];
    for (int w = 0; w < wave_id(); ++w) run += s_w[0][w];
    for (uint32_t k = 0; k < per; ++k) {
        if (b0 + k < blocks) {
            block_offsets[b0 + k] = run;
            run += block_sums[b0 + k];
        }
    }
    if (threadIdx.x < 4u) {
        const uint32_t q = threadIdx.x;
        counts_out[q] = s_w[q][0] + s_w[q][1] + s_w[q][2] + s_w[q][3];
    }
}

// offsets[g] = o(g), the index of g's first output
__global__ __launch_bounds__(256) void k_dens_offsets(const DensifyArgs a) {
    __shared__ uint32_t s_w[4];
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    const uint32_t kind = g < a.n ? densify_kind_of(a.records, a.grad_accum, a.seen, a.max_radius, g, a.rule) : 0u;
    const uint32_t cnt = kind == 0u ? 0u : (kind == 1u ? 1u : 2u);
    const uint32_t inc = wave_inclusive_scan(cnt);
    if (lane_id() == 63) s_w[wave_id()] = inc;
    __syncthreads();
    uint32_t before = a.block_offsets[blockIdx.x] + (inc - cnt);
    for (int w = 0; w < wave_id(); ++w) before += s_w[w];
    if (g < a.n) a.offsets[g] = before;
}

// A lane per (input splat g, group q of four floats): consecutive lanes read consecutive 16 bytes of records, m and v.  The
// lanes of g write group q of its k(g) outputs, rows o(g) .. o(g) + k(g) - 1, while they are below max_out.  Group 0 of a
// split child carries the new position, group 1 the new scale; every other float is the parent's.
template <bool MOMENTS>
__global__ __launch_bounds__(256) void k_dens_write(const DensifyArgs a) {
    const uint64_t item = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t g = (uint32_t)(item / kRecordQuads), q = (uint32_t)(item % kRecordQuads);
    if (g >= a.n) return;
    const uint32_t kind = densify_kind_of(a.records, a.grad_accum, a.seen, a.max_radius, g, a.rule);
    if (kind == 0u) return;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 rec = reinterpret_cast<const float4*>(a.records)[item];
    float4 mm = zero4, vv = zero4;
    if (MOMENTS && kind != 3u) {       // kept, and the first output of a clone: the moments travel with the record
        mm = reinterpret_cast<const float4*>(a.m)[item];
        vv = reinterpret_cast<const float4*>(a.v)[item];
    }
    const uint32_t o = a.offsets[g];
    float4 out[2] = {rec, rec};
    if (kind == 3u && q < 2u) {
        const float* p = a.records + (size_t)g * 84u;
        const float s[3] = {p[4], p[5], p[6]};
        if (q == 1u) {
            out[0] = make_float4(s[0] / a.split_shrink, s[1] / a.split_shrink, s[2] / a.split_shrink, rec.w);
            out[1] = out[0];
        } else {
            const float qr = p[8], qx = p[9], qy = p[10], qz = p[11];
            float R[3][3];                                          // R[row][col] of getRotMat, as gs_backward.hip writes it
            R[0][0] = 1.0f - 2.0f * qy * qy - 2.0f * qz * qz; R[1][0] = 2.0f * qx * qy - 2.0f * qr * qz; R[2][0] = 2.0f * qx * qz + 2.0f * qr * qy;
            R[0][1] = 2.0f * qx * qy + 2.0f * qr * qz; R[1][1] = 1.0f - 2.0f * qx * qx - 2.0f * qz * qz; R[2][1] = 2.0f * qy * qz - 2.0f * qr * qx;
            R[0][2] = 2.0f * qx * qz - 2.0f * qr * qy; R[1][2] = 2.0f * qy * qz + 2.0f * qr * qx; R[2][2] = 1.0f - 2.0f * qx * qx - 2.0f * qy * qy;
            const uint32_t h = mix32(mix32(g ^ (uint32_t)a.seed) + (uint32_t)(a.seed >> 32));
#pragma unroll
            for (uint32_t c = 0; c < 2u; ++c) {
                const float z[3] = {densify_normal(h, c, 0u), densify_normal(h, c, 1u), densify_normal(h, c, 2u)};
                float pos[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float off = ((R[i][0] * s[0]) * z[0] + (R[i][1] * s[1]) * z[1]) + (R[i][2] * s[2]) * z[2];
                    pos[i] = p[i] + off;
                }
                out[c] = make_float4(pos[0], pos[1], pos[2], rec.w);
            }
        }
    }
    const bool two = kind >= 2u;
    if (o < a.max_out) {
        const size_t at = (size_t)o * kRecordQuads + q;
        reinterpret_cast<float4*>(a.records_out)[at] = out[0];
        if (MOMENTS) {
            reinterpret_cast<float4*>(a.m_out)[at] = kind == 3u ? zero4 : mm;
            reinterpret_cast<float4*>(a.v_out)[at] = kind == 3u ? zero4 : vv;
        }
    }
    if (two && o + 1u < a.max_out) {           // o + 1 < 2^32: the outputs number at most 2 n
        const size_t at = (size_t)(o + 1u) * kRecordQuads + q;
        reinterpret_cast<float4*>(a.records_out)[at] = out[1];
        if (MOMENTS) {
            reinterpret_cast<float4*>(a.m_out)[at] = zero4;
            reinterpret_cast<float4*>(a.v_out)[at] = zero4;
        }
    }
}

void launch_densify(const DensifyArgs& a, uint32_t* counts_out, hipStream_t stream) {
    const uint32_t blocks = backward_blocks(a.n);
    hipLaunchKernelGGL(k_dens_block_sums, dim3(blocks), dim3(256), 0, stream, a, blocks);
    hipLaunchKernelGGL(k_dens_scan_blocks, dim3(1), dim3(256), 0, stream, a.block_sums, blocks, a.block_offsets, counts_out);
    hipLaunchKernelGGL(k_dens_offsets, dim3(blocks), dim3(256), 0, stream, a);
    if (a.max_out == 0) return;
    const uint64_t wblocks = ((uint64_t)a.n * kRecordQuads + 255u) / 256u;       // < 2^28 for n < 2^31
    if (a.m) hipLaunchKernelGGL(k_dens_write<true>, dim3((uint32_t)wblocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k_dens_write<false>, dim3((uint32_t)wblocks), dim3(256), 0, stream, a);
}

}  // namespace gs
