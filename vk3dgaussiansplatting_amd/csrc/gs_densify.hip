// gs_densify.hip -- adaptive density control on the device (include/gsplat.h, no reference counterpart):
//   gs_densify_stats_device : k_densify_stats, per listed splat of the frame the screen-gradient norm, a visit count and the
//                   largest screen radius, accumulated into the caller's arrays;
//   gs_densify_device       : the rule per input splat (pruned / kept / clone / split) evaluated three times instead of stored --
//                   the per-splat scan of gs_splat_scan.h over DensifySource gives o(g), the exclusive scan of the number of
//                   outputs k(g), and the four totals (outputs, cloned, split, pruned), and k_dens_write moves the records: a
//                   lane per (input splat, quad), so a wave reads 1 KiB of consecutive bytes of records, m and v and writes
//                   the outputs of g next to those of g - 1 -- the children sit beside their parent, and the storage order
//                   keeps its locality;
//   gs_prune_below_device   : the stable compaction of the cloud by a per-splat score -- the same scan over PruneSource (kept,
//                   dropped) and k_prune_write, k_dens_write's mapping with plain copies.
// No float atomics, nothing read back by the host: all three calls are bitwise reproducible.
#include "gs_splat_math.h"
#include "gs_splat_scan.h"

namespace gs {

namespace {

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
    const float4 sc = *reinterpret_cast<const float4*>(records + (size_t)g * kRecordFloats + kRecScale);
    return densify_kind(sc.x, sc.y, sc.z, records[(size_t)g * kRecordFloats + kRecOpacity], grad_accum[g], seen[g], max_radius[g], r);
}

// The rows of the scan: the outputs k(g) of splat g, then the flags cloned, split, pruned (their totals alone are used)
struct DensifySource {
    static constexpr uint32_t K = 4u, kPlaced = 1u, kTotalsFrom = 0u;
    DensifyArgs a;
    __device__ void counts(uint32_t g, uint32_t (&c)[K]) const {
        const uint32_t kind = densify_kind_of(a.records, a.grad_accum, a.seen, a.max_radius, g, a.rule);
        c[0] = kind == 0u ? 0u : (kind == 1u ? 1u : 2u);
        c[1] = kind == 2u ? 1u : 0u;
        c[2] = kind == 3u ? 1u : 0u;
        c[3] = kind == 0u ? 1u : 0u;
    }
};

}  // namespace

// ---- statistics of one step ---------------------------------------------------------------------------------------

// Thread i < min(*count, max_rows) handles g = ids[i] (an id >= n is skipped).  Columns 0 and 1 of the splat's summed row are
// the dsx, dsy of the backward's chain; the radius is the frame's, on the covariance it stored in the raster record.
__global__ __launch_bounds__(256) void k_densify_stats(const DensifyStatsArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t listed = *a.count, rows = listed < a.max_rows ? listed : a.max_rows;
    if (i >= rows) return;
    const uint32_t g = a.ids[i];
    if (g >= a.n) return;
    float ds[2];
    splat_row_sum(a.counts, a.offsets, a.rows, g, a.capacity, ds);
    const float gx = ds[0] * 0.5f * (float)a.width, gy = ds[1] * 0.5f * (float)a.height;
    const float norm = sqrtf(gx * gx + gy * gy);
    a.grad_accum[g] = a.grad_accum[g] + norm;
    a.seen[g] += 1u;

    // the frame stores the records of emitting splats (k_project): a listed id that emitted nothing in this frame (a caller's
    // union of several frames' lists) has a stale or zero record, which counts as the zero one -- radius 0
    if (a.counts.of(g) == 0u) return;
    const SplatRaster* rec = a.raster + g;
    const float radius = tile_extent_radius(rec->cx, rec->cy, rec->cz);
    const float old = a.max_radius[g];
    a.max_radius[g] = radius > old ? radius : old;
}

void launch_densify_stats(const DensifyStatsArgs& a, hipStream_t stream) {
    if (a.max_rows == 0) return;
    hipLaunchKernelGGL(k_densify_stats, dim3(backward_blocks(a.max_rows)), dim3(256), 0, stream, a);
}

// ---- absolute screen gradients (gs_set_abs_gradients) -------------------------------------------------------------

// Thread i < min(*count, max_rows) handles g = ids[i]: the pairs of BackwardBuffers::abs_rows of splat g summed in slot
// order (splat_row_sum over rows of two floats).  ACCUM: out[g] += the norm of the pair in NDC units, an id >= n is skipped
// (k_densify_stats' expression on the absolute sums); else out[i] = the pair, (0, 0) for an id >= n.
template <bool ACCUM>
__global__ __launch_bounds__(256) void k_abs_gradient(const AbsGradArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t listed = *a.count, rows = listed < a.max_rows ? listed : a.max_rows;
    if (i >= rows) return;
    const uint32_t g = a.ids[i];
    float s[kAbsRowFloats] = {0.0f, 0.0f};
    if (g < a.n) splat_row_sum<kAbsRowFloats>(a.counts, a.offsets, a.abs_rows, g, a.capacity, s);
    if constexpr (ACCUM) {
        if (g >= a.n) return;
        const float ax = s[0] * 0.5f * (float)a.width, ay = s[1] * 0.5f * (float)a.height;
        a.out[g] = a.out[g] + sqrtf(ax * ax + ay * ay);
    } else {
        a.out[(size_t)i * kAbsRowFloats] = s[0];
        a.out[(size_t)i * kAbsRowFloats + 1] = s[1];
    }
}

void launch_abs_screen_gradient(const AbsGradArgs& a, hipStream_t stream) {
    if (a.max_rows == 0) return;
    hipLaunchKernelGGL(k_abs_gradient<false>, dim3(backward_blocks(a.max_rows)), dim3(256), 0, stream, a);
}

void launch_densify_stats_abs(const AbsGradArgs& a, hipStream_t stream) {
    if (a.max_rows == 0) return;
    hipLaunchKernelGGL(k_abs_gradient<true>, dim3(backward_blocks(a.max_rows)), dim3(256), 0, stream, a);
}

// ---- the new cloud ------------------------------------------------------------------------------------------------

// A lane per (input splat g, group q of four floats): consecutive lanes read consecutive 16 bytes of records, m and v.  The
// lanes of g write group q of its k(g) outputs, rows o(g) .. o(g) + k(g) - 1, while they are below max_out.  The position quad of
// a split child carries the new position, the scale quad the new scale; every other float is the parent's.
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
    const uint32_t o = a.scan.offsets[g];
    float4 out[2] = {rec, rec};
    if (kind == 3u && q <= kRecScale / 4u) {         // the quads of position and scale
        const float* p = a.records + (size_t)g * kRecordFloats;
        const float s[3] = {p[kRecScale], p[kRecScale + 1], p[kRecScale + 2]};
        if (q == kRecScale / 4u) {
            out[0] = make_float4(s[0] / a.split_shrink, s[1] / a.split_shrink, s[2] / a.split_shrink, rec.w);
            out[1] = out[0];
        } else {
            const Mat3 rm = get_rot_mat(p[kRecRot], p[kRecRot + 1], p[kRecRot + 2], p[kRecRot + 3]);   // R[row][col] = rm.m[col][row]
            const uint32_t h = mix32(mix32(g ^ (uint32_t)a.seed) + (uint32_t)(a.seed >> 32));
#pragma unroll
            for (uint32_t c = 0; c < 2u; ++c) {
                const float z[3] = {densify_normal(h, c, 0u), densify_normal(h, c, 1u), densify_normal(h, c, 2u)};
                float pos[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float off = ((rm.m[0][i] * s[0]) * z[0] + (rm.m[1][i] * s[1]) * z[1]) + (rm.m[2][i] * s[2]) * z[2];
                    pos[i] = p[kRecPos + i] + off;
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
    launch_splat_scan(DensifySource{a}, a.n, a.scan, counts_out, stream);      // n < 2^31 (the host refuses more): nothing saturates
    if (a.max_out == 0) return;
    const uint64_t wblocks = ((uint64_t)a.n * kRecordQuads + 255u) / 256u;       // < 2^28 for n < 2^31
    if (a.m) hipLaunchKernelGGL(k_dens_write<true>, dim3((uint32_t)wblocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k_dens_write<false>, dim3((uint32_t)wblocks), dim3(256), 0, stream, a);
}

// ---- pruning by a score -------------------------------------------------------------------------------------------

namespace {

// The comparison of the header as it writes it: a NaN score compares false and is dropped
__device__ __forceinline__ bool prune_keeps(const float* __restrict__ score, uint32_t g, float threshold) {
    return score[g] >= threshold;
}

// The rows of the scan: kept, dropped (both totals are the call's counts)
struct PruneSource {
    static constexpr uint32_t K = 2u, kPlaced = 1u, kTotalsFrom = 0u;
    const float* score;
    float threshold;
    __device__ void counts(uint32_t g, uint32_t (&c)[K]) const {
        c[0] = prune_keeps(score, g, threshold) ? 1u : 0u;
        c[1] = 1u - c[0];
    }
};

}  // namespace

// A lane per (input splat g, group q of four floats), like k_dens_write: a kept g below max_out has its quads copied to row
// offsets[g] of every output that is given.
__global__ __launch_bounds__(256) void k_prune_write(const PruneArgs a) {
    const uint64_t item = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t g = (uint32_t)(item / kRecordQuads), q = (uint32_t)(item % kRecordQuads);
    if (g >= a.n) return;
    if (!prune_keeps(a.score, g, a.threshold)) return;
    const uint32_t o = a.scan.offsets[g];
    if (o >= a.max_out) return;
    const size_t at = (size_t)o * kRecordQuads + q;
    reinterpret_cast<float4*>(a.records_out)[at] = reinterpret_cast<const float4*>(a.records)[item];
    if (a.raw) reinterpret_cast<float4*>(a.raw_out)[at] = reinterpret_cast<const float4*>(a.raw)[item];
    if (a.m) reinterpret_cast<float4*>(a.m_out)[at] = reinterpret_cast<const float4*>(a.m)[item];
    if (a.v) reinterpret_cast<float4*>(a.v_out)[at] = reinterpret_cast<const float4*>(a.v)[item];
}

void launch_prune_below(const PruneArgs& a, uint32_t* counts_out, hipStream_t stream) {
    launch_splat_scan(PruneSource{a.score, a.threshold}, a.n, a.scan, counts_out, stream);   // n < 2^31: nothing saturates
    if (a.max_out == 0) return;
    const uint64_t wblocks = ((uint64_t)a.n * kRecordQuads + 255u) / 256u;       // < 2^28 for n < 2^31
    hipLaunchKernelGGL(k_prune_write, dim3((uint32_t)wblocks), dim3(256), 0, stream, a);
}

}  // namespace gs
