// gs_backward.hip -- gradients of the last GS_RENDER_EXACT frame w.r.t. the uploaded gaussians (gs_backward*,
// include/gsplat.h), as five launches after the frame's own kernels.  The dense form (gs_backward*: a record gradient for
// every splat) and the visible form (gs_backward_visible*: for the splats of V = { g : tiles_touched[g] != 0 } alone, with
// their ids) run the same kernels; where they differ the kernel is a template on VIS.  tiles_touched[g] is everywhere the
// count of THIS frame, SplatCounts::of (gs_internal.h): in a band of tile rows the stored word of a culled block is stale.
// A band context (gs_set_band_gradients) runs the same launches over its own tiles: the result is the sum over its pixels.
//   the per-splat scan of gs_splat_scan.h over BwdSource<VIS> (three launches): offset[g] = sum of tiles_touched over the
//                   splats before g, the splat-order position of g's first element -- the position InitSortList's truncation
//                   goes by (k_emit, k_gather_sorted), so an element of the list has offset[g] + (its tile's index in g's box)
//                   below the capacity, and every such slot is an element of the list.  VIS carries a second row beside
//                   the first, the flag tiles_touched != 0: its exclusive scan is the position of g in V (ascending g by
//                   construction), vis_ids[position] = g, and its total is |V| (visible_count_of);
//   k_bwd_blend   : per tile, the blend of RenderGaussians.comp:112-142 replayed front to back with the pieces of
//                   gs_tile_replay.h (the staging, the entry test and the transmittance step, shared with k_contrib_blend
//                   of gs_contrib.hip: the same entries contribute and each pixel stops on the same entry K with the same
//                   T_K).  What this kernel adds: the walk back to front with the colour behind every entry as a running
//                   sum; the 256 pixels' derivatives of each list entry are reduced on chip in a fixed tree and stored as
//                   one 10-float row in the slot of the entry, with plain stores.  A template on ABS (gs_set_abs_gradients):
//                   <true> also reduces |d/dsx| and |d/dsy| of every (entry, pixel) and stores the pair in the entry's slot of
//                   abs_rows, which gs_abs_screen_gradient_device / gs_densify_stats_abs_device sum (gs_densify.hip);
//   k_bwd_rowsum_chain<VIS> : per splat, its rows summed in slot order (= tile raster order inside its box), then the sum
//                   through the per-splat part of the frame (conic <- 2-D covariance <- scale, rotation; screen position
//                   and depth <- position; colour <- SH coefficients and position: bwd_chain<false> of gs_bwd_chain.h, which
//                   gs_camera.hip instantiates with <true> for the camera), written in the 336-byte record layout
//                   of gs_upload_gaussians.  Dense: thread g < N writes record g.  VIS: thread i < min(|V|, max_rows)
//                   handles g = vis_ids[i] and writes record i.
// Dense: launch_backward runs all five.  Visible: launch_backward_visible_scan runs the scan (alone it is
// gs_visible_count), launch_backward_visible_rows the last two.
// No float atomics anywhere: the gradients are bitwise reproducible, and the same for every sorter and launch shape of
// the forward (they depend on the sorted list and the pixels only).
#include "gs_bwd_chain.h"
#include "gs_splat_scan.h"
#include "gs_tile_replay.h"

#include <type_traits>

namespace gs {

constexpr int kBwdBatch = 64;             // list entries staged per step of k_bwd_blend

// ---- per-splat slot offsets ---------------------------------------------------------------------------------------
// The rows of the scan.  VIS: the flag tiles_touched[g] != 0 beside tiles_touched[g], and V from its positions: vis_ids[position
// of g in V] = g for every g of V, and the same into ids_out (may be null) below max_rows.  The dense source carries none of it
// (its pointers are null and unused).
template <bool VIS>
struct BwdSource {
    static constexpr uint32_t K = VIS ? 2u : 1u, kPlaced = K, kTotalsFrom = 1u;
    SplatCounts frame;
    uint32_t *vis_ids, *ids_out;
    uint32_t max_rows;
    __device__ void counts(uint32_t g, uint32_t (&c)[K]) const {
        c[0] = frame.of(g);
        if constexpr (VIS) c[1] = c[0] != 0u ? 1u : 0u;
    }
    __device__ void place(uint32_t g, const uint32_t (&c)[K], const uint32_t (&pos)[K]) const {
        if constexpr (VIS) {
            if (c[0] != 0u) {                     // pos[1] < |V| <= n
                vis_ids[pos[1]] = g;
                if (ids_out && pos[1] < max_rows) ids_out[pos[1]] = g;
            }
        }
    }
};

// ---- blend backward -----------------------------------------------------------------------------------------------

struct BwdBlendArgs : TileListArgs {
    const float* pos;               // SceneBuffers::pos (the view depth of an entry) with grad_depth, else null
    const float4* grad_rgba;        // [H][W] dL/dRGBA32F
    const float* grad_depth;        // [H][W] dL/dDEPTH or null
    float* rows;                    // [capacity][kRowFloats]
};
struct BwdBlendAbsArgs : BwdBlendArgs {
    float* abs_rows;                // [capacity][kAbsRowFloats]  BackwardBuffers::abs_rows
};

// One 256-thread workgroup per owned tile, one pixel per lane: the replay of gs_tile_replay.h, then its walk back.
// ABS (gs_set_abs_gradients): two more columns per (entry, pixel), |v[0]| and |v[1]| of the very terms the signed columns
// add, through the same tree and the same combination of the four waves, stored as a pair in the entry's slot of abs_rows.
// Without ABS the columns, their LDS and their stores are compiled out: the kernel is the one it was, argument block included.
template <bool ABS>
__global__ __launch_bounds__(256) void k_bwd_blend(const FrameParams fp,
                                                   const std::conditional_t<ABS, BwdBlendAbsArgs, BwdBlendArgs> a) {
    constexpr int kPartFloats = ABS ? kRowFloats + kAbsRowFloats : kRowFloats;
    __shared__ float s_e[kBwdBatch][12];                 // staged entries, with colour and depth
    __shared__ float s_part[4][kBwdBatch][kPartFloats];  // per-wave sums of an entry's row (ABS: and of its absolute pair)
    __shared__ uint32_t s_kend;

    const TilePixel t = tile_pixel(fp, a.ranges);
    const uint32_t start = t.start, end = t.end;
    if (t.tid == 0) s_kend = 0u;

    // 1. forward replay: the last contributing entry K of the pixel and the transmittance T_K in front of it
    uint32_t last = 0xFFFFFFFFu;
    float T = 1.0f, TK = 0.0f;
    bool done = !t.inside;
    for (uint32_t i0 = start; i0 < end; i0 += kBwdBatch) {
        const uint32_t cnt = end - i0 < (uint32_t)kBwdBatch ? end - i0 : (uint32_t)kBwdBatch;
        stage_entries<true>(s_e, t, fp, a, a.pos, i0, cnt);
        __syncthreads();
        if (!done) {
            for (uint32_t j = 0; j < cnt; ++j) {
                float ex, ey, ef, next_t;
                bool contributes;
                const float alpha = entry_alpha(s_e[j], t, ex, ey, ef, contributes);
                if (!contributes) continue;
                const bool stops = transmittance_step(T, alpha, next_t);
                last = i0 + j;
                TK = T;
                if (stops) { done = true; break; }
                T = next_t;
            }
        }
        if (__syncthreads_and(done)) break;                                    // also: s_e is free again
    }
    if (last != 0xFFFFFFFFu) atomicMax(&s_kend, last + 1u);                  // entries at or after s_kend: zero rows
    __syncthreads();
    const uint32_t kend = s_kend > start ? s_kend : start;

    // 2. back to front over [start, kend)
    float4 gc = make_float4(0.f, 0.f, 0.f, 0.f);
    float gd = 0.0f;
    if (t.inside && last != 0xFFFFFFFFu) {
        gc = a.grad_rgba[(size_t)t.py * fp.width + t.px];
        if (a.pos) gd = a.grad_depth[(size_t)t.py * fp.width + t.px];
    }
    float Tcur = TK;                                  // T in front of the entry processed last (walking back)
    float Sr = 0.f, Sg = 0.f, Sb = 0.f, Sa = 0.f, Sz = 0.f;   // colour, alpha, depth behind it (divided by its T)
    for (uint32_t i1 = kend; i1 > start;) {
        const uint32_t i0 = i1 - start > (uint32_t)kBwdBatch ? i1 - (uint32_t)kBwdBatch : start;
        const uint32_t cnt = i1 - i0;
        stage_entries<true>(s_e, t, fp, a, a.pos, i0, cnt);
        __syncthreads();
        for (int j = (int)cnt - 1; j >= 0; --j) {
            const uint32_t i = i0 + (uint32_t)j;
            const float* e = s_e[j];
            float ex, ey, ef;
            bool contributes;
            const float alpha = entry_alpha(e, t, ex, ey, ef, contributes);
            contributes = contributes && last != 0xFFFFFFFFu && i <= last;
            float v[kPartFloats];
#pragma unroll
            for (int k = 0; k < kPartFloats; ++k) v[k] = 0.0f;
            if (contributes) {
                const float one_m = 1.0f - alpha;                              // the forward's own (1 - alpha)
                const float Ti = i == last ? TK : Tcur / one_m;                // T_{i+1} >= 1e-4 here: no early-out before K
                const float cr = e[kEntColour], cg = e[kEntColour + 1], cb = e[kEntColour + 2], z = e[kEntDepth];
                const float dalpha = Ti * (gc.x * (cr - Sr) + gc.y * (cg - Sg) + gc.z * (cb - Sb) + gc.w * (1.0f - Sa) +
                                           gd * (z - Sz));
                const float w = Ti * alpha;
                const float df = dalpha * alpha;                               // alpha = a * exp(f)
                const float ix = e[kEntIx], iy = e[kEntIy], iz = e[kEntIz];
                v[0] = df * (-(ix * ex) - iy * ey);                            // d f / d sx  (ex = sx - px)
                v[1] = df * (iz * ey + iy * ex);                               // d f / d sy  (ey = py - sy)
                v[2] = df * (-0.5f * ex * ex);
                v[3] = df * (-ex * ey);
                v[4] = df * (-0.5f * ey * ey);
                v[5] = gc.x * w; v[6] = gc.y * w; v[7] = gc.z * w;
                v[8] = dalpha * ef;
                v[9] = gd * w;
                if constexpr (ABS) { v[kRowFloats] = fabsf(v[0]); v[kRowFloats + 1] = fabsf(v[1]); }
                Sr = alpha * cr + one_m * Sr;
                Sg = alpha * cg + one_m * Sg;
                Sb = alpha * cb + one_m * Sb;
                Sa = alpha + one_m * Sa;
                Sz = alpha * z + one_m * Sz;
                Tcur = Ti;
            }
            // the wave's sum in a fixed butterfly (every lane ends with the same bits), then one lane parks it
            if (__ballot(contributes) != 0ull) {
#pragma unroll
                for (int k = 0; k < kPartFloats; ++k) v[k] = wave_tree(v[k], [](float x, float y) { return x + y; });
            }
            if (t.lane == 0) {
#pragma unroll
                for (int k = 0; k < kPartFloats; ++k) s_part[t.wave][j][k] = v[k];
            }
        }
        __syncthreads();
        // the four waves' sums -> the entry's row, in its slot
        for (uint32_t q = (uint32_t)t.tid; q < cnt * kPartFloats; q += 256u) {
            const uint32_t j = q / kPartFloats, k = q % kPartFloats;
            const uint32_t slot = __float_as_uint(s_e[j][kEntSlot<true>]);
            const float sum = ((s_part[0][j][k] + s_part[1][j][k]) + s_part[2][j][k]) + s_part[3][j][k];
            if constexpr (ABS) {
                if (slot != kNoSlot) {
                    if (k < (uint32_t)kRowFloats) a.rows[(size_t)slot * kRowFloats + k] = sum;
                    else a.abs_rows[(size_t)slot * kAbsRowFloats + (k - kRowFloats)] = sum;
                }
            } else {
                if (slot != kNoSlot) a.rows[(size_t)slot * kRowFloats + k] = sum;
            }
        }
        __syncthreads();
        i1 = i0;
    }
    // 3. entries no pixel of the tile reaches
    zero_rows<kRowFloats, kBwdBatch>(t, a, kend, a.rows);
    if constexpr (ABS) zero_rows<kAbsRowFloats, kBwdBatch>(t, a, kend, a.abs_rows);     // a stale pair must never be summed
}

static void launch_blend(const BackwardFrame& f, const float* grad_rgba, const float* grad_depth, hipStream_t stream) {
    const BwdBlendArgs args{{f.sc.raster, f.sorted_id, f.ranges, f.bb.scan.offsets, f.sc.extents, f.fp.capacity},
                            grad_depth ? f.scene.pos : nullptr, reinterpret_cast<const float4*>(grad_rgba), grad_depth, f.bb.rows};
    if (!f.fp.rows_owned) return;                     // an empty band: no tile, no element, no row
    if (f.bb.abs_rows)                                // the switch is on (backward_frame): the absolute pairs beside the rows
        hipLaunchKernelGGL(k_bwd_blend<true>, replay_grid(f.fp), dim3(256), 0, stream, f.fp, BwdBlendAbsArgs{args, f.bb.abs_rows});
    else
        hipLaunchKernelGGL(k_bwd_blend<false>, replay_grid(f.fp), dim3(256), 0, stream, f.fp, args);
}

// ---- per splat ----------------------------------------------------------------------------------------------------

// Row sum + chain.  Dense: thread g < N sums the rows of splat g and writes record gradient g (all zero for a splat outside
// V).  VIS: thread i < min(|V|, max_rows) does so for g = vis_ids[i] and writes record gradient i; the grid covers
// min(N, max_rows) (|V| lives on the device, in *vis_count) and the threads beyond the count leave.
template <bool VIS>
__global__ __launch_bounds__(256) void k_bwd_rowsum_chain(const FrameParams fp, const SceneBuffers scene,
                                                           const SplatCounts counts,
                                                           const uint32_t* __restrict__ offsets,
                                                           const float* __restrict__ rows,
                                                           const uint32_t* __restrict__ vis_ids,
                                                           const uint32_t* __restrict__ vis_count, uint32_t max_rows,
                                                           float* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t g = i;
    bool any = true;
    if constexpr (VIS) {
        const uint32_t count = *vis_count;
        if (i >= (count < max_rows ? count : max_rows)) return;
        g = vis_ids[i];
    } else {
        if (g >= fp.num_gaussians) return;
        any = counts.of(g) != 0u;
    }
    float row[kRowFloats];
    splat_row_sum(counts, offsets, rows, g, fp.capacity, row);
    bwd_chain<false>(fp, scene, g, any, row, reinterpret_cast<float4*>(out + (size_t)i * kRecordFloats), nullptr);
}

// gs_debug_read(GS_BUF_BACKWARD_ROWS): the row k_bwd_rowsum_chain handed bwd_chain for splat g (the same splat_row_sum, hence
// the same bits), as out[g][kRowFloats]; zeros for a splat that is not in the list.  Nothing of a backward launches it.
__global__ __launch_bounds__(256) void k_bwd_row_sums(uint32_t n, uint32_t capacity, const SplatCounts counts,
                                                       const uint32_t* __restrict__ offsets,
                                                       const float* __restrict__ rows, float* __restrict__ out) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n) return;
    float row[kRowFloats];
#pragma unroll
    for (int k = 0; k < kRowFloats; ++k) row[k] = 0.0f;
    if (counts.of(g) != 0u) splat_row_sum(counts, offsets, rows, g, capacity, row);
#pragma unroll
    for (int k = 0; k < kRowFloats; ++k) out[(size_t)g * kRowFloats + k] = row[k];
}

void launch_backward_row_sums(const BackwardFrame& f, float* out, hipStream_t stream) {
    const uint32_t n = f.fp.num_gaussians;
    hipLaunchKernelGGL(k_bwd_row_sums, dim3(backward_blocks(n)), dim3(256), 0, stream, n, f.fp.capacity,
                       splat_counts_of(f.sc, f.fp), f.bb.scan.offsets, f.bb.rows, out);
}

void launch_slot_offsets(const SplatCounts& counts, uint32_t n, const SplatScan& scan, hipStream_t stream) {
    launch_splat_scan(BwdSource<false>{counts, nullptr, nullptr, 0u}, n, scan, nullptr, stream);
}

void launch_backward(const BackwardFrame& f, const float* grad_rgba, const float* grad_depth, float* grad_records,
                     hipStream_t stream) {
    launch_slot_offsets(splat_counts_of(f.sc, f.fp), f.fp.num_gaussians, f.bb.scan, stream);
    launch_blend(f, grad_rgba, grad_depth, stream);
    hipLaunchKernelGGL(k_bwd_rowsum_chain<false>, dim3(backward_blocks(f.fp.num_gaussians)), dim3(256), 0, stream, f.fp,
                       f.scene, splat_counts_of(f.sc, f.fp), f.bb.scan.offsets, f.bb.rows, nullptr, nullptr, 0u, grad_records);
}

void launch_backward_visible_scan(const BackwardFrame& f, uint32_t* ids_out, uint32_t max_rows, uint32_t* count_out,
                                  hipStream_t stream) {
    launch_splat_scan(BwdSource<true>{splat_counts_of(f.sc, f.fp), f.bb.vis_ids, ids_out, max_rows}, f.fp.num_gaussians, f.bb.scan, count_out,
                      stream);
}

void launch_backward_visible_rows(const BackwardFrame& f, const float* grad_rgba, const float* grad_depth,
                                  uint32_t max_rows, float* grad_rows, hipStream_t stream) {
    const uint32_t n = f.fp.num_gaussians;
    launch_blend(f, grad_rgba, grad_depth, stream);
    hipLaunchKernelGGL(k_bwd_rowsum_chain<true>, dim3(backward_blocks(n < max_rows ? n : max_rows)), dim3(256), 0, stream,
                       f.fp, f.scene, splat_counts_of(f.sc, f.fp), f.bb.scan.offsets, f.bb.rows, f.bb.vis_ids, visible_count_of(f.bb),
                       max_rows, grad_rows);
}

} // namespace gs
