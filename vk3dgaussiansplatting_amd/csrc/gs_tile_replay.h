// gs_tile_replay.h -- what the kernels that replay the blend of a GS_RENDER_EXACT frame evaluate alike, each written once
// (device): k_bwd_blend of gs_backward.hip and k_contrib_blend of gs_contrib.hip.  One 256-thread workgroup per tile the
// context owns (the whole grid, or the tile rows of a band: replay_grid), one pixel per lane; the tile's list entries are
// staged in LDS a batch at a time and every pixel walks them
// front to back in the EXACT arithmetic of RenderGaussians.comp:112-142 (same expressions, same pinned exp), so a replay
// makes the forward's decision for every (entry, pixel) pair -- the entry contributes or not, the pixel stops on it or
// not -- because it calls the same functions.  What a kernel does with a pair, its loop over the batches and the row it
// stores in the entry's slot are its own.
#pragma once

#include "gs_device_utils.h"
#include "gs_internal.h"

namespace gs {

constexpr uint32_t kNoSlot = 0xFFFFFFFFu;   // entry_slot of a list element at or past the capacity: it has no row

// A staged entry: the common prefix, then with COLOUR the colour and the view depth, then the slot (bits)
enum : int { kEntSx, kEntSy, kEntIx, kEntIy, kEntIz, kEntAlpha0, kEntPrefix,
             kEntColour = kEntPrefix /* r, g, b */, kEntDepth = kEntColour + 3 };
template <bool COLOUR>
constexpr int kEntSlot = COLOUR ? kEntDepth + 1 : kEntPrefix;

// The frame's list and the per-splat slot offsets of gs_backward.hip (launch_slot_offsets)
struct TileListArgs {
    const SplatRaster* raster;
    const uint32_t* sorted_id;
    const uint32_t* ranges;
    const uint32_t* offsets;        // [N] slot offsets
    const uint2* extents;           // SplatScratch::extents
    uint32_t capacity;
};

// The workgroup's tile and this thread's pixel of it (wave w: pixel rows 4 w .. 4 w + 3).  A launch is replay_grid(fp):
// grid_w x rows_owned workgroups, dispatched in the raster order of the owned tiles.  Workgroup (x, k) takes column x of the
// k-th owned row, which is row first_row + k * row_stride of the grid (global_tile of gs_render.hip; the identity for a
// context that owns every row).  ranges[] and the pixels go by the row of the grid, the slot by k (SplatScratch::extents
// holds compact rows).  Two grid dimensions, not one divided by grid_w: the load of the tile's range, which everything
// waits for, then hangs on a multiply-add of kernel arguments instead of on the division (with it k_bwd_blend measured
// 2 % slower at config C, profiles/band_backward_cost.txt).
struct TilePixel {
    int tid, lane, wave;
    uint32_t tx, ty, start, end;    // the tile (ty: its row of the grid) and its range of the list
    uint32_t ky;                    // the row's index among the owned rows
    uint32_t px, py;
    bool inside;                    // the pixel lies in the frame
    float fpx, fpy;
};
inline dim3 replay_grid(const FrameParams& fp) { return dim3(fp.grid_w, fp.rows_owned); }   // rows_owned == 0 (an empty band): no launch
__device__ __forceinline__ TilePixel tile_pixel(const FrameParams& fp, const uint32_t* ranges) {
    TilePixel t;
    t.tid = threadIdx.x; t.lane = t.tid & 63; t.wave = t.tid >> 6;
    t.tx = blockIdx.x; t.ky = blockIdx.y;
    t.ty = fp.first_row + t.ky * fp.row_stride;
    const uint32_t tile = t.ty * fp.grid_w + t.tx;
    t.start = ranges[tile * 2 + 0]; t.end = ranges[tile * 2 + 1];
    t.px = t.tx * kTile + (uint32_t)(t.tid & 15); t.py = t.ty * kTile + (uint32_t)(t.tid >> 4);
    t.inside = t.px < fp.width && t.py < fp.height;
    t.fpx = (float)t.px; t.fpy = (float)t.py;
    return t;
}

// The slot of splat gi's list element in column tx of owned row ky: its offset + the tile's raster index inside its box
__device__ __forceinline__ uint32_t entry_slot(const uint32_t* offsets, const uint2* extents, uint32_t gi, uint32_t tx,
                                               uint32_t ky, uint32_t capacity) {
    const uint2 ext = extents[gi];
    const uint32_t min_x = ext.x & 0xFFFFu, k0 = ext.x >> 16, max_x = ext.y & 0xFFFFu;
    const uint64_t slot = (uint64_t)offsets[gi] + (uint64_t)(ky - k0) * (max_x - min_x) + (tx - min_x);
    return slot < capacity ? (uint32_t)slot : kNoSlot;
}

// Stages entries [i0, i0 + count) of the list into s_e (threads 0 .. count - 1).  COLOUR: the colour too, and with pos
// (SceneBuffers::pos; null without a depth gradient) the view depth, else 0
template <bool COLOUR, int WIDTH>
__device__ __forceinline__ void stage_entries(float (*s_e)[WIDTH], const TilePixel& t, const FrameParams& fp,
                                              const TileListArgs& a, const float* pos, uint32_t i0, uint32_t count) {
    static_assert(WIDTH > kEntSlot<COLOUR>, "the row holds the staged fields");
    if ((uint32_t)t.tid < count) {
        const uint32_t gi = a.sorted_id[i0 + t.tid];
        const float4* rp = reinterpret_cast<const float4*>(a.raster + gi);
        const float4 r0 = rp[0], r1 = rp[1], r2 = rp[2];
        float z = 0.0f;
        if (COLOUR && pos) {   // -viewSpacePos.z as k_project computes it (mat4_mul_vec4, row 2)
            const size_t n = fp.num_gaussians;
            float acc = fp.view[2] * pos[gi];
            acc = acc + fp.view[6] * pos[n + gi];
            acc = acc + fp.view[10] * pos[2 * n + gi];
            acc = acc + fp.view[14] * 1.0f;
            z = -acc;
        }
        const uint32_t slot = entry_slot(a.offsets, a.extents, gi, t.tx, t.ky, a.capacity);
        float* e = s_e[t.tid];
        e[kEntSx] = r0.x; e[kEntSy] = r0.y; e[kEntIx] = r0.z; e[kEntIy] = r0.w; e[kEntIz] = r1.x;
        e[kEntAlpha0] = r2.x;
        if constexpr (COLOUR) {
            e[kEntColour] = r1.y; e[kEntColour + 1] = r1.z; e[kEntColour + 2] = r1.w; e[kEntDepth] = z;
        }
        e[kEntSlot<COLOUR>] = __uint_as_float(slot);
    }
}

// The exponent of RenderGaussians.comp:119-123 in the operand order of k_render / blend_pair (contraction is off)
__device__ __forceinline__ float blend_exponent(float sx, float sy, float ix, float iy, float iz, float fpx, float fpy,
                                                float& ex, float& ey) {
    ex = sx - fpx;
    ey = -(sy - fpy);
    return -0.5f * (ix * ex * ex + iz * ey * ey) - iy * ex * ey;
}

// The entry's test and alpha at the pixel, bit for bit those of the forward: contributes = !(f > 0) && !(alpha < 1/255)
__device__ __forceinline__ float entry_alpha(const float* e, const TilePixel& t, float& ex, float& ey, float& expf_,
                                             bool& contributes) {
    const float f = blend_exponent(e[kEntSx], e[kEntSy], e[kEntIx], e[kEntIy], e[kEntIz], t.fpx, t.fpy, ex, ey);
    expf_ = exp_pinned_live(f);
    const float alpha = e[kEntAlpha0] * expf_;
    contributes = !(f > 0.0f) && !(alpha < 1.0f / 255.0f);
    return alpha;
}

// The transmittance behind a contributing entry (:133); true when the pixel stops on it (:136-140, colour already added)
__device__ __forceinline__ bool transmittance_step(float T, float alpha, float& next_t) {
    next_t = T * (1.0f - alpha);
    return next_t < 0.0001f;
}

// Entries [i0, end) of the tile, which no pixel reaches: zero rows of WORDS words, BATCH entries per step
template <int WORDS, int BATCH, class Word>
__device__ __forceinline__ void zero_rows(const TilePixel& t, const TileListArgs& a, uint32_t i0, Word* rows) {
    for (; i0 < t.end; i0 += BATCH) {
        const uint32_t cnt = t.end - i0 < (uint32_t)BATCH ? t.end - i0 : (uint32_t)BATCH;
        if ((uint32_t)t.tid < cnt) {
            const uint32_t slot = entry_slot(a.offsets, a.extents, a.sorted_id[i0 + t.tid], t.tx, t.ky, a.capacity);
            if (slot != kNoSlot) {
                Word* row = rows + (size_t)slot * WORDS;
#pragma unroll
                for (int k = 0; k < WORDS; ++k) row[k] = Word(0);
            }
        }
    }
}

} // namespace gs
