// gs_contrib.hip -- per-splat blend contributions of the last GS_RENDER_EXACT frame (gs_contrib_device, include/gsplat.h):
// for every splat the largest blend weight w = T * alpha it has in any pixel, the sum of its weights and the number of
// (pixel, list entry) pairs in which it adds its colour.  Two launches behind the per-splat slot offsets of gs_backward.hip
// (launch_slot_offsets: offset[g] + the tile's index in g's box = the slot of a list element):
//   k_contrib_blend  : the first half of k_bwd_blend -- per tile, the blend of RenderGaussians.comp:112-142 replayed front to
//                      back in the EXACT arithmetic (same expressions, same pinned exp: the same entries contribute and each
//                      pixel stops on the same entry), one pass, no colour and no depth.  The 256 pixels' weights of a list
//                      entry are reduced on chip in a fixed tree and stored as one 12-byte row {sum, max, count} in the slot
//                      of the entry, with plain stores; entries no pixel reaches get zero rows;
//   k_contrib_rowsum : per splat, its rows combined in slot order (= tile raster order inside its box) and accumulated into
//                      the caller's arrays; a splat without a pair touches none of them.
// The fixed order of the sum (restated by tests/host/contrib_ref.c): per entry e = ((W0 + W1) + W2) + W3, Ww the balanced
// tree over wave w's 64 lanes (lane = (ly & 3) * 16 + lx of pixel rows 4 w .. 4 w + 3; lanes 2 k and 2 k + 1 first, then
// adjacent pair sums), a lane that does not blend the entry adding +0.0f; per splat S = 0.0f, S = S + e in slot order.
// No float atomics: the three arrays are bitwise reproducible and depend on the sorted list and the pixels only.
#include "gs_device_utils.h"
#include "gs_internal.h"

namespace gs {

constexpr int kContribBatch = 64;         // list entries staged per step of k_contrib_blend

namespace {

struct ContribBlendArgs {
    const SplatRaster* raster;
    const uint32_t* sorted_id;
    const uint32_t* ranges;
    const uint32_t* offsets;        // [N] slot offsets
    const uint2* extents;           // SplatScratch::extents
    uint32_t* rows;                 // [capacity][kContribRowWords]: sum (float bits), max (float bits), count
    uint32_t capacity;
};

// The value of another lane of the row of 16 by DPP (pure VALU, no LDS crossbar); every lane of the wave must be active
template <int CTRL>
__device__ __forceinline__ float row_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

// The six-level butterfly of the header's tree: lane l combines with lane l ^ 1, ^ 2, ^ 4, ^ 8 by DPP -- quad_perm [1,0,3,2] and
// [2,3,0,1], then row_half_mirror and row_mirror: once the lanes of a group of 4 (8) hold the same bits, the mirrored lane holds
// those of the group l ^ 4 (l ^ 8) lies in -- and with l ^ 16, ^ 32 by shuffles.  Both operands of every level are the same
// two values in either order, so every lane ends with the same bits.
template <class Op>
__device__ __forceinline__ float wave_tree(float v, Op op) {
    v = op(v, row_dpp<0xB1>(v));
    v = op(v, row_dpp<0x4E>(v));
    v = op(v, row_dpp<0x141>(v));
    v = op(v, row_dpp<0x140>(v));
    v = op(v, __shfl_xor(v, 16, 64));
    return op(v, __shfl_xor(v, 32, 64));
}

}  // namespace

// One 256-thread workgroup per tile, one pixel per lane (wave w: pixel rows 4 w .. 4 w + 3).
__global__ __launch_bounds__(256) void k_contrib_blend(const FrameParams fp, const ContribBlendArgs a) {
    // staged entries: sx, sy, ix, iy, iz, alpha0, slot (bits), -
    __shared__ float s_e[kContribBatch][8];
    __shared__ uint32_t s_part[4][kContribBatch][kContribRowWords];   // per-wave sum, max, count of an entry

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t tile = blockIdx.x;                                // a full grid: compact id == global id
    const uint32_t ty = tile / fp.grid_w, tx = tile % fp.grid_w;
    const uint32_t start = a.ranges[tile * 2 + 0], end = a.ranges[tile * 2 + 1];
    const uint32_t px = tx * kTile + (uint32_t)(tid & 15), py = ty * kTile + (uint32_t)(tid >> 4);
    const float fpx = (float)px, fpy = (float)py;

    // stages entries [i0, i0 + count) of the list into s_e (threads 0 .. count - 1)
    auto stage = [&](uint32_t i0, uint32_t count) {
        if ((uint32_t)tid < count) {
            const uint32_t gi = a.sorted_id[i0 + tid];
            const float4* rp = reinterpret_cast<const float4*>(a.raster + gi);
            const float4 r0 = rp[0], r1 = rp[1], r2 = rp[2];
            const uint2 ext = a.extents[gi];
            const uint32_t min_x = ext.x & 0xFFFFu, k0 = ext.x >> 16, max_x = ext.y & 0xFFFFu;
            const uint64_t slot = (uint64_t)a.offsets[gi] + (uint64_t)(ty - k0) * (max_x - min_x) + (tx - min_x);
            float* e = s_e[tid];
            e[0] = r0.x; e[1] = r0.y; e[2] = r0.z; e[3] = r0.w; e[4] = r1.x;
            e[5] = r2.x;
            e[6] = __uint_as_float(slot < a.capacity ? (uint32_t)slot : 0xFFFFFFFFu);
        }
    };

    float T = 1.0f;
    bool done = !(px < fp.width && py < fp.height);
    uint32_t i0 = start;
    for (; i0 < end; i0 += kContribBatch) {
        const uint32_t cnt = end - i0 < (uint32_t)kContribBatch ? end - i0 : (uint32_t)kContribBatch;
        stage(i0, cnt);
        __syncthreads();
        if (__ballot(!done) == 0ull) {                                 // the whole wave has stopped: zeros for the batch
            if ((uint32_t)lane < cnt) {
#pragma unroll
                for (int k = 0; k < kContribRowWords; ++k) s_part[wave][lane][k] = 0u;
            }
        } else {
            for (uint32_t j = 0; j < cnt; ++j) {
                const float* e = s_e[j];
                float w = 0.0f;
                bool blends = false;
                if (!done) {
                    // the entry's test and alpha, bit for bit those of the forward (k_bwd_blend's entry_alpha)
                    const float ex = e[0] - fpx;
                    const float ey = -(e[1] - fpy);
                    const float f = -0.5f * (e[2] * ex * ex + e[4] * ey * ey) - e[3] * ex * ey;
                    const float alpha = e[5] * exp_pinned_live(f);
                    blends = !(f > 0.0f) && !(alpha < 1.0f / 255.0f);
                    if (blends) {
                        w = T * alpha;
                        const float next_t = T * (1.0f - alpha);               // :133
                        if (next_t < 0.0001f) done = true;                     // :136-140, colour already added
                        T = next_t;
                    }
                }
                const uint64_t who = __ballot(blends);
                float sum = 0.0f, top = 0.0f;
                if (who != 0ull) {     // the wave's sum and maximum in a fixed butterfly (every lane ends with the same bits)
                    sum = wave_tree(w, [](float x, float y) { return x + y; });
                    top = wave_tree(w, [](float x, float y) { return maxf(x, y); });
                }
                if (lane == 0) {
                    s_part[wave][j][0] = __float_as_uint(sum);
                    s_part[wave][j][1] = __float_as_uint(top);
                    s_part[wave][j][2] = (uint32_t)__popcll(who);
                }
            }
        }
        __syncthreads();
        // the four waves in a fixed order -> the entry's row, in its slot
        if ((uint32_t)tid < cnt) {
            const uint32_t slot = __float_as_uint(s_e[tid][6]);
            if (slot != 0xFFFFFFFFu) {
                auto part = [&](int w, int k) { return __uint_as_float(s_part[w][tid][k]); };
                const float sum = ((part(0, 0) + part(1, 0)) + part(2, 0)) + part(3, 0);
                const float top = maxf(maxf(maxf(part(0, 1), part(1, 1)), part(2, 1)), part(3, 1));
                uint32_t* row = a.rows + (size_t)slot * kContribRowWords;
                row[0] = __float_as_uint(sum);
                row[1] = __float_as_uint(top);
                row[2] = s_part[0][tid][2] + s_part[1][tid][2] + s_part[2][tid][2] + s_part[3][tid][2];
            }
        }
        if (__syncthreads_and(done)) { i0 += kContribBatch; break; }           // also: s_e and s_part are free again
    }
    // entries no pixel of the tile reaches: zero rows
    for (; i0 < end; i0 += kContribBatch) {
        const uint32_t cnt = end - i0 < (uint32_t)kContribBatch ? end - i0 : (uint32_t)kContribBatch;
        if ((uint32_t)tid < cnt) {
            const uint32_t gi = a.sorted_id[i0 + tid];
            const uint2 ext = a.extents[gi];
            const uint32_t min_x = ext.x & 0xFFFFu, k0 = ext.x >> 16, max_x = ext.y & 0xFFFFu;
            const uint64_t slot = (uint64_t)a.offsets[gi] + (uint64_t)(ty - k0) * (max_x - min_x) + (tx - min_x);
            if (slot < a.capacity) {
                uint32_t* row = a.rows + (size_t)slot * kContribRowWords;
                row[0] = 0u; row[1] = 0u; row[2] = 0u;
            }
        }
    }
}

// Thread g < N combines the rows of splat g in slot order, over the slots below the capacity.  A splat that emits nothing,
// lies past the capacity or has no pair in the frame leaves without a load or a store on the caller's arrays.
__global__ __launch_bounds__(256) void k_contrib_rowsum(uint32_t n, uint32_t capacity, const uint32_t* __restrict__ touched,
                                                         const uint32_t* __restrict__ offsets,
                                                         const uint32_t* __restrict__ rows, float* __restrict__ wmax,
                                                         float* __restrict__ wsum, uint32_t* __restrict__ pixels) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n) return;
    const uint64_t o = offsets[g];
    const uint64_t e = o + touched[g];
    const uint64_t stop = e < capacity ? e : capacity;
    float S = 0.0f, M = 0.0f;
    uint64_t count = 0;
    for (uint64_t s = o; s < stop; ++s) {
        const uint32_t* r = rows + s * kContribRowWords;
        S = S + __uint_as_float(r[0]);
        M = maxf(M, __uint_as_float(r[1]));
        count += r[2];
    }
    if (count == 0) return;
    const float old = wmax[g];
    wmax[g] = M > old ? M : old;
    if (wsum) wsum[g] = wsum[g] + S;
    if (pixels) {
        const uint64_t sum = (uint64_t)pixels[g] + count;
        pixels[g] = sum < 0xFFFFFFFFull ? (uint32_t)sum : 0xFFFFFFFFu;
    }
}

void launch_contrib(const BackwardFrame& f, const uint32_t* offsets, uint32_t* rows, float* wmax, float* wsum,
                    uint32_t* pixels, hipStream_t stream) {
    const ContribBlendArgs args{f.sc.raster, f.sorted_id, f.ranges, offsets, f.sc.extents, rows, f.fp.capacity};
    hipLaunchKernelGGL(k_contrib_blend, dim3(f.fp.grid_w * f.fp.grid_h), dim3(256), 0, stream, f.fp, args);
    hipLaunchKernelGGL(k_contrib_rowsum, dim3(backward_blocks(f.fp.num_gaussians)), dim3(256), 0, stream, f.fp.num_gaussians,
                       f.fp.capacity, f.sc.tiles_touched, offsets, rows, wmax, wsum, pixels);
}

}  // namespace gs
