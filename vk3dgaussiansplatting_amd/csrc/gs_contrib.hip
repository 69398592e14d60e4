// gs_contrib.hip -- per-splat blend contributions of the last GS_RENDER_EXACT frame (gs_contrib_device, include/gsplat.h):
// for every splat the largest blend weight w = T * alpha it has in any pixel, the sum of its weights and the number of
// (pixel, list entry) pairs in which it adds its colour.  Two launches behind the per-splat slot offsets of gs_backward.hip
// (launch_slot_offsets: offset[g] + the tile's index in g's box = the slot of a list element):
//   k_contrib_blend  : per tile, the replay of gs_tile_replay.h (the staging, the entry test and the transmittance step
//                      k_bwd_blend calls too: the same entries contribute and each pixel stops on the same entry), one
//                      pass, no colour and no depth.  What this kernel adds: the 256 pixels' weights of a list entry are
//                      reduced on chip in a fixed tree, every entry across the wave, and stored as one 12-byte row
//                      {sum, max, count} in the slot of the entry, with plain stores; entries no pixel reaches get zero rows;
//   k_contrib_rowsum : per splat, its rows combined in slot order (= tile raster order inside its box) and accumulated into
//                      the caller's arrays; a splat without a pair touches none of them.
// The fixed order of the sum (restated by tests/host/contrib_ref.c): per entry e = ((W0 + W1) + W2) + W3, Ww the balanced
// tree over wave w's 64 lanes (lane = (ly & 3) * 16 + lx of pixel rows 4 w .. 4 w + 3; lanes 2 k and 2 k + 1 first, then
// adjacent pair sums), a lane that does not blend the entry adding +0.0f; per splat S = 0.0f, S = S + e in slot order.
// No float atomics: the three arrays are bitwise reproducible and depend on the sorted list and the pixels only.
#include "gs_tile_replay.h"

namespace gs {

constexpr int kContribBatch = 64;         // list entries staged per step of k_contrib_blend

namespace {

struct ContribBlendArgs : TileListArgs {
    uint32_t* rows;                 // [capacity][kContribRowWords]: sum (float bits), max (float bits), count
};

}  // namespace

// One 256-thread workgroup per owned tile, one pixel per lane: the replay of gs_tile_replay.h, every entry reduced over the wave
__global__ __launch_bounds__(256) void k_contrib_blend(const FrameParams fp, const ContribBlendArgs a) {
    __shared__ float s_e[kContribBatch][8];                           // staged entries, the prefix alone
    __shared__ uint32_t s_part[4][kContribBatch][kContribRowWords];   // per-wave sum, max, count of an entry

    const TilePixel t = tile_pixel(fp, a.ranges);
    const int tid = t.tid, lane = t.lane, wave = t.wave;
    const uint32_t end = t.end;

    float T = 1.0f;
    bool done = !t.inside;
    uint32_t i0 = t.start;
    for (; i0 < end; i0 += kContribBatch) {
        const uint32_t cnt = end - i0 < (uint32_t)kContribBatch ? end - i0 : (uint32_t)kContribBatch;
        stage_entries<false>(s_e, t, fp, a, nullptr, i0, cnt);
        __syncthreads();
        if (__ballot(!done) == 0ull) {                                 // the whole wave has stopped: zeros for the batch
            if ((uint32_t)lane < cnt) {
#pragma unroll
                for (int k = 0; k < kContribRowWords; ++k) s_part[wave][lane][k] = 0u;
            }
        } else {
            for (uint32_t j = 0; j < cnt; ++j) {
                float w = 0.0f;
                bool blends = false;
                if (!done) {
                    float ex, ey, ef, next_t;
                    const float alpha = entry_alpha(s_e[j], t, ex, ey, ef, blends);
                    if (blends) {
                        w = T * alpha;
                        if (transmittance_step(T, alpha, next_t)) done = true;
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
        // the four waves -> the entry's row, in its slot
        if ((uint32_t)tid < cnt) {
            const uint32_t slot = __float_as_uint(s_e[tid][kEntSlot<false>]);
            if (slot != kNoSlot) {
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
    // entries no pixel of the tile reaches
    zero_rows<kContribRowWords, kContribBatch>(t, a, i0, a.rows);
}

// Thread g < N combines the rows of splat g in slot order, over the slots below the capacity.  A splat that emits nothing
// in this frame (SplatCounts::of), lies past the capacity or has no pair leaves without a load or a store on the caller's arrays.
__global__ __launch_bounds__(256) void k_contrib_rowsum(uint32_t n, uint32_t capacity, const SplatCounts counts,
                                                         const uint32_t* __restrict__ offsets,
                                                         const uint32_t* __restrict__ rows, float* __restrict__ wmax,
                                                         float* __restrict__ wsum, uint32_t* __restrict__ pixels) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n) return;
    const uint64_t o = offsets[g];
    const uint64_t e = o + counts.of(g);
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
    const ContribBlendArgs args{{f.sc.raster, f.sorted_id, f.ranges, offsets, f.sc.extents, f.fp.capacity}, rows};
    if (!f.fp.rows_owned) return;                     // an empty band: no pair, nothing of the caller's is touched
    hipLaunchKernelGGL(k_contrib_blend, replay_grid(f.fp), dim3(256), 0, stream, f.fp, args);
    hipLaunchKernelGGL(k_contrib_rowsum, dim3(backward_blocks(f.fp.num_gaussians)), dim3(256), 0, stream, f.fp.num_gaussians,
                       f.fp.capacity, splat_counts_of(f.sc, f.fp), offsets, rows, wmax, wsum, pixels);
}

}  // namespace gs
