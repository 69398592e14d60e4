/*
 * contrib_ref.c -- CPU restatement of gs_contrib_device (include/gsplat.h): the blend weights w = T * alpha of an EXACT
 * frame per (list entry, tile pixel), and their per-splat maximum, sum and count in the header's fixed order.
 *   gsb_contrib_weights: the walk of blend_walk_ref.h (the restatement of RenderGaussians.comp:112-142 that, as
 *     blend_outputs_ref.c, reproduces the oracle's frame byte for byte) with `wgt` written out instead of blended:
 *     w[e * 256 + ly * 16 + lx], 0 where the
 *     pixel does not blend the entry (skipped, behind the pixel's stop, or a pixel outside the frame).
 *   gsb_contrib_reduce: per entry e = ((W0 + W1) + W2) + W3 with Ww the balanced tree over the 64 pixels of wave w (pixel
 *     rows 4 w .. 4 w + 3, lane = (ly & 3) * 16 + lx = tile pixel index - 64 w: lanes 2 k and 2 k + 1 first, then adjacent
 *     pair sums, six levels), the maximum and the count; per splat S = 0.0f, S = S + e over its list elements in slot
 *     order (slot = the splat's offset + the tile's raster index inside its box) below the capacity, accumulated into
 *     wmax / wsum / pixels as the header writes it.  A splat without a pair is not touched.
 * Test infrastructure only (tests/test_contrib_cpu.py compiles it with -O2 -ffp-contract=off against
 * oracle/libgs_oracle.so for gso_exp, and trusts it only after its weights rebuild the restatement's float colour bit for
 * bit and are non-zero exactly where blend_trace_ref.c flags).
 */
#include "blend_walk_ref.h"

static inline void weights_pair(void* ctx, uint32_t e, uint32_t lx, uint32_t ly, const float* o, float wgt, float alpha,
                                float next_t, int stops) {
    (void)o; (void)alpha; (void)next_t; (void)stops;
    ((float*)ctx)[(size_t)e * 256u + ly * 16u + lx] = wgt;
}

/* w: [E][256] floats, zero on entry */
void gsb_contrib_weights(const gso_params* p, const float* aos, const float* color, const float* cov,
                         const uint32_t* sorted_id, const uint32_t* ranges, float* w) {
    gsb_blend_walk(p, aos, color, cov, sorted_id, ranges, 0, gso_num_tiles_y(p->height, p->tile_size), weights_pair, NULL, w);
}

/* w: [E][256] of gsb_contrib_weights, flags: [E][256] of gsb_blend_trace (which pairs count: a weight may be any float);
 * slot: [E] the slot of every list entry; touched, offset: [n] per splat (tiles of its box, its first slot); entry_e,
 * entry_max: [E] floats and entry_count: [E] out; wmax, wsum: [n] floats and pixels: [n] in / out (wsum, pixels may be null). */
void gsb_contrib_reduce(const float* w, const uint8_t* flags, uint32_t E, const uint32_t* slot, uint32_t capacity, uint32_t n,
                        const uint32_t* touched, const uint64_t* offset, float* entry_e, float* entry_max,
                        uint32_t* entry_count, float* wmax, float* wsum, uint32_t* pixels) {
    int64_t* at = (int64_t*)malloc((size_t)(capacity ? capacity : 1) * sizeof(int64_t));      /* slot -> entry */
    for (uint32_t s = 0; s < capacity; ++s) at[s] = -1;
    for (uint32_t e = 0; e < E; ++e) {
        float W[4], top = 0.0f;
        uint32_t count = 0;
        for (int wave = 0; wave < 4; ++wave) {
            float a[64];
            for (int l = 0; l < 64; ++l) {
                const size_t i = (size_t)e * 256u + (size_t)wave * 64u + (size_t)l;
                a[l] = flags[i] ? w[i] : 0.0f;
                if (flags[i]) {
                    ++count;
                    top = a[l] > top ? a[l] : top;
                }
            }
            for (int width = 32; width >= 1; width >>= 1)
                for (int k = 0; k < width; ++k) a[k] = a[2 * k] + a[2 * k + 1];
            W[wave] = a[0];
        }
        entry_e[e] = ((W[0] + W[1]) + W[2]) + W[3];
        entry_max[e] = top;
        entry_count[e] = count;
        if (slot[e] < capacity) at[slot[e]] = (int64_t)e;
    }
    for (uint32_t g = 0; g < n; ++g) {
        const uint64_t o = offset[g], end = o + touched[g];
        const uint64_t stop = end < capacity ? end : capacity;
        float S = 0.0f, M = 0.0f;
        uint64_t count = 0;
        for (uint64_t s = o; s < stop; ++s) {
            if (at[s] < 0) continue;
            S = S + entry_e[at[s]];
            M = entry_max[at[s]] > M ? entry_max[at[s]] : M;
            count += entry_count[at[s]];
        }
        if (!count) continue;
        wmax[g] = M > wmax[g] ? M : wmax[g];
        if (wsum) wsum[g] = wsum[g] + S;
        if (pixels) {
            const uint64_t sum = (uint64_t)pixels[g] + count;
            pixels[g] = sum < 0xFFFFFFFFull ? (uint32_t)sum : 0xFFFFFFFFu;
        }
    }
    free(at);
}
