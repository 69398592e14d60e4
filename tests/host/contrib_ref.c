/*
 * contrib_ref.c -- CPU restatement of gs_contrib_device (include/gsplat.h): the blend weights w = T * alpha of an EXACT
 * frame per (list entry, tile pixel), and their per-splat maximum, sum and count in the header's fixed order.
 *   gsb_contrib_weights: the loop of blend_outputs_ref.c (the restatement of RenderGaussians.comp:112-142 that reproduces
 *     the oracle's frame byte for byte) with `wgt` written out instead of blended: w[e * 256 + ly * 16 + lx], 0 where the
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
#include <stdint.h>
#include <stdlib.h>

#include "gs_oracle.h"

static void mat4_mul_vec4(const float* m, const float v[4], float out[4]) {
    for (int r = 0; r < 4; ++r) {
        float acc = m[0 * 4 + r] * v[0];
        acc = acc + m[1 * 4 + r] * v[1];
        acc = acc + m[2 * 4 + r] * v[2];
        acc = acc + m[3 * 4 + r] * v[3];
        out[r] = acc;
    }
}

/* w: [E][256] floats, zero on entry */
void gsb_contrib_weights(const gso_params* p, const float* aos, const float* color, const float* cov,
                         const uint32_t* sorted_id, const uint32_t* ranges, float* w) {
    const uint32_t ts = p->tile_size;
    const uint32_t grid_w = gso_num_tiles_x(p->width, ts);
    const uint32_t grid_h = gso_num_tiles_y(p->height, ts);
    for (uint32_t ty = 0; ty < grid_h; ++ty)
        for (uint32_t tx = 0; tx < grid_w; ++tx) {
            const uint32_t tile_index = ty * grid_w + tx;
            const uint32_t start = ranges[tile_index * 2 + 0];
            const uint32_t end = ranges[tile_index * 2 + 1];
            const uint32_t cnt = end > start ? end - start : 0;
            float* sd = (float*)malloc((size_t)(cnt ? cnt : 1) * 6 * sizeof(float));
            for (uint32_t k = 0; k < cnt; ++k) {
                const uint32_t gi = sorted_id[start + k];
                const float* rec = aos + (size_t)gi * GSO_FLOATS_PER_GAUSSIAN;
                float world[4] = {rec[0], rec[1], rec[2], 1.0f}, pv[4], q[4];
                mat4_mul_vec4(p->view, world, pv);
                mat4_mul_vec4(p->proj, pv, q);
                float x = q[0] / q[3], y = q[1] / q[3];
                y = -y;
                x = (x + 1.0f) * 0.5f;
                y = (y + 1.0f) * 0.5f;
                float* o = sd + (size_t)k * 6;
                o[0] = x * (float)p->width;
                o[1] = y * (float)p->height;
                o[2] = color[(size_t)gi * 4 + 3];
                const float cx = cov[(size_t)gi * 4 + 0], cy = cov[(size_t)gi * 4 + 1], cz = cov[(size_t)gi * 4 + 2];
                const float det = cx * cz - cy * cy;
                if (det != 0.0f) {
                    const float det_inv = 1.0f / det;
                    o[3] = cz * det_inv;
                    o[4] = -cy * det_inv;
                    o[5] = cx * det_inv;
                } else {
                    o[3] = o[4] = o[5] = 0.0f;
                    o[2] = 0.0f;
                }
            }
            for (uint32_t ly = 0; ly < ts; ++ly)
                for (uint32_t lx = 0; lx < ts; ++lx) {
                    const uint32_t px = tx * ts + lx, py = ty * ts + ly;
                    if (!(px < p->width && py < p->height)) continue;
                    float Ti = 1.0f;
                    const float fpx = (float)px, fpy = (float)py;
                    for (uint32_t k = 0; k < cnt; ++k) {
                        const float* o = sd + (size_t)k * 6;
                        float ex_x = o[0] - fpx;
                        float ex_y = o[1] - fpy;
                        ex_y = -ex_y;
                        const float f = -0.5f * (o[3] * ex_x * ex_x + o[5] * ex_y * ex_y) - o[4] * ex_x * ex_y;
                        const float alpha = o[2] * gso_exp(f);
                        if (f > 0.0f || alpha < 1.0f / 255.0f) continue;
                        const float wgt = Ti * alpha;
                        w[(size_t)(start + k) * 256u + ly * 16u + lx] = wgt;
                        const float next_t = Ti * (1.0f - alpha);
                        if (next_t < 0.0001f) break;
                        Ti = next_t;
                    }
                }
            free(sd);
        }
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
