/*
 * blend_trace_ref.c -- which list entries every pixel of an EXACT frame blends: the loop of blend_outputs_ref.c (the
 * restatement of RenderGaussians.comp:112-142 that reproduces the oracle's frame byte for byte) with its per-entry
 * decisions written out instead of the colour.  Test infrastructure only: tests/test_backward_cpu.py holds these
 * decisions fixed in its float64 restatement of the frame (the `f > 0 || alpha < 1/255` skip and the nextT < 1e-4
 * early-out are the discrete part of the frame the backward differentiates around).
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

/* flags: [E][256], flags[e * 256 + ly * 16 + lx] = 1 when entry e (of its tile's range) adds its colour to the pixel
 * (lx, ly) of the tile, 2 when it does and the pixel stops on it (nextT < 1e-4); 0 otherwise (also for the entries after
 * the pixel's early-out and for pixels outside the frame). */
void gsb_blend_trace(const gso_params* p, const float* aos, const float* color, const float* cov, const uint32_t* sorted_id,
                     const uint32_t* ranges, uint8_t* flags) {
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
                        const float next_t = Ti * (1.0f - alpha);
                        flags[(size_t)(start + k) * 256u + ly * 16u + lx] = next_t < 0.0001f ? 2 : 1;
                        if (next_t < 0.0001f) break;
                        Ti = next_t;
                    }
                }
            free(sd);
        }
}
