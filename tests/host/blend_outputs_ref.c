/*
 * blend_outputs_ref.c -- CPU restatement of RenderGaussians.comp:56-152 with the optional outputs of gs_set_outputs
 * (include/gsplat.h, GS_OUTPUT_*): the loop of gso_render (oracle/gs_oracle.c, render_impl) operand by operand, plus
 *   - T_end: the transmittance after the last entry whose colour was added (the early-out of :136-140 adds the colour,
 *     then leaves with nextT -- here T_end = nextT, so colour and alpha describe the same entries);
 *   - depth: sum T_i * alpha_i * z_i with z_i = -(viewMat * vec4(pos, 1)).z, blended like a fourth colour channel.
 * Test infrastructure only (tests/test_outputs_cpu.py compiles it with -O2 -ffp-contract=off against oracle/libgs_oracle.so
 * for gso_exp): the RGBA8 bytes it writes must equal gso_render's before its alpha and depth are trusted.
 */
#include <stdint.h>
#include <stdlib.h>

#include "gs_oracle.h"

static inline float clampf(float x, float lo, float hi) {   /* GLSL clamp = min(max(x, lo), hi), as gs_oracle.c */
    float t = x > lo ? x : lo;
    return t < hi ? t : hi;
}

/* GLSL `M * v`, M column-major: ((M[0]*v.x + M[1]*v.y) + M[2]*v.z) + M[3]*v.w */
static void mat4_mul_vec4(const float* m, const float v[4], float out[4]) {
    for (int r = 0; r < 4; ++r) {
        float acc = m[0 * 4 + r] * v[0];
        acc = acc + m[1 * 4 + r] * v[1];
        acc = acc + m[2 * 4 + r] * v[2];
        acc = acc + m[3 * 4 + r] * v[3];
        out[r] = acc;
    }
}

/* Common.glsl:80-89 */
static void screen_pos(const gso_params* p, const float pv[4], float* sx, float* sy) {
    float q[4];
    mat4_mul_vec4(p->proj, pv, q);
    float x = q[0] / q[3];
    float y = q[1] / q[3];
    y = -y;
    x = (x + 1.0f) * 0.5f;
    y = (y + 1.0f) * 0.5f;
    *sx = x * (float)p->width;
    *sy = y * (float)p->height;
}

/* rgba_out: [H][W][4] bytes, rgba32f_out: [H][W][4] floats, depth_out: [H][W] floats.  Only the tile rows
 * [row_begin, row_end) of p are written (the other pixels are left untouched), as gso_render does. */
void gsb_render_outputs(const gso_params* p, const float* aos, const float* color, const float* cov,
                        const uint32_t* sorted_id, const uint32_t* ranges, uint8_t* rgba_out, float* rgba32f_out,
                        float* depth_out) {
    const uint32_t ts = p->tile_size;
    const uint32_t grid_w = gso_num_tiles_x(p->width, ts);
    const uint32_t grid_h = gso_num_tiles_y(p->height, ts);
    const uint32_t row_end = p->row_end < grid_h ? p->row_end : grid_h;
    for (uint32_t ty = p->row_begin; ty < row_end; ++ty)
        for (uint32_t tx = 0; tx < grid_w; ++tx) {
            const uint32_t tile_index = ty * grid_w + tx;
            const uint32_t start = ranges[tile_index * 2 + 0];
            const uint32_t end = ranges[tile_index * 2 + 1];
            const uint32_t cnt = end > start ? end - start : 0;
            float* sd = (float*)malloc((size_t)(cnt ? cnt : 1) * 10 * sizeof(float));
            for (uint32_t k = 0; k < cnt; ++k) {
                const uint32_t gi = sorted_id[start + k];
                const float* rec = aos + (size_t)gi * GSO_FLOATS_PER_GAUSSIAN;
                float world[4] = {rec[0], rec[1], rec[2], 1.0f}, pv[4];
                mat4_mul_vec4(p->view, world, pv);
                float* o = sd + (size_t)k * 10;
                screen_pos(p, pv, &o[0], &o[1]);
                o[2] = color[(size_t)gi * 4 + 0];
                o[3] = color[(size_t)gi * 4 + 1];
                o[4] = color[(size_t)gi * 4 + 2];
                o[5] = color[(size_t)gi * 4 + 3];
                const float cx = cov[(size_t)gi * 4 + 0], cy = cov[(size_t)gi * 4 + 1], cz = cov[(size_t)gi * 4 + 2];
                const float det = cx * cz - cy * cy;
                if (det != 0.0f) {
                    const float det_inv = 1.0f / det;
                    o[6] = cz * det_inv;
                    o[7] = -cy * det_inv;
                    o[8] = cx * det_inv;
                } else {
                    o[6] = o[7] = o[8] = 0.0f;
                    o[5] = 0.0f;
                }
                o[9] = -pv[2];                                  /* z: what getDepthKey quantises */
            }
            for (uint32_t ly = 0; ly < ts; ++ly)
                for (uint32_t lx = 0; lx < ts; ++lx) {
                    const uint32_t px = tx * ts + lx, py = ty * ts + ly;
                    if (!(px < p->width && py < p->height)) continue;
                    float col[3] = {0.0f, 0.0f, 0.0f};
                    float d = 0.0f;
                    float Ti = 1.0f;
                    const float fpx = (float)px, fpy = (float)py;
                    for (uint32_t k = 0; k < cnt; ++k) {
                        const float* o = sd + (size_t)k * 10;
                        float ex_x = o[0] - fpx;
                        float ex_y = o[1] - fpy;
                        ex_y = -ex_y;
                        const float f = -0.5f * (o[6] * ex_x * ex_x + o[8] * ex_y * ex_y) - o[7] * ex_x * ex_y;
                        const float alpha = o[5] * gso_exp(f);
                        if (f > 0.0f || alpha < 1.0f / 255.0f) continue;
                        const float wgt = Ti * alpha;
                        col[0] = col[0] + wgt * o[2];
                        col[1] = col[1] + wgt * o[3];
                        col[2] = col[2] + wgt * o[4];
                        d = d + wgt * o[9];
                        const float next_t = Ti * (1.0f - alpha);
                        if (next_t < 0.0001f) { Ti = next_t; break; }   /* T_end of the early-out */
                        Ti = next_t;
                    }
                    const size_t pix = (size_t)py * p->width + px;
                    uint8_t* out = rgba_out + pix * 4;
                    for (int c = 0; c < 3; ++c) out[c] = (uint8_t)(clampf(col[c], 0.0f, 1.0f) * 255.0f + 0.5f);
                    out[3] = 255;
                    rgba32f_out[pix * 4 + 0] = col[0];
                    rgba32f_out[pix * 4 + 1] = col[1];
                    rgba32f_out[pix * 4 + 2] = col[2];
                    rgba32f_out[pix * 4 + 3] = 1.0f - Ti;
                    depth_out[pix] = d;
                }
            free(sd);
        }
}
