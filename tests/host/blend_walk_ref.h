/*
 * blend_walk_ref.h -- what the CPU restatements of the blend share (blend_outputs_ref.c, blend_trace_ref.c, contrib_ref.c):
 * the loop of gso_render (oracle/gs_oracle.c, render_impl; RenderGaussians.comp:56-152) operand by operand -- per tile the
 * staging of its list entries, per pixel the walk over them with the `f > 0 || alpha < 1/255` skip and the nextT < 1e-4
 * early-out -- with what is done with a blended (entry, pixel) pair left to a visitor.  blend_outputs_ref.c blends colour
 * and depth and must reproduce the oracle's RGBA8 frame byte for byte before anything that walks this loop is trusted.
 * Test infrastructure only; compiled with -O2 -ffp-contract=off against oracle/libgs_oracle.so for gso_exp.
 */
#ifndef BLEND_WALK_REF_H
#define BLEND_WALK_REF_H

#include <stdint.h>
#include <stdlib.h>

#include "gs_oracle.h"

/* GLSL `M * v`, M column-major: ((M[0]*v.x + M[1]*v.y) + M[2]*v.z) + M[3]*v.w */
static inline void mat4_mul_vec4(const float* m, const float v[4], float out[4]) {
    for (int r = 0; r < 4; ++r) {
        float acc = m[0 * 4 + r] * v[0];
        acc = acc + m[1 * 4 + r] * v[1];
        acc = acc + m[2 * 4 + r] * v[2];
        acc = acc + m[3 * 4 + r] * v[3];
        out[r] = acc;
    }
}

/* Common.glsl:80-89 */
static inline void screen_pos(const gso_params* p, const float pv[4], float* sx, float* sy) {
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

/* a staged entry: screen position, colour, opacity, inverse 2-D covariance, view depth */
enum { GSB_SX, GSB_SY, GSB_R, GSB_G, GSB_B, GSB_ALPHA0, GSB_IX, GSB_IY, GSB_IZ, GSB_Z, GSB_ENTRY_FLOATS };

static inline void gsb_stage_entry(const gso_params* p, const float* aos, const float* color, const float* cov, uint32_t gi,
                                   float* o) {
    const float* rec = aos + (size_t)gi * GSO_FLOATS_PER_GAUSSIAN;
    float world[4] = {rec[0], rec[1], rec[2], 1.0f}, pv[4];
    mat4_mul_vec4(p->view, world, pv);
    screen_pos(p, pv, &o[GSB_SX], &o[GSB_SY]);
    o[GSB_R] = color[(size_t)gi * 4 + 0];
    o[GSB_G] = color[(size_t)gi * 4 + 1];
    o[GSB_B] = color[(size_t)gi * 4 + 2];
    o[GSB_ALPHA0] = color[(size_t)gi * 4 + 3];
    const float cx = cov[(size_t)gi * 4 + 0], cy = cov[(size_t)gi * 4 + 1], cz = cov[(size_t)gi * 4 + 2];
    const float det = cx * cz - cy * cy;
    if (det != 0.0f) {
        const float det_inv = 1.0f / det;
        o[GSB_IX] = cz * det_inv;
        o[GSB_IY] = -cy * det_inv;
        o[GSB_IZ] = cx * det_inv;
    } else {
        o[GSB_IX] = o[GSB_IY] = o[GSB_IZ] = 0.0f;
        o[GSB_ALPHA0] = 0.0f;
    }
    o[GSB_Z] = -pv[2];                                  /* z: what getDepthKey quantises */
}

/* A pixel (lx, ly) of a tile blends list entry e (staged as o) with wgt = T * alpha and has next_t behind it; stops: the
 * early-out of :136-140 (the colour is added, then the pixel leaves with next_t). */
typedef void (*gsb_pair_fn)(void* ctx, uint32_t e, uint32_t lx, uint32_t ly, const float* o, float wgt, float alpha,
                            float next_t, int stops);
/* A pixel inside the frame is through its tile's list (or has stopped) with transmittance t_end; may be null. */
typedef void (*gsb_pixel_fn)(void* ctx, uint32_t px, uint32_t py, float t_end);

/* The tile rows [row_begin, row_end) of the grid */
static inline void gsb_blend_walk(const gso_params* p, const float* aos, const float* color, const float* cov,
                                  const uint32_t* sorted_id, const uint32_t* ranges, uint32_t row_begin, uint32_t row_end,
                                  gsb_pair_fn pair, gsb_pixel_fn pixel, void* ctx) {
    const uint32_t ts = p->tile_size;
    const uint32_t grid_w = gso_num_tiles_x(p->width, ts);
    for (uint32_t ty = row_begin; ty < row_end; ++ty)
        for (uint32_t tx = 0; tx < grid_w; ++tx) {
            const uint32_t tile_index = ty * grid_w + tx;
            const uint32_t start = ranges[tile_index * 2 + 0];
            const uint32_t end = ranges[tile_index * 2 + 1];
            const uint32_t cnt = end > start ? end - start : 0;
            float* sd = (float*)malloc((size_t)(cnt ? cnt : 1) * GSB_ENTRY_FLOATS * sizeof(float));
            for (uint32_t k = 0; k < cnt; ++k)
                gsb_stage_entry(p, aos, color, cov, sorted_id[start + k], sd + (size_t)k * GSB_ENTRY_FLOATS);
            for (uint32_t ly = 0; ly < ts; ++ly)
                for (uint32_t lx = 0; lx < ts; ++lx) {
                    const uint32_t px = tx * ts + lx, py = ty * ts + ly;
                    if (!(px < p->width && py < p->height)) continue;
                    float Ti = 1.0f;
                    const float fpx = (float)px, fpy = (float)py;
                    for (uint32_t k = 0; k < cnt; ++k) {
                        const float* o = sd + (size_t)k * GSB_ENTRY_FLOATS;
                        float ex_x = o[GSB_SX] - fpx;
                        float ex_y = o[GSB_SY] - fpy;
                        ex_y = -ex_y;
                        const float f = -0.5f * (o[GSB_IX] * ex_x * ex_x + o[GSB_IZ] * ex_y * ex_y) - o[GSB_IY] * ex_x * ex_y;
                        const float alpha = o[GSB_ALPHA0] * gso_exp(f);
                        if (f > 0.0f || alpha < 1.0f / 255.0f) continue;
                        const float wgt = Ti * alpha;
                        const float next_t = Ti * (1.0f - alpha);
                        const int stops = next_t < 0.0001f;
                        pair(ctx, start + k, lx, ly, o, wgt, alpha, next_t, stops);
                        Ti = next_t;                                    /* T_end of the early-out too */
                        if (stops) break;
                    }
                    if (pixel) pixel(ctx, px, py, Ti);
                }
            free(sd);
        }
}

#endif
