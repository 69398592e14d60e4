/*
 * blend_outputs_ref.c -- CPU restatement of RenderGaussians.comp:56-152 with the optional outputs of gs_set_outputs
 * (include/gsplat.h, GS_OUTPUT_*): the loop of gso_render (oracle/gs_oracle.c, render_impl) operand by operand, plus
 *   - T_end: the transmittance after the last entry whose colour was added (the early-out of :136-140 adds the colour,
 *     then leaves with nextT -- here T_end = nextT, so colour and alpha describe the same entries);
 *   - depth: sum T_i * alpha_i * z_i with z_i = -(viewMat * vec4(pos, 1)).z, blended like a fourth colour channel.
 * Test infrastructure only (tests/test_outputs_cpu.py compiles it with -O2 -ffp-contract=off against oracle/libgs_oracle.so
 * for gso_exp): the RGBA8 bytes it writes must equal gso_render's before its alpha and depth are trusted.
 */
#include "blend_walk_ref.h"

static inline float clampf(float x, float lo, float hi) {   /* GLSL clamp = min(max(x, lo), hi), as gs_oracle.c */
    float t = x > lo ? x : lo;
    return t < hi ? t : hi;
}

typedef struct {
    uint32_t width;
    uint8_t* rgba;
    float *rgba32f, *depth;
    float col[3], d;                /* the pixel under way */
} outputs_ctx;

static inline void outputs_pair(void* ctx, uint32_t e, uint32_t lx, uint32_t ly, const float* o, float wgt, float alpha,
                                float next_t, int stops) {
    outputs_ctx* c = (outputs_ctx*)ctx;
    (void)e; (void)lx; (void)ly; (void)alpha; (void)next_t; (void)stops;
    c->col[0] = c->col[0] + wgt * o[GSB_R];
    c->col[1] = c->col[1] + wgt * o[GSB_G];
    c->col[2] = c->col[2] + wgt * o[GSB_B];
    c->d = c->d + wgt * o[GSB_Z];
}

static inline void outputs_pixel(void* ctx, uint32_t px, uint32_t py, float t_end) {
    outputs_ctx* c = (outputs_ctx*)ctx;
    const size_t pix = (size_t)py * c->width + px;
    uint8_t* out = c->rgba + pix * 4;
    for (int k = 0; k < 3; ++k) out[k] = (uint8_t)(clampf(c->col[k], 0.0f, 1.0f) * 255.0f + 0.5f);
    out[3] = 255;
    c->rgba32f[pix * 4 + 0] = c->col[0];
    c->rgba32f[pix * 4 + 1] = c->col[1];
    c->rgba32f[pix * 4 + 2] = c->col[2];
    c->rgba32f[pix * 4 + 3] = 1.0f - t_end;
    c->depth[pix] = c->d;
    c->col[0] = c->col[1] = c->col[2] = c->d = 0.0f;    /* the next pixel starts from zero */
}

/* rgba_out: [H][W][4] bytes, rgba32f_out: [H][W][4] floats, depth_out: [H][W] floats.  Only the tile rows
 * [row_begin, row_end) of p are written (the other pixels are left untouched), as gso_render does. */
void gsb_render_outputs(const gso_params* p, const float* aos, const float* color, const float* cov,
                        const uint32_t* sorted_id, const uint32_t* ranges, uint8_t* rgba_out, float* rgba32f_out,
                        float* depth_out) {
    const uint32_t grid_h = gso_num_tiles_y(p->height, p->tile_size);
    outputs_ctx c = {p->width, rgba_out, rgba32f_out, depth_out, {0.0f, 0.0f, 0.0f}, 0.0f};
    gsb_blend_walk(p, aos, color, cov, sorted_id, ranges, p->row_begin, p->row_end < grid_h ? p->row_end : grid_h, outputs_pair,
                   outputs_pixel, &c);
}
