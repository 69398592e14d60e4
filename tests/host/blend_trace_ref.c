/*
 * blend_trace_ref.c -- which list entries every pixel of an EXACT frame blends: the walk of blend_walk_ref.h (the
 * restatement of RenderGaussians.comp:112-142 that, as blend_outputs_ref.c, reproduces the oracle's frame byte for byte)
 * with its per-entry decisions written out instead of the colour.  Test infrastructure only: tests/test_backward_cpu.py
 * holds these decisions fixed in its float64 restatement of the frame (the `f > 0 || alpha < 1/255` skip and the
 * nextT < 1e-4 early-out are the discrete part of the frame the backward differentiates around).
 */
#include "blend_walk_ref.h"

static inline void trace_pair(void* ctx, uint32_t e, uint32_t lx, uint32_t ly, const float* o, float wgt, float alpha,
                              float next_t, int stops) {
    (void)o; (void)wgt; (void)alpha; (void)next_t;
    ((uint8_t*)ctx)[(size_t)e * 256u + ly * 16u + lx] = stops ? 2 : 1;
}

/* flags: [E][256], flags[e * 256 + ly * 16 + lx] = 1 when entry e (of its tile's range) adds its colour to the pixel
 * (lx, ly) of the tile, 2 when it does and the pixel stops on it (nextT < 1e-4); 0 otherwise (also for the entries after
 * the pixel's early-out and for pixels outside the frame). */
void gsb_blend_trace(const gso_params* p, const float* aos, const float* color, const float* cov, const uint32_t* sorted_id,
                     const uint32_t* ranges, uint8_t* flags) {
    gsb_blend_walk(p, aos, color, cov, sorted_id, ranges, 0, gso_num_tiles_y(p->height, p->tile_size), trace_pair, NULL, flags);
}
