// gs_train.cpp -- the training calls of include/gsplat.h, which have no counterpart in the reference: Adam on listed rows,
// the raw parameter space, gs_backward*, gs_visible_count, gs_photometric_loss*, density control, pruning by contribution, the MCMC strategy, the rows of several views and a cloud from points.  Every entry point
// refuses first (nothing enqueued, the context unchanged), then enqueues on the context's stream; a host-pointer form is
// its _device twin between staging copies and a wait.
#include "gs_ctx.h"

#include <initializer_list>
#include <iterator>
#include <limits>

using namespace gs;

namespace {

// ---- the vocabulary of the refusals: every text is "<entry point>: <what>", who = the entry point's __func__

int refuse(gs_ctx* c, const std::string& who, const std::string& what, int code = GS_ERR_INVALID) {
    return fail(c, code, who + ": " + what);
}

// rows are listed (max_rows > 0) and one of the arrays that hold them is null; names: those arrays as the text lists them
int check_row_arrays(gs_ctx* c, const char* who, uint32_t max_rows, std::initializer_list<const void*> arrays, const char* names) {
    const bool missing = max_rows && std::find(arrays.begin(), arrays.end(), nullptr) != arrays.end();
    return missing ? refuse(c, who, std::string("null ") + names + " with max_rows > 0") : GS_OK;
}

// a gs_<kind>_params of another size than this library's
int check_struct_size(gs_ctx* c, const char* who, const char* kind, uint32_t struct_size, size_t expected) {
    if (struct_size == expected) return GS_OK;
    return refuse(c, who, std::string("gs_") + kind + "_params.struct_size does not match this library (call gs_default_" + kind + "_params first)");
}

// two arrays share at least one byte (a null or empty array shares nothing)
struct Span { const void* at; size_t bytes; };
bool overlap(const Span& a, const Span& b) {
    const uintptr_t a0 = (uintptr_t)a.at, b0 = (uintptr_t)b.at;
    return a.at && b.at && a.bytes && b.bytes && a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

// The context holds a whole frame: not sharded (that refusal ends in sharded_tail), `ready` (else not_ready), all tile rows
// -- or, with band_ok, the rows of a band whose caller has opted in (gs_set_band_gradients)
int check_whole_frame(gs_ctx* c, const char* who, const char* sharded_tail, bool ready = true, const char* not_ready = "",
                      bool band_ok = false) {
    if (c->dist_sharded) return refuse(c, who, std::string("a sharded context (gs_dist_shard_rows) ") + sharded_tail);
    if (!ready) return refuse(c, who, not_ready);
    const bool band = c->row_begin != 0u || c->row_end != c->grid_h || c->row_stride != 1u;
    if (band && !(band_ok && c->band_gradients))
        return refuse(c, who, "the context owns a subset of the tile rows");
    return GS_OK;
}

// ---- Adam

// what gs_adam_rows_device and gs_adam_rows_raw_device check of their parameters, and the step they hand the kernel
int adam_step_of(gs_ctx* c, const char* who, uint32_t n, const gs_adam_params* p, AdamStep& a) {
    if (!p) return refuse(c, who, "null gs_adam_params");
    if (n == 0) return refuse(c, who, "n is 0");
    if (int r = check_struct_size(c, who, "adam", p->struct_size, sizeof(gs_adam_params))) return r;
    if (p->step == 0) return refuse(c, who, "step counts from 1");
    if (!(p->beta1 >= 0.0f && p->beta1 < 1.0f) || !(p->beta2 >= 0.0f && p->beta2 < 1.0f))
        return refuse(c, who, "beta1 and beta2 must be in [0, 1)");
    if (!(p->eps >= 0.0f) || !std::isfinite(p->eps)) return refuse(c, who, "eps must be finite and not negative");
    a.beta1 = p->beta1; a.beta2 = p->beta2; a.eps = p->eps;
    a.c1 = 1.0f - p->beta1; a.c2 = 1.0f - p->beta2;
    // the bias correction of step t in double, rounded once per group
    const double t = (double)p->step;
    const double root2 = std::sqrt(1.0 - std::pow((double)p->beta2, t)), bias1 = 1.0 - std::pow((double)p->beta1, t);
    for (int g = 0; g < GS_ADAM_GROUPS; ++g) {
        if (!(p->lr[g] >= 0.0f) || !std::isfinite(p->lr[g])) return refuse(c, who, "lr must be finite and not negative");
        if (!(p->lo[g] <= p->hi[g])) return refuse(c, who, "lo must not exceed hi, and neither may be a NaN");
        a.step[g] = (float)((double)p->lr[g] * root2 / bias1);
        if (!std::isfinite(a.step[g])) return refuse(c, who, "lr times the bias correction is not a finite float");
        a.lo[g] = p->lo[g]; a.hi[g] = p->hi[g];
    }
    return GS_OK;
}

// ---- the raw parameter space (gs_raw.hip)

int convert_space(gs_ctx* c, const char* who, const float* src, float* dst, uint32_t n, bool to_raw) {
    if (!c) return GS_ERR_INVALID;
    if (!src || !dst) return refuse(c, who, "null raw or records");
    if (n == 0) return refuse(c, who, "n is 0");
    const size_t bytes = (size_t)n * GS_GAUSSIAN_RECORD_BYTES;
    if (overlap({src, bytes}, {dst, bytes})) return refuse(c, who, "raw aliases records");
    HIP_TRY(c, hipSetDevice(c->device));
    launch_convert_space(src, dst, n, to_raw, c->stream);
    return check_launch(c, who);
}

// ---- gs_backward*

// The buffers of a per-splat scan (gs_splat_scan.h) of K sums over n splats, into the lifetime `mem`
hipError_t alloc_splat_scan(DeviceOwner& mem, SplatScan& s, uint32_t n, uint32_t K) {
    const size_t rows = (size_t)K * backward_blocks(n) * sizeof(uint32_t);
    hipError_t e = mem.alloc(s.offsets, (size_t)n * sizeof(uint32_t));
    if (e == hipSuccess) e = mem.alloc(s.block_sums, rows);
    if (e == hipSuccess) e = mem.alloc(s.block_offsets, rows);
    if (e == hipSuccess) e = mem.alloc(s.totals, K * sizeof(uint32_t));
    return e;
}

// what gs_backward* and gs_contrib_device refuse of the context (nothing enqueued); band_ok: the call's result decomposes
// over the tile rows, so a band context with gs_set_band_gradients on is served
int backward_refusals(gs_ctx* c, const char* who, bool band_ok = true) {
    if (c->cfg.render_mode != GS_RENDER_EXACT) return refuse(c, who, "only GS_RENDER_EXACT frames can be differentiated");
    const bool frame = c->capacity && c->n && c->last.differentiable;
    const char* no_frame = "no frame since the last gs_set_resolution, gs_set_tile_rows* or upload";
    return check_whole_frame(c, who, "cannot be differentiated", frame, no_frame, band_ok);
}

// the refusals, then the scratch of the first call
int backward_prepare(gs_ctx* c, const char* who, bool band_ok = true) {
    if (int r = backward_refusals(c, who, band_ok)) return r;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->bwd.rows) {
        DeviceOwner& mem = c->bwd_mem;
        hipError_t e = mem.alloc(c->bwd.rows, backward_row_bytes(c->capacity));
        if (e == hipSuccess) e = alloc_splat_scan(mem, c->bwd.scan, c->n, 2);
        if (e == hipSuccess) e = mem.alloc(c->bwd.vis_ids, (size_t)c->n * sizeof(uint32_t));
        if (e != hipSuccess) {
            mem.release();
            c->bwd_vis_rows = 0;
            return refuse(c, who, hipGetErrorString(e), GS_ERR_HIP);
        }
    }
    return GS_OK;
}

// gs_set_abs_gradients is on and a gs_backward* form is about to run its blend: the pairs' scratch of the first such call
int abs_rows_prepare(gs_ctx* c, const char* who) {
    if (!c->abs_gradients || c->bwd.abs_rows) return GS_OK;
    const hipError_t e = c->bwd_mem.alloc(c->bwd.abs_rows, backward_abs_row_bytes(c->capacity));
    return e == hipSuccess ? GS_OK : refuse(c, who, hipGetErrorString(e), GS_ERR_HIP);
}

// The last frame as the backward launchers take it; bb.abs_rows only while the switch is on (launch_blend goes by it)
BackwardFrame backward_frame(const gs_ctx* c) {
    BackwardFrame f{c->last.fp, c->scene, c->scratch, c->sort.id[c->last.sorted_index], c->ranges, c->bwd};
    if (!c->abs_gradients) f.bb.abs_rows = nullptr;
    return f;
}

// Host gradients onto the device (bwd_host_in, allocated on first use), enqueued on the context's stream: the two host
// pointers are replaced by their device copies (a null grad_depth stays null)
int stage_host_grads(gs_ctx* c, const float*& grad_rgba32f, const float*& grad_depth) {
    const size_t px = (size_t)c->width * c->height;
    if (!c->bwd_host_in) HIP_TRY(c, c->bwd_mem.alloc(c->bwd_host_in, px * 5 * sizeof(float)));
    float* din = c->bwd_host_in;
    HIP_TRY(c, hipMemcpyAsync(din, grad_rgba32f, px * 4 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (grad_depth) HIP_TRY(c, hipMemcpyAsync(din + px * 4, grad_depth, px * sizeof(float), hipMemcpyHostToDevice, c->stream));
    grad_rgba32f = din;
    if (grad_depth) grad_depth = din + px * 4;
    return GS_OK;
}

// what gs_backward and gs_backward_device enqueue (device pointers)
int enqueue_backward(gs_ctx* c, const char* who, const float* grad_rgba32f, const float* grad_depth, float* grad_records) {
    launch_backward(backward_frame(c), grad_rgba32f, grad_depth, grad_records, c->stream);
    backward_ran(c);
    return check_launch(c, who);
}

// ... and both visible forms: the blend and the row sums of the first max_rows splats of V (which a scan has listed)
int enqueue_visible_rows(gs_ctx* c, const char* who, const float* grad_rgba32f, const float* grad_depth, uint32_t max_rows,
                         float* grad_rows) {
    launch_backward_visible_rows(backward_frame(c), grad_rgba32f, grad_depth, max_rows, grad_rows, c->stream);
    backward_ran(c);
    return check_launch(c, who);
}

// V of the last frame into bwd.vis_ids and |V| into *count, on the host: the scan, then a wait for the stream
int visible_count_sync(gs_ctx* c, const char* who, uint32_t* count) {
    launch_backward_visible_scan(backward_frame(c), nullptr, 0u, nullptr, c->stream);
    if (int r = check_launch(c, who)) return r;
    HIP_TRY(c, hipMemcpyAsync(count, visible_count_of(c->bwd), 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GS_OK;
}

// gs_backward_camera*: the refusals (nothing enqueued), then the scratch of the first call
int backward_camera_prepare(gs_ctx* c, const char* who, const float* grad_camera) {
    if (!grad_camera) return refuse(c, who, "null gradient pointer");
    if (int r = backward_prepare(c, who)) return r;
    if (!c->last.has_backward) return refuse(c, who, "no gs_backward* on this frame");
    if (!c->bwd_cam_partials) {
        const hipError_t e = c->bwd_mem.alloc(c->bwd_cam_partials, backward_camera_partial_bytes(c->n));
        if (e != hipSuccess) return refuse(c, who, hipGetErrorString(e), GS_ERR_HIP);
    }
    return GS_OK;
}

// what both forms enqueue (a device pointer)
int enqueue_backward_camera(gs_ctx* c, const char* who, float* grad_camera) {
    launch_backward_camera(backward_frame(c), c->bwd_cam_partials, grad_camera, c->stream);
    return check_launch(c, who);
}

int backward_visible_refusals(gs_ctx* c, const char* who, const float* grad_rgba32f, const uint32_t* ids_out,
                              const float* grad_rows_out, uint32_t max_rows, const uint32_t* count_out) {
    if (!grad_rgba32f) return refuse(c, who, "null gradient pointer");
    if (!count_out) return refuse(c, who, "null count_out");
    if (int r = check_row_arrays(c, who, max_rows, {ids_out, grad_rows_out}, "ids_out or grad_rows_out")) return r;
    if (int r = backward_prepare(c, who)) return r;
    return abs_rows_prepare(c, who);
}

// gs_abs_screen_gradient_device / gs_densify_stats_abs_device: what gs_densify_stats_device refuses of the context, in its
// order and words, then the blend that left the pairs
int abs_gradient_refusals(gs_ctx* c, const char* who, bool band_ok) {
    if (int r = backward_prepare(c, who, band_ok)) return r;
    if (!c->last.has_backward) return refuse(c, who, "no gs_backward* on this frame");
    if (!c->last.has_abs_backward) return refuse(c, who, "no gs_backward* on this frame with gs_set_abs_gradients on");
    return GS_OK;
}

AbsGradArgs abs_gradient_args(const gs_ctx* c, const uint32_t* ids, const uint32_t* count, uint32_t max_rows, float* out) {
    const FrameParams& fp = c->last.fp;
    return AbsGradArgs{ids, count, max_rows, c->n, splat_counts_of(c->scratch, fp), c->bwd.scan.offsets, c->bwd.abs_rows,
                       fp.capacity, fp.width, fp.height, out};
}

// ---- gs_photometric_loss*

// the refusals (nothing enqueued), the image the call reads (rgba32f, or the context's own GS_OUTPUT_RGBA32F buffer for
// NULL), then the scratch of the first call
int loss_prepare(gs_ctx* c, const char* who, const float*& rgba32f, const float* target_rgb, float lambda,
                 const float* bg, const float* loss_out, const float* grad_rgba32f) {
    if (!target_rgb || !loss_out) return refuse(c, who, "null target_rgb or loss_out");
    if (!(lambda >= 0.0f && lambda <= 1.0f)) return refuse(c, who, "lambda must be a finite value in [0, 1]");
    if (bg && !(std::isfinite(bg[0]) && std::isfinite(bg[1]) && std::isfinite(bg[2]))) return refuse(c, who, "bg must be finite");
    if (!c->capacity) return refuse(c, who, "gs_set_resolution not called");
    if (int r = check_whole_frame(c, who, "has no whole frame to compare")) return r;
    if (!rgba32f) {
        void* dev = nullptr;
        size_t size = 0;
        if (int r = output_buffer(c, GS_OUTPUT_RGBA32F, who, &dev, &size)) return r;
        if (!c->outputs_valid) return refuse(c, who, "no frame rendered since the outputs were enabled or resized");
        rgba32f = static_cast<const float*>(dev);
    }
    if (grad_rgba32f && grad_rgba32f == rgba32f) return refuse(c, who, "grad_rgba32f must not be the image it differentiates");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->loss.maps) {
        hipError_t e = c->loss_mem.alloc(c->loss.maps, loss_map_bytes(c->width, c->height));
        if (e == hipSuccess) e = c->loss_mem.alloc(c->loss.tile_sums, loss_tile_bytes(c->width, c->height));
        if (e != hipSuccess) {
            c->loss_mem.release();
            return refuse(c, who, hipGetErrorString(e), GS_ERR_HIP);
        }
    }
    return GS_OK;
}

// what both forms enqueue (device pointers; bg is a host value)
int enqueue_loss(gs_ctx* c, const char* who, const float* rgba32f, const float* target_rgb, float lambda, const float* bg,
                 float* loss_out, float* grad_rgba32f) {
    launch_photometric_loss(c->loss, rgba32f, target_rgb, lambda, bg, c->width, c->height, loss_out, grad_rgba32f, c->stream);
    return check_launch(c, who);
}

// ---- density control

// the scratch of gs_densify_device and gs_rows_collect_device for n splats, kept from call to call and grown when a larger cloud comes
int densify_scratch(gs_ctx* c, uint32_t n, const char* who) {
    if (c->densify_cap >= n) return GS_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // an earlier call may still be running on the old arrays
    DeviceOwner& mem = c->densify_mem;
    mem.release();
    c->densify_cap = 0;
    const hipError_t e = alloc_splat_scan(mem, c->densify_scan, n, 4);
    if (e != hipSuccess) {
        mem.release();
        return refuse(c, who, hipGetErrorString(e), GS_ERR_HIP);
    }
    c->densify_cap = n;
    return GS_OK;
}

// ---- MCMC (gs_mcmc.hip)

// the sampler's scratch of gs_relocate_device and gs_grow_device for n splats, kept from call to call and grown when a larger
// cloud comes; the two tables go up once per allocation
int mcmc_scratch(gs_ctx* c, uint32_t n, const char* who) {
    if (c->mcmc_cap >= n) return GS_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // an earlier call may still be running on the old arrays
    DeviceOwner& mem = c->mcmc_mem;
    mem.release();
    c->mcmc_cap = 0;
    McmcScratch& s = c->mcmc;
    const size_t blocks = backward_blocks(n);
    hipError_t e = mem.alloc(s.within, (size_t)n * sizeof(uint32_t));
    if (e == hipSuccess) e = mem.alloc(s.block_sums, blocks * sizeof(uint64_t));
    if (e == hipSuccess) e = mem.alloc(s.block_prefix, (blocks + 1) * sizeof(uint64_t));
    if (e == hipSuccess) e = mem.alloc(s.cnt, (size_t)n * sizeof(uint32_t));
    if (e == hipSuccess) e = mem.alloc(s.src_of, (size_t)n * sizeof(uint32_t));
    if (e == hipSuccess) e = mem.alloc(s.tables, kMcmcTableFloats * sizeof(float));
    if (e == hipSuccess) {
        float tables[kMcmcTableFloats];
        mcmc_fill_tables(tables);
        e = hipMemcpy(s.tables, tables, sizeof(tables), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        mem.release();
        return refuse(c, who, hipGetErrorString(e), GS_ERR_HIP);
    }
    c->mcmc_cap = n;
    return GS_OK;
}

// what gs_relocate_device and gs_grow_device check of the cloud and the threshold
int check_mcmc_cloud(gs_ctx* c, const char* who, const float* m, const float* v, uint32_t n, float min_opacity) {
    if (!m != !v) return refuse(c, who, "m and v must be given together or not at all");
    if (n == 0) return refuse(c, who, "n is 0");
    if (n >= 0x80000000u) return refuse(c, who, "n must be below 2^31 (the rows are counted in 32 bits)");
    if (!(min_opacity >= 0x1p-24f && min_opacity < 1.0f)) return refuse(c, who, "min_opacity must lie in [2^-24, 1)");
    return GS_OK;
}

// ---- a cloud from points (gs_init.hip)

// what both calls check of the points, in the header's order
int check_points(gs_ctx* c, const char* who, bool arrays, uint32_t n) {
    if (!arrays) return refuse(c, who, "null points, dist2_out or records_out");
    if (n < 4u) return refuse(c, who, "fewer than four points have no three neighbours");
    if (n >= 0x80000000u) return refuse(c, who, "n must be below 2^31");
    return GS_OK;
}

// the scratch of both calls for n points (45 bytes per point), kept from call to call and grown when a larger cloud comes
int init_scratch(gs_ctx* c, uint32_t n, const char* who) {
    if (c->init_cap >= n) return GS_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // an earlier call may still be running on the old arrays
    DeviceOwner& mem = c->init_mem;
    mem.release();
    c->init_cap = 0;
    InitScratch& s = c->init;
    const size_t boxes = ((size_t)n + 63u) / 64u;
    int rc = alloc_sort(c, mem, c->init_sort, n);
    hipError_t e = hipSuccess;
    if (rc == GS_OK) e = mem.alloc(s.partial, (size_t)kInitBoundBlocks * 6 * sizeof(float));
    if (rc == GS_OK && e == hipSuccess) e = mem.alloc(s.bounds, 6 * sizeof(float));
    if (rc == GS_OK && e == hipSuccess) e = mem.alloc(s.sorted, (size_t)n * sizeof(float4));
    if (rc == GS_OK && e == hipSuccess) e = mem.alloc(s.boxes, boxes * 2 * sizeof(float4));
    if (rc == GS_OK && e == hipSuccess) e = mem.alloc(s.dist2, (size_t)n * sizeof(float));
#ifdef GS_INIT_PROBE
    if (rc == GS_OK && e == hipSuccess) e = mem.alloc(s.probe, boxes * 2 * sizeof(uint32_t));
#endif
    if (rc == GS_OK && e != hipSuccess) rc = refuse(c, who, hipGetErrorString(e), GS_ERR_HIP);
    if (rc != GS_OK) { mem.release(); return rc; }
    c->init_cap = n;
    return GS_OK;
}

} // namespace

extern "C" {

void gs_default_init_params(gs_init_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(*p);
    p->opacity = 0.1f;
    p->min_dist2 = 1e-7f;
    p->max_scale = std::numeric_limits<float>::infinity();
}

int gs_knn_mean_dist2_device(gs_ctx* c, const float* points_dev, uint32_t n, float* dist2_out_dev) {
    if (!c) return GS_ERR_INVALID;
    if (int r = check_points(c, __func__, points_dev && dist2_out_dev, n)) return r;
    if (overlap({points_dev, (size_t)n * 12}, {dist2_out_dev, (size_t)n * 4})) return refuse(c, __func__, "dist2_out aliases points");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = init_scratch(c, n, __func__)) return r;
    if (launch_knn_mean_dist2(points_dev, n, c->init, c->init_sort, whole_list_run(c, n, 32u), dist2_out_dev, c->stream) < 0)
        return refuse(c, __func__, "the sorter refused the run", GS_ERR_HIP);
    return check_launch(c, __func__);
}

int gs_records_from_points_device(gs_ctx* c, const float* points_dev, const float* colors_dev, uint32_t n,
                                  const gs_init_params* p, float* records_out_dev, uint32_t* order_out_dev) {
    if (!c) return GS_ERR_INVALID;
    if (int r = check_points(c, __func__, points_dev && records_out_dev, n)) return r;
    if (!p) return refuse(c, __func__, "null gs_init_params");
    if (int r = check_struct_size(c, __func__, "init", p->struct_size, sizeof(gs_init_params))) return r;
    if (!(p->opacity > 0.0f && p->opacity < 1.0f)) return refuse(c, __func__, "opacity must lie strictly between 0 and 1");
    if (!(p->min_dist2 >= 0.0f) || !std::isfinite(p->min_dist2)) return refuse(c, __func__, "min_dist2 must be finite and not negative");
    if (!(p->max_scale > 0.0f)) return refuse(c, __func__, "max_scale must be greater than 0");
    // no output may share bytes with an input, or with the other output
    const Span ins[] = {{points_dev, (size_t)n * 12}, {colors_dev, (size_t)n * 12}};
    const Span outs[] = {{records_out_dev, (size_t)n * GS_GAUSSIAN_RECORD_BYTES}, {order_out_dev, (size_t)n * 4}};
    for (const Span& o : outs)
        for (const Span& i : ins)
            if (overlap(o, i)) return refuse(c, __func__, "an output array aliases an input");
    if (overlap(outs[0], outs[1])) return refuse(c, __func__, "two output arrays alias each other");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = init_scratch(c, n, __func__)) return r;
    if (launch_records_from_points(points_dev, colors_dev, n, c->init, c->init_sort, whole_list_run(c, n, 32u), p->opacity,
                                   p->min_dist2, p->max_scale, records_out_dev, order_out_dev, c->stream) < 0)
        return refuse(c, __func__, "the sorter refused the run", GS_ERR_HIP);
    return check_launch(c, __func__);
}

#ifdef GS_INIT_PROBE
// A tuning build only (tools/init_cost.py): the boxes that survived the coarse and the per-lane test of the last search,
// summed over its waves, and the milliseconds of the last call's six launches.  Waits for the stream.
int gs_init_probe_read(gs_ctx* c, uint32_t n, uint64_t* coarse_out, uint64_t* lane_out, float ms_out[6]) {
    if (!c || !c->init.probe || n > c->init_cap) return GS_ERR_INVALID;
    std::vector<uint32_t> h(((size_t)n + 63u) / 64u * 2);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, init_probe_ms(ms_out));
    HIP_TRY(c, hipMemcpy(h.data(), c->init.probe, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *coarse_out = *lane_out = 0;
    for (size_t i = 0; i < h.size(); i += 2) { *coarse_out += h[i]; *lane_out += h[i + 1]; }
    return GS_OK;
}
#endif

void gs_default_adam_params(gs_adam_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(*p);
    p->step = 1;
    p->beta1 = 0.9f; p->beta2 = 0.999f; p->eps = 1e-15f;
    const float inf = std::numeric_limits<float>::infinity();
    for (int g = 0; g < GS_ADAM_GROUPS; ++g) { p->lo[g] = -inf; p->hi[g] = inf; }
    p->lr[GS_ADAM_POSITION] = 1.6e-4f;
    p->lr[GS_ADAM_SCALE] = 5e-3f;     p->lo[GS_ADAM_SCALE] = 1e-7f;
    p->lr[GS_ADAM_ROTATION] = 1e-3f;
    p->lr[GS_ADAM_SH_DC] = 2.5e-3f;
    p->lr[GS_ADAM_OPACITY] = 5e-2f;   p->lo[GS_ADAM_OPACITY] = 0.0f; p->hi[GS_ADAM_OPACITY] = 1.0f;
    p->lr[GS_ADAM_SH_REST] = 1.25e-4f;
}

void gs_default_adam_params_raw(gs_adam_params* p) {
    if (!p) return;
    gs_default_adam_params(p);
    const float inf = std::numeric_limits<float>::infinity();
    for (int g = 0; g < GS_ADAM_GROUPS; ++g) { p->lo[g] = -inf; p->hi[g] = inf; }
}

int gs_adam_rows_device(gs_ctx* c, float* records_dev, float* m_dev, float* v_dev, uint32_t n, const uint32_t* ids_dev,
                        const float* grad_rows_dev, const uint32_t* count_dev, uint32_t max_rows, const gs_adam_params* p) {
    if (!c) return GS_ERR_INVALID;
    const char* rows = "records, m, v, ids, grad_rows or count";
    if (int r = check_row_arrays(c, __func__, max_rows, {records_dev, m_dev, v_dev, ids_dev, grad_rows_dev, count_dev}, rows)) return r;
    AdamStep a;
    if (int r = adam_step_of(c, __func__, n, p, a)) return r;
    if (!max_rows) return GS_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    launch_adam_rows(records_dev, m_dev, v_dev, n, ids_dev, grad_rows_dev, count_dev, max_rows, a, c->stream);
    return check_launch(c, __func__);
}

int gs_adam_rows_raw_device(gs_ctx* c, float* raw_dev, float* records_dev, float* m_dev, float* v_dev, uint32_t n,
                            const uint32_t* ids_dev, const float* grad_rows_dev, const uint32_t* count_dev, uint32_t max_rows,
                            const gs_adam_params* p) {
    if (!c) return GS_ERR_INVALID;
    const char* rows = "raw, records, m, v, ids, grad_rows or count";
    if (int r = check_row_arrays(c, __func__, max_rows, {raw_dev, records_dev, m_dev, v_dev, ids_dev, grad_rows_dev, count_dev}, rows)) return r;
    AdamStep a;
    if (int r = adam_step_of(c, __func__, n, p, a)) return r;
    const size_t bytes = (size_t)n * GS_GAUSSIAN_RECORD_BYTES;
    for (const float* other : {raw_dev, m_dev, v_dev})
        if (overlap({records_dev, bytes}, {other, bytes})) return refuse(c, __func__, "records aliases raw, m or v");
    if (!max_rows) return GS_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    launch_adam_rows_raw(raw_dev, records_dev, m_dev, v_dev, n, ids_dev, grad_rows_dev, count_dev, max_rows, a, c->stream);
    return check_launch(c, __func__);
}

int gs_records_from_raw_device(gs_ctx* c, const float* raw_dev, float* records_dev, uint32_t n) {
    return convert_space(c, "gs_records_from_raw_device", raw_dev, records_dev, n, false);
}

int gs_raw_from_records_device(gs_ctx* c, const float* records_dev, float* raw_dev, uint32_t n) {
    return convert_space(c, "gs_raw_from_records_device", records_dev, raw_dev, n, true);
}

int gs_reset_opacity_raw_device(gs_ctx* c, float* raw_dev, float* records_dev, float* m_dev, float* v_dev, uint32_t n,
                                float max_opacity) {
    if (!c) return GS_ERR_INVALID;
    if (!raw_dev || !records_dev) return refuse(c, __func__, "null raw or records");
    if (!m_dev != !v_dev) return refuse(c, __func__, "m and v must be given together or not at all");
    if (n == 0) return refuse(c, __func__, "n is 0");
    if (!(max_opacity > 0.0f && max_opacity < 1.0f)) return refuse(c, __func__, "max_opacity must lie strictly between 0 and 1");
    const float logit = (float)std::log((double)max_opacity / (1.0 - (double)max_opacity));
    HIP_TRY(c, hipSetDevice(c->device));
    launch_reset_opacity_raw(raw_dev, records_dev, m_dev, v_dev, n, max_opacity, logit, c->stream);
    return check_launch(c, __func__);
}

int gs_set_band_gradients(gs_ctx* c, uint32_t enable) {
    if (!c) return GS_ERR_INVALID;
    if (enable > 1u) return refuse(c, __func__, "enable must be 0 or 1");
    c->band_gradients = enable != 0u;
    return GS_OK;
}

// A host flag and nothing else: the last frame stays what it was (its FrameParams, flag included, are in c->last.fp, which is what
// gs_backward*, gs_backward_camera* and gs_contrib_device go by), and no captured graph holds a launch that reads the flag
// (enqueue_frame launches k_project directly)
int gs_set_antialias(gs_ctx* c, uint32_t enable) {
    if (!c) return GS_ERR_INVALID;
    if (enable > 1u) return refuse(c, __func__, "enable must be 0 or 1");
    c->antialias = enable != 0u;
    return GS_OK;
}

// A host flag and nothing else: what a gs_backward* form enqueues from now on.  The pairs a blend has left stay those of
// their frame (LastFrame::has_abs_backward); a frame is not touched.
int gs_set_abs_gradients(gs_ctx* c, uint32_t enable) {
    if (!c) return GS_ERR_INVALID;
    if (enable > 1u) return refuse(c, __func__, "enable must be 0 or 1");
    c->abs_gradients = enable != 0u;
    return GS_OK;
}

int gs_backward_device(gs_ctx* c, const float* grad_rgba32f, const float* grad_depth, float* grad_records) {
    if (!c) return GS_ERR_INVALID;
    if (!grad_rgba32f || !grad_records) return refuse(c, __func__, "null gradient pointer");
    if (int r = backward_prepare(c, __func__)) return r;
    if (int r = abs_rows_prepare(c, __func__)) return r;
    return enqueue_backward(c, __func__, grad_rgba32f, grad_depth, grad_records);
}

int gs_backward(gs_ctx* c, const float* grad_rgba32f, const float* grad_depth, float* grad_records) {
    if (!c) return GS_ERR_INVALID;
    if (!grad_rgba32f || !grad_records) return refuse(c, __func__, "null gradient pointer");
    if (int r = backward_prepare(c, __func__)) return r;
    if (int r = abs_rows_prepare(c, __func__)) return r;
    const size_t bytes = (size_t)c->n * GS_GAUSSIAN_RECORD_BYTES;
    if (!c->bwd_host_out) HIP_TRY(c, c->bwd_mem.alloc(c->bwd_host_out, bytes));
    if (int r = stage_host_grads(c, grad_rgba32f, grad_depth)) return r;
    if (int r = enqueue_backward(c, __func__, grad_rgba32f, grad_depth, c->bwd_host_out)) return r;
    HIP_TRY(c, hipMemcpyAsync(grad_records, c->bwd_host_out, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GS_OK;
}

int gs_photometric_loss_device(gs_ctx* c, const float* rgba32f, const float* target_rgb, float lambda, const float bg[3],
                               float* loss_out, float* grad_rgba32f) {
    if (!c) return GS_ERR_INVALID;
    if (int r = loss_prepare(c, __func__, rgba32f, target_rgb, lambda, bg, loss_out, grad_rgba32f)) return r;
    return enqueue_loss(c, __func__, rgba32f, target_rgb, lambda, bg, loss_out, grad_rgba32f);
}

int gs_photometric_loss(gs_ctx* c, const float* rgba32f, const float* target_rgb, float lambda, const float bg[3],
                        float loss_out[3], float* grad_rgba32f) {
    if (!c) return GS_ERR_INVALID;
    const float* image = rgba32f;      // host, or (NULL form) the context's device buffer after loss_prepare
    if (int r = loss_prepare(c, __func__, image, target_rgb, lambda, bg, loss_out, grad_rgba32f)) return r;
    // device copies: rgba [px][4] | gradient [px][4] | target [px][3] | the three numbers (+ 1: 16-byte multiples)
    const size_t px = (size_t)c->width * c->height;
    if (!c->loss_host) HIP_TRY(c, c->loss_mem.alloc(c->loss_host, (px * 11 + 4) * sizeof(float)));
    float* d_rgba = c->loss_host, *d_grad = d_rgba + px * 4, *d_target = d_grad + px * 4, *d_loss = d_target + px * 3;
    if (rgba32f) {
        HIP_TRY(c, hipMemcpyAsync(d_rgba, rgba32f, px * 4 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        image = d_rgba;
    }
    HIP_TRY(c, hipMemcpyAsync(d_target, target_rgb, px * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (int r = enqueue_loss(c, __func__, image, d_target, lambda, bg, d_loss, grad_rgba32f ? d_grad : nullptr)) return r;
    HIP_TRY(c, hipMemcpyAsync(loss_out, d_loss, 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (grad_rgba32f) HIP_TRY(c, hipMemcpyAsync(grad_rgba32f, d_grad, px * 4 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GS_OK;
}

int gs_visible_count(gs_ctx* c, uint32_t* count_out) {
    if (!c) return GS_ERR_INVALID;
    if (!count_out) return refuse(c, __func__, "null count_out");
    if (int r = backward_prepare(c, __func__)) return r;
    return visible_count_sync(c, __func__, count_out);
}

int gs_backward_visible_device(gs_ctx* c, const float* grad_rgba32f, const float* grad_depth, uint32_t* ids_out,
                               float* grad_rows_out, uint32_t max_rows, uint32_t* count_out) {
    if (!c) return GS_ERR_INVALID;
    if (int r = backward_visible_refusals(c, __func__, grad_rgba32f, ids_out, grad_rows_out, max_rows, count_out)) return r;
    launch_backward_visible_scan(backward_frame(c), ids_out, max_rows, count_out, c->stream);
    if (!max_rows) return check_launch(c, __func__);
    return enqueue_visible_rows(c, __func__, grad_rgba32f, grad_depth, max_rows, grad_rows_out);
}

int gs_backward_visible(gs_ctx* c, const float* grad_rgba32f, const float* grad_depth, uint32_t* ids_out,
                        float* grad_rows_out, uint32_t max_rows, uint32_t* count_out) {
    if (!c) return GS_ERR_INVALID;
    if (int r = backward_visible_refusals(c, __func__, grad_rgba32f, ids_out, grad_rows_out, max_rows, count_out)) return r;
    // V and its size first (the count has to reach the host anyway), then exactly min(|V|, max_rows) rows
    if (int r = visible_count_sync(c, __func__, count_out)) return r;
    const uint32_t count = *count_out, k = count < max_rows ? count : max_rows;
    if (k) {
        if (c->bwd_vis_rows < k) {
            c->bwd_mem.free(c->bwd_vis_out);
            c->bwd_vis_rows = 0;
            HIP_TRY(c, c->bwd_mem.alloc(c->bwd_vis_out, (size_t)k * GS_GAUSSIAN_RECORD_BYTES));
            c->bwd_vis_rows = k;
        }
        if (int r = stage_host_grads(c, grad_rgba32f, grad_depth)) return r;
        if (int r = enqueue_visible_rows(c, __func__, grad_rgba32f, grad_depth, k, c->bwd_vis_out)) return r;
        HIP_TRY(c, hipMemcpyAsync(ids_out, c->bwd.vis_ids, (size_t)k * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(grad_rows_out, c->bwd_vis_out, (size_t)k * GS_GAUSSIAN_RECORD_BYTES, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    const bool count_only = !max_rows && !ids_out && !grad_rows_out;      // asked for no row: none is missing
    return count > max_rows && !count_only ? GS_WARN_OVERFLOW : GS_OK;
}

int gs_backward_camera_device(gs_ctx* c, float* grad_camera_dev) {
    if (!c) return GS_ERR_INVALID;
    if (int r = backward_camera_prepare(c, __func__, grad_camera_dev)) return r;
    return enqueue_backward_camera(c, __func__, grad_camera_dev);
}

int gs_backward_camera(gs_ctx* c, float grad_camera[GS_CAMERA_GRAD_FLOATS]) {
    if (!c) return GS_ERR_INVALID;
    if (int r = backward_camera_prepare(c, __func__, grad_camera)) return r;
    const size_t bytes = GS_CAMERA_GRAD_FLOATS * sizeof(float);
    if (!c->bwd_cam_out) HIP_TRY(c, c->bwd_mem.alloc(c->bwd_cam_out, bytes));
    if (int r = enqueue_backward_camera(c, __func__, c->bwd_cam_out)) return r;
    HIP_TRY(c, hipMemcpyAsync(grad_camera, c->bwd_cam_out, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GS_OK;
}

int gs_contrib_device(gs_ctx* c, uint32_t n, float* wmax_dev, float* wsum_dev, uint32_t* pixels_dev) {
    if (!c) return GS_ERR_INVALID;
    if (!wmax_dev) return refuse(c, __func__, "null wmax");
    if (int r = backward_refusals(c, __func__)) return r;
    if (n != c->n) return refuse(c, __func__, "n differs from the scene's");
    HIP_TRY(c, hipSetDevice(c->device));
    // the slot offsets: the backward's scan where one exists (the same values), else a scan of this call's own
    const bool own_scan = !c->bwd.rows;
    DeviceOwner& mem = c->bwd_mem;
    hipError_t e = hipSuccess;
    if (!c->contrib_rows) e = mem.alloc(c->contrib_rows, contrib_row_bytes(c->capacity));
    if (e == hipSuccess && own_scan && !c->contrib_scan.totals) {
        e = alloc_splat_scan(mem, c->contrib_scan, c->n, 1);
        if (e != hipSuccess) {       // `totals` is allocated last: without it the next call starts over
            SplatScan& s = c->contrib_scan;
            mem.free(s.offsets); mem.free(s.block_sums); mem.free(s.block_offsets); mem.free(s.totals);
        }
    }
    if (e != hipSuccess) return refuse(c, __func__, hipGetErrorString(e), GS_ERR_HIP);
    const SplatScan& scan = own_scan ? c->contrib_scan : c->bwd.scan;
    launch_slot_offsets(splat_counts_of(c->scratch, c->last.fp), c->n, scan, c->stream);
    launch_contrib(backward_frame(c), scan.offsets, c->contrib_rows, wmax_dev, wsum_dev, pixels_dev, c->stream);
    return check_launch(c, __func__);
}

int gs_prune_below_device(gs_ctx* c, const float* score_dev, float threshold, uint32_t n, const float* records,
                          const float* raw, const float* m, const float* v, float* records_out, float* raw_out, float* m_out,
                          float* v_out, uint32_t max_out, uint32_t* counts_out_dev) {
    if (!c) return GS_ERR_INVALID;
    if (!score_dev || !records || !counts_out_dev) return refuse(c, __func__, "null score, records or counts_out");
    if (max_out && !records_out) return refuse(c, __func__, "null records_out with max_out > 0");
    if (n == 0) return refuse(c, __func__, "n is 0");
    if (n >= 0x80000000u) return refuse(c, __func__, "n must be below 2^31 (the outputs are counted in 32 bits)");
    if (threshold != threshold) return refuse(c, __func__, "threshold is a NaN");
    // with max_out == 0 no row is written and an output may stay away; an output without its input never
    const bool paired = (raw || !raw_out) && (m || !m_out) && (v || !v_out) &&
                        (!max_out || ((!raw || raw_out) && (!m || m_out) && (!v || v_out)));
    if (!paired) return refuse(c, __func__, "raw, m and v must each be null together with their own output");
    // no output may share bytes with an input, with the score or with another output
    const size_t in_bytes = (size_t)n * GS_GAUSSIAN_RECORD_BYTES, out_bytes = (size_t)max_out * GS_GAUSSIAN_RECORD_BYTES;
    const Span ins[] = {{records, in_bytes}, {raw, in_bytes}, {m, in_bytes}, {v, in_bytes}, {score_dev, (size_t)n * 4}};
    const Span outs[] = {{records_out, out_bytes}, {raw_out, out_bytes}, {m_out, out_bytes}, {v_out, out_bytes}, {counts_out_dev, 8}};
    for (const Span& o : outs)
        for (const Span& i : ins)
            if (overlap(o, i)) return refuse(c, __func__, "an output array aliases an input");
    for (size_t o = 0; o < std::size(outs); ++o)
        for (size_t k = o + 1; k < std::size(outs); ++k)
            if (overlap(outs[o], outs[k])) return refuse(c, __func__, "two output arrays alias each other");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = densify_scratch(c, n, __func__)) return r;
    // with max_out == 0 the writer is not launched: its pointers may be anything
    const PruneArgs a{score_dev, threshold, n, records, raw, m, v, records_out, raw_out, m_out, v_out, max_out, c->densify_scan};
    launch_prune_below(a, counts_out_dev, c->stream);
    return check_launch(c, __func__);
}

int gs_densify_stats_device(gs_ctx* c, const uint32_t* ids_dev, const uint32_t* count_dev, uint32_t max_rows, uint32_t n,
                            float* grad_accum, uint32_t* seen, float* max_radius) {
    if (!c) return GS_ERR_INVALID;
    const char* rows = "ids, count, grad_accum, seen or max_radius";
    if (int r = check_row_arrays(c, __func__, max_rows, {ids_dev, count_dev, grad_accum, seen, max_radius}, rows)) return r;
    if (int r = backward_prepare(c, __func__, false)) return r;      // a norm and a count per frame: no sum over bands
    if (!c->last.has_backward) return refuse(c, __func__, "no gs_backward* on this frame");
    if (n != c->n) return refuse(c, __func__, "n differs from the scene's");
    if (!max_rows) return GS_OK;
    const FrameParams& fp = c->last.fp;
    const DensifyStatsArgs a{ids_dev, count_dev, max_rows, n, splat_counts_of(c->scratch, c->last.fp), c->bwd.scan.offsets, c->bwd.rows,
                             c->scratch.raster, fp.capacity, fp.width, fp.height, grad_accum, seen, max_radius};
    launch_densify_stats(a, c->stream);
    return check_launch(c, __func__);
}

int gs_abs_screen_gradient_device(gs_ctx* c, const uint32_t* ids_dev, const uint32_t* count_dev, uint32_t max_rows,
                                  float* abs_out) {
    if (!c) return GS_ERR_INVALID;
    if (int r = check_row_arrays(c, __func__, max_rows, {ids_dev, count_dev, abs_out}, "ids, count or abs_out")) return r;
    if (int r = abs_gradient_refusals(c, __func__, true)) return r;      // a sum of absolute terms over pixels: it adds up over bands
    if (!max_rows) return GS_OK;
    launch_abs_screen_gradient(abs_gradient_args(c, ids_dev, count_dev, max_rows, abs_out), c->stream);
    return check_launch(c, __func__);
}

int gs_densify_stats_abs_device(gs_ctx* c, const uint32_t* ids_dev, const uint32_t* count_dev, uint32_t max_rows, uint32_t n,
                                float* grad_accum_abs) {
    if (!c) return GS_ERR_INVALID;
    if (int r = check_row_arrays(c, __func__, max_rows, {ids_dev, count_dev, grad_accum_abs}, "ids, count or grad_accum_abs")) return r;
    if (int r = abs_gradient_refusals(c, __func__, false)) return r;     // a norm per frame: no sum over bands
    if (n != c->n) return refuse(c, __func__, "n differs from the scene's");
    if (!max_rows) return GS_OK;
    launch_densify_stats_abs(abs_gradient_args(c, ids_dev, count_dev, max_rows, grad_accum_abs), c->stream);
    return check_launch(c, __func__);
}

int gs_rows_accumulate_device(gs_ctx* c, float* acc_dev, uint32_t* mark_dev, uint32_t n, const uint32_t* ids_dev,
                              const float* grad_rows_dev, const uint32_t* count_dev, uint32_t max_rows, float weight) {
    if (!c) return GS_ERR_INVALID;
    const char* rows = "acc, mark, ids, grad_rows or count";
    if (int r = check_row_arrays(c, __func__, max_rows, {acc_dev, mark_dev, ids_dev, grad_rows_dev, count_dev}, rows)) return r;
    if (n == 0) return refuse(c, __func__, "n is 0");
    if (!std::isfinite(weight)) return refuse(c, __func__, "weight must be finite");
    if (overlap({acc_dev, (size_t)n * GS_GAUSSIAN_RECORD_BYTES}, {grad_rows_dev, (size_t)max_rows * GS_GAUSSIAN_RECORD_BYTES}))
        return refuse(c, __func__, "acc aliases grad_rows");
    if (!max_rows) return GS_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    launch_rows_accumulate(acc_dev, mark_dev, n, ids_dev, grad_rows_dev, count_dev, max_rows, weight, c->stream);
    return check_launch(c, __func__);
}

int gs_rows_collect_device(gs_ctx* c, const float* acc_dev, uint32_t* mark_dev, uint32_t n, uint32_t* ids_out_dev,
                           float* rows_out_dev, uint32_t max_rows, uint32_t* count_out_dev) {
    if (!c) return GS_ERR_INVALID;
    if (!acc_dev || !mark_dev || !count_out_dev) return refuse(c, __func__, "null acc, mark or count_out");
    if (n == 0) return refuse(c, __func__, "n is 0");
    if (n >= 0x80000000u) return refuse(c, __func__, "n must be below 2^31 (the rows are counted in 32 bits)");
    if (int r = check_row_arrays(c, __func__, max_rows, {ids_out_dev, rows_out_dev}, "ids_out or rows_out")) return r;
    if (overlap({rows_out_dev, (size_t)max_rows * GS_GAUSSIAN_RECORD_BYTES}, {acc_dev, (size_t)n * GS_GAUSSIAN_RECORD_BYTES}))
        return refuse(c, __func__, "rows_out aliases acc");
    const Span marks{mark_dev, (size_t)n * 4};
    if (overlap({ids_out_dev, (size_t)max_rows * 4}, marks) || overlap({count_out_dev, 4}, marks))
        return refuse(c, __func__, "ids_out or count_out aliases mark");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = densify_scratch(c, n, __func__)) return r;
    launch_rows_collect(acc_dev, mark_dev, n, c->densify_scan, ids_out_dev, rows_out_dev, max_rows, count_out_dev, c->stream);
    return check_launch(c, __func__);
}

void gs_default_densify_params(gs_densify_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(*p);
    p->grad_threshold = 2e-4f;
    p->split_scale = 0.01f;
    p->prune_opacity = 0.005f;
    p->prune_scale = std::numeric_limits<float>::infinity();
    p->prune_radius = std::numeric_limits<float>::infinity();
    p->split_shrink = 1.6f;
    p->seed = 0;
}

int gs_densify_device(gs_ctx* c, const float* records, const float* m, const float* v, uint32_t n, const float* grad_accum,
                      const uint32_t* seen, const float* max_radius, const gs_densify_params* p, float* records_out,
                      float* m_out, float* v_out, uint32_t max_out, uint32_t* counts_out) {
    if (!c) return GS_ERR_INVALID;
    if (!records || !grad_accum || !seen || !max_radius || !counts_out)
        return refuse(c, __func__, "null records, grad_accum, seen, max_radius or counts_out");
    if (max_out && !records_out) return refuse(c, __func__, "null records_out with max_out > 0");
    if (!p) return refuse(c, __func__, "null gs_densify_params");
    if (n == 0) return refuse(c, __func__, "n is 0");
    if (n >= 0x80000000u) return refuse(c, __func__, "n must be below 2^31 (the outputs are counted in 32 bits)");
    if (int r = check_struct_size(c, __func__, "densify", p->struct_size, sizeof(gs_densify_params))) return r;
    if (p->grad_threshold != p->grad_threshold) return refuse(c, __func__, "grad_threshold is a NaN");
    if (!(p->split_shrink > 0.0f)) return refuse(c, __func__, "split_shrink must be greater than 0");
    const bool moments = m || v || m_out || v_out;
    if (moments && !(m && v && (!max_out || (m_out && v_out))))
        return refuse(c, __func__, "m, v, m_out and v_out must be given all together or not at all");
    // no output may share bytes with an input, or with another output
    const size_t in_bytes = (size_t)n * GS_GAUSSIAN_RECORD_BYTES, out_bytes = (size_t)max_out * GS_GAUSSIAN_RECORD_BYTES;
    const Span ins[] = {{records, in_bytes}, {m, in_bytes}, {v, in_bytes}, {grad_accum, (size_t)n * 4}, {seen, (size_t)n * 4},
                        {max_radius, (size_t)n * 4}};
    const Span outs[] = {{records_out, out_bytes}, {m_out, out_bytes}, {v_out, out_bytes}, {counts_out, 16}};
    for (const Span& o : outs)
        for (const Span& i : ins)
            if (overlap(o, i)) return refuse(c, __func__, "an output array aliases an input");
    for (size_t o = 0; o < std::size(outs); ++o)
        for (size_t k = o + 1; k < std::size(outs); ++k)
            if (overlap(outs[o], outs[k])) return refuse(c, __func__, "two output arrays alias each other");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = densify_scratch(c, n, __func__)) return r;
    DensifyArgs a{};
    a.records = records; a.m = m; a.v = v; a.n = n;
    a.grad_accum = grad_accum; a.seen = seen; a.max_radius = max_radius;
    a.rule = DensifyRule{p->grad_threshold, p->split_scale, p->prune_opacity, p->prune_scale, p->prune_radius};
    a.split_shrink = p->split_shrink; a.seed = p->seed;
    a.records_out = records_out; a.m_out = m_out; a.v_out = v_out; a.max_out = max_out;
    a.scan = c->densify_scan;
    launch_densify(a, counts_out, c->stream);
    return check_launch(c, __func__);
}

int gs_relocate_device(gs_ctx* c, float* records, float* raw, float* m, float* v, uint32_t n, float min_opacity, uint64_t seed,
                       uint32_t* ids_out, uint32_t max_rows, uint32_t* counts_out) {
    if (!c) return GS_ERR_INVALID;
    if (!records || !counts_out) return refuse(c, __func__, "null records or counts_out");
    if (int r = check_mcmc_cloud(c, __func__, m, v, n, min_opacity)) return r;
    if (int r = check_row_arrays(c, __func__, max_rows, {ids_out}, "ids_out")) return r;
    const size_t bytes = (size_t)n * GS_GAUSSIAN_RECORD_BYTES;
    const Span arrays[] = {{records, bytes}, {raw, bytes}, {m, bytes}, {v, bytes}, {ids_out, (size_t)max_rows * 4}, {counts_out, 12}};
    for (size_t a = 0; a < std::size(arrays); ++a)
        for (size_t b = a + 1; b < std::size(arrays); ++b)
            if (overlap(arrays[a], arrays[b])) return refuse(c, __func__, "two arrays alias each other");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = densify_scratch(c, n, __func__)) return r;
    if (int r = mcmc_scratch(c, n, __func__)) return r;
    const McmcArgs a{records, raw, m, v, n, min_opacity, seed, c->mcmc, c->densify_scan};
    launch_relocate(a, ids_out, max_rows, counts_out, c->stream);
    return check_launch(c, __func__);
}

int gs_grow_device(gs_ctx* c, const float* records, const float* raw, const float* m, const float* v, uint32_t n,
                   float min_opacity, uint64_t seed, uint32_t n_add, float* records_out, float* raw_out, float* m_out,
                   float* v_out, uint32_t max_out, uint32_t* counts_out) {
    if (!c) return GS_ERR_INVALID;
    if (!records || !counts_out) return refuse(c, __func__, "null records or counts_out");
    if (max_out && !records_out) return refuse(c, __func__, "null records_out with max_out > 0");
    // with max_out == 0 no row is written and an output may stay away; an output without its input never
    const bool paired = (raw || !raw_out) && (m || !m_out) && (v || !v_out) &&
                        (!max_out || ((!raw || raw_out) && (!m || m_out) && (!v || v_out)));
    if (!paired) return refuse(c, __func__, "raw, m and v must each be null together with their own output");
    if (int r = check_mcmc_cloud(c, __func__, m, v, n, min_opacity)) return r;
    if ((uint64_t)n + n_add >= 0x80000000ull) return refuse(c, __func__, "n + n_add must be below 2^31 (the outputs are counted in 32 bits)");
    // no output may share bytes with an input, or with another output
    const size_t in_bytes = (size_t)n * GS_GAUSSIAN_RECORD_BYTES, out_bytes = (size_t)max_out * GS_GAUSSIAN_RECORD_BYTES;
    const Span ins[] = {{records, in_bytes}, {raw, in_bytes}, {m, in_bytes}, {v, in_bytes}};
    const Span outs[] = {{records_out, out_bytes}, {raw_out, out_bytes}, {m_out, out_bytes}, {v_out, out_bytes}, {counts_out, 8}};
    for (const Span& o : outs)
        for (const Span& i : ins)
            if (overlap(o, i)) return refuse(c, __func__, "an output array aliases an input");
    for (size_t o = 0; o < std::size(outs); ++o)
        for (size_t k = o + 1; k < std::size(outs); ++k)
            if (overlap(outs[o], outs[k])) return refuse(c, __func__, "two output arrays alias each other");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = densify_scratch(c, n, __func__)) return r;
    if (int r = mcmc_scratch(c, n, __func__)) return r;
    // the kernels only read the inputs: one argument struct serves both calls
    const McmcArgs a{const_cast<float*>(records), const_cast<float*>(raw), const_cast<float*>(m), const_cast<float*>(v), n,
                     min_opacity, seed, c->mcmc, c->densify_scan};
    launch_grow(a, n_add, records_out, raw_out, m_out, v_out, max_out, counts_out, c->stream);
    return check_launch(c, __func__);
}

int gs_position_noise_device(gs_ctx* c, float* records, float* raw, uint32_t n, const uint32_t* ids, const uint32_t* count_dev,
                             uint32_t max_rows, float scale, float gate_k, float gate_x0, uint64_t seed) {
    if (!c) return GS_ERR_INVALID;
    if (!records) return refuse(c, __func__, "null records");
    if (n == 0) return refuse(c, __func__, "n is 0");
    if (!std::isfinite(scale) || !std::isfinite(gate_k) || !std::isfinite(gate_x0))
        return refuse(c, __func__, "scale, gate_k and gate_x0 must be finite");
    if (ids && max_rows && !count_dev) return refuse(c, __func__, "null count with ids and max_rows > 0");
    if (ids && !max_rows) return GS_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    launch_position_noise(records, raw, n, ids, count_dev, max_rows, scale, gate_k, gate_x0, seed, c->stream);
    return check_launch(c, __func__);
}

} // extern "C"
