// gsplat.hpp -- header-only C++17 convenience layer over the C-ABI of gsplat.h, shaped like the
// reference's Renderer (Engine/Graphics/Renderer.h:154-161: init / initForScene / draw / cleanup) so
// that a maintainer of the reference can swap the class in.  No state beyond the
// gs_ctx handle; errors surface as status codes + lastError(), never as exceptions or aborts
// (the reference logs and continues, Engine/Dev/Log.cpp:40-43).
#pragma once

#include "gsplat.h"

#include <cstdint>
#include <string>
#include <vector>

namespace gsplat {

struct Timings : gs_timings {};   // init_sort_list_ms, radix_sort_ms, find_ranges_ms, render_ms, total_ms

class Renderer {
public:
    // Renderer.h:142-143: the averages skip the first WARMUP frames and are final after FRAMES more (the reference hard-codes
    // both; here they are constructor arguments so that a test or a short benchmark can use 3 + 5)
    static constexpr uint32_t WAIT_ELAPSED_WARMUP_FRAMES_FOR_AVG = 1000;
    static constexpr uint32_t WAIT_ELAPSED_FRAMES_FOR_AVG = 1000;

    Renderer(uint32_t width, uint32_t height, uint32_t warmupFramesForAvg = WAIT_ELAPSED_WARMUP_FRAMES_FOR_AVG,
             uint32_t framesForAvg = WAIT_ELAPSED_FRAMES_FOR_AVG)
        : width_(width), height_(height), warmupFrames_(warmupFramesForAvg), avgFrames_(framesForAvg) {}
    Renderer(const Renderer&) = delete;
    Renderer& operator=(const Renderer&) = delete;
    ~Renderer() { cleanup(); }

    // Renderer::init (Renderer.cpp:688-694).  cfg == nullptr: the reference's constants, with the GPU timestamps on
    // (this class keeps the RECORD_GPU_TIMES averages; gs_default_config leaves them off like GfxSettings.h:7).
    int init(const gs_config* cfg = nullptr) {
        const int rc_clean = cleanup();
        if (rc_clean != GS_OK) return rc_clean;
        if (gs_api_version() != GS_API_VERSION) {   // the structs below are laid out as THIS header declares them
            error_ = "libgsplat_hip.so has API version " + std::to_string(gs_api_version()) + ", this header " +
                     std::to_string(GS_API_VERSION);
            return GS_ERR_INVALID;
        }
        gs_config def;
        if (!cfg) { gs_default_config(&def); def.record_timings = 1; cfg = &def; }
        const int rc = gs_create(cfg, &ctx_);
        if (rc != GS_OK) error_ = gs_last_error(nullptr);
        return rc;
    }

    // Renderer::initForScene (Renderer.cpp:712-756): records = ResourceManager::getGaussians(), 336 B each.
    int initForScene(const void* gaussianRecords, uint32_t numGaussians) {
        int rc = gs_upload_gaussians(ctx_, gaussianRecords, numGaussians);
        if (rc == GS_OK) rc = gs_set_resolution(ctx_, width_, height_);
        if (rc != GS_OK) error_ = gs_last_error(ctx_);
        resetAverages();
        return rc;
    }
    // Frame slot (GfxSettings::FRAMES_IN_FLIGHT, GfxSettings.h:15): render the scene `owner` uploaded, with this
    // renderer's own per-frame buffers and stream.  The arrays are reference-counted inside the library, so the two
    // renderers may be cleaned up or destructed in any order.
    int initForSceneSharedWith(Renderer& owner) {
        int rc = gs_share_scene(ctx_, owner.ctx_);
        if (rc == GS_OK) rc = gs_set_resolution(ctx_, width_, height_);
        if (rc != GS_OK) error_ = gs_last_error(ctx_);
        resetAverages();
        return rc;
    }
    int initForScenePly(const std::string& path) {   // ResourceManager::loadGaussians + initForScene
        int rc = gs_load_ply(ctx_, path.c_str());
        if (rc == GS_OK) rc = gs_set_resolution(ctx_, width_, height_);
        if (rc != GS_OK) error_ = rc == GS_ERR_IO || rc == GS_ERR_FORMAT ? gs_ply_last_error() : gs_last_error(ctx_);
        resetAverages();
        return rc;
    }

    // Renderer::draw (Renderer.cpp:297-515).  view/proj: column-major float[16] (glm::mat4 memory);
    // shMode: one of GS_SH_* (0/1/2 = Camera.h:7-12, 5/4 = SH degree 1 and 2); rgbaOut: height*width*4 bytes, top row first.
    // The mode of an active SH degree 0..3 (gs_sh_mode_of_degree; a trainer's schedule: shModeOfDegree(min(3, t / 1000))),
    // or -1 for a degree above 3.  No context, no GPU.
    static int shModeOfDegree(uint32_t degree) {
        uint32_t mode = 0;
        return gs_sh_mode_of_degree(degree, &mode) == GS_OK ? (int)mode : -1;
    }
    int draw(const float* view, const float* proj, const float* camPos, uint32_t shMode, uint8_t* rgbaOut) {
        return frameDone(gs_render(ctx_, view, proj, camPos, shMode, rgbaOut));
    }
    // The same frame without the sink: the image stays in HBM -- rgbaOutDevice (a device pointer of height*width*4 bytes) or,
    // with nullptr, the library's own framebuffer (gs_debug_read(GS_BUF_IMAGE)) -- like the reference's frame, which ends
    // in the swapchain image and is never copied to the host.
    int drawDevice(const float* view, const float* proj, const float* camPos, uint32_t shMode, void* rgbaOutDevice = nullptr) {
        return frameDone(gs_render_device(ctx_, view, proj, camPos, shMode, rgbaOutDevice));
    }

    // The frame on R GPUs, one process per GPU (no reference counterpart; INTEGRATION.md "N GPUs from the same C++ host"):
    // init(cfg with device_ordinal = rank) -> initDist(id from distUniqueId() on one rank, rank, world) -> initForScene ->
    // shardRows -> drawSharded on every rank every frame; rank 0 gets the whole frame in rgbaOut, the others pass nullptr.
    static int distUniqueId(void* id128) { return gs_dist_unique_id(id128); }
    int initDist(const void* id128, int rank, int world) {
        const int rc = gs_dist_init(ctx_, id128, rank, world);
        if (rc != GS_OK) error_ = gs_last_error(ctx_);
        return rc;
    }
    // dealing: GS_ROWS_CONTIGUOUS / GS_ROWS_INTERLEAVED / GS_ROWS_BALANCED (bool converts: false / true = the first two)
    int shardRows(uint32_t dealing = GS_ROWS_CONTIGUOUS) {
        const int rc = gs_dist_shard_rows(ctx_, dealing);
        if (rc != GS_OK) error_ = gs_last_error(ctx_);
        return rc;
    }
    // synchronous: frame + exchange + copy to rgbaOut (rank 0); the averages take this rank's own rows
    int drawSharded(const float* view, const float* proj, const float* camPos, uint32_t shMode, uint8_t* rgbaOut) {
        return frameDone(gs_render_sharded(ctx_, view, proj, camPos, shMode, rgbaOut));
    }
    // two frames in flight: returns after enqueueing; the assembled frame stays in rank 0's HBM (shardedFrame / shardedRead;
    // which = 0: the frame just enqueued, 1: the one before).  No timings (nothing waits).
    int drawShardedAsync(const float* view, const float* proj, const float* camPos, uint32_t shMode) {
        const int rc = gs_render_sharded_async(ctx_, view, proj, camPos, shMode);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }
    int shardedFrame(uint32_t which, void** frameDevice) {
        const int rc = gs_sharded_frame(ctx_, which, frameDevice);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }
    int shardedRead(uint32_t which, uint8_t* rgbaOut) {
        const int rc = gs_sharded_read(ctx_, which, rgbaOut);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }
    // GS_ROWS_BALANCED, collective: move the band edges towards equal cost (gsplat.h); *moved = the edges changed
    int rebalance(bool* moved = nullptr) {
        uint32_t m = 0;
        const int rc = gs_dist_rebalance(ctx_, &m);
        if (rc < 0) error_ = gs_last_error(ctx_);
        if (moved) *moved = m != 0u;
        return rc;
    }

    // Optional per-pixel outputs of every later frame (gsplat.h, GS_OUTPUT_*): mask 0 = the RGBA8 frame alone (default).
    int setOutputs(uint32_t mask) {
        const int rc = gs_set_outputs(ctx_, mask);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }
    // host copy of the last frame's buffer `which` (one GS_OUTPUT_* bit): bytes >= H * W * 16 (RGBA32F) or H * W * 4 (DEPTH)
    int readOutput(uint32_t which, void* dst, size_t bytes) {
        const int rc = gs_read_output(ctx_, which, dst, bytes);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }
    // the device buffer itself (nullptr on failure, see lastError()); its contents are the last enqueued frame's once the
    // context's stream has been waited for
    void* outputDevice(uint32_t which, size_t* bytes = nullptr) {
        void* dev = nullptr;
        if (gs_output_device(ctx_, which, &dev, bytes) < 0) error_ = gs_last_error(ctx_);
        return dev;
    }

    // Gradients of the last frame (gsplat.h, gs_backward): HOST dL/dRGBA32F [H][W][4], dL/dDEPTH [H][W] (may be nullptr)
    // -> dL/d(record) [N][84]; device = true: the same as device pointers, enqueued without waiting.
    int backward(const float* grad_rgba32f, const float* grad_depth, float* grad_records, bool device = false) {
        const int rc = device ? gs_backward_device(ctx_, grad_rgba32f, grad_depth, grad_records)
                              : gs_backward(ctx_, grad_rgba32f, grad_depth, grad_records);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }

    // A context that owns a band of tile rows serves backward*, visibleCount and contribDevice with the terms of its own
    // pixels (gsplat.h, gs_set_band_gradients): partial sums, which the caller adds up over the bands of the frame.
    int setBandGradients(bool enable) {
        const int rc = gs_set_band_gradients(ctx_, enable ? 1u : 0u);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }

    // Anti-aliased frames (gsplat.h, gs_set_antialias): from the next frame on every splat is blended at its opacity times
    // sqrt(det S / det(S + 0.3 I)), S its 2-D covariance before the dilation.  A host flag of this context.
    int setAntialias(bool enable) {
        const int rc = gs_set_antialias(ctx_, enable ? 1u : 0u);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }

    // |V| of the last frame: the splats it rasterised (gsplat.h, gs_visible_count); 0 with error() set on a refusal.
    uint32_t visibleCount() {
        uint32_t count = 0;
        if (gs_visible_count(ctx_, &count) < 0) error_ = gs_last_error(ctx_);
        return count;
    }

    // The visible form of backward (gsplat.h, gs_backward_visible): the ids of V ascending and one [84] row for each, at
    // most max_rows of them; *count_out = |V|.  GS_WARN_OVERFLOW: |V| > max_rows (host form).  device = true: every
    // pointer is a device pointer and the call is enqueued without waiting.
    int backwardVisible(const float* grad_rgba32f, const float* grad_depth, uint32_t* ids_out, float* grad_rows_out,
                        uint32_t max_rows, uint32_t* count_out, bool device = false) {
        const int rc = device ? gs_backward_visible_device(ctx_, grad_rgba32f, grad_depth, ids_out, grad_rows_out, max_rows, count_out)
                              : gs_backward_visible(ctx_, grad_rgba32f, grad_depth, ids_out, grad_rows_out, max_rows, count_out);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }

    // The camera's gradients of the last frame (gsplat.h, gs_backward_camera), behind a backward() or backwardVisible() that
    // computed rows: grad_camera[GS_CAMERA_GRAD_FLOATS] = dL/dview[16], dL/dproj[16], dL/dcam_pos[3] on the HOST;
    // device = true: a device pointer, enqueued without waiting.
    int backwardCamera(float* grad_camera, bool device = false) {
        const int rc = device ? gs_backward_camera_device(ctx_, grad_camera) : gs_backward_camera(ctx_, grad_camera);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }

    // L1 + D-SSIM of a frame against a target (gsplat.h, gs_photometric_loss): HOST rgba [H][W][4] (nullptr = the context's
    // own GS_OUTPUT_RGBA32F buffer), target [H][W][3], bg[3] (nullptr = black) -> loss_out[3] = {loss, L1, DSSIM} and
    // dloss/d(rgba) [H][W][4] (nullptr = the numbers only), which backward() takes as it is.
    int photometricLoss(const float* rgba32f, const float* target_rgb, float lambda, const float* bg, float* loss_out,
                        float* grad_rgba32f) {
        const int rc = gs_photometric_loss(ctx_, rgba32f, target_rgb, lambda, bg, loss_out, grad_rgba32f);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }
    // the same with DEVICE pointers (bg stays a host pointer), enqueued on the context's stream without waiting
    int photometricLossDevice(const float* rgba32f, const float* target_rgb, float lambda, const float* bg, float* loss_out,
                              float* grad_rgba32f) {
        const int rc = gs_photometric_loss_device(ctx_, rgba32f, target_rgb, lambda, bg, loss_out, grad_rgba32f);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }

    // One optimiser step on the rows backwardVisible(device = true) lists (gsplat.h, gs_adam_rows_device and
    // gs_upload_rows_device): Adam on the caller's DEVICE records [N][84] and moments m, v, then the planes of the listed
    // splats rewritten from those records.  Both are enqueued on the context's stream without waiting; ids, grad_rows and
    // count are device pointers as backwardVisible left them.
    static gs_adam_params defaultAdamParams() {
        gs_adam_params p;
        gs_default_adam_params(&p);
        return p;
    }
    int adamRows(float* records, float* m, float* v, uint32_t n, const uint32_t* ids, const float* grad_rows,
                 const uint32_t* count, uint32_t max_rows, const gs_adam_params& params) {
        const int rc = gs_adam_rows_device(ctx_, records, m, v, n, ids, grad_rows, count, max_rows, &params);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }
    int uploadRows(const void* records, uint32_t n, const uint32_t* ids, const uint32_t* count, uint32_t max_rows) {
        const int rc = gs_upload_rows_device(ctx_, records, n, ids, count, max_rows);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }

    // The raw parameter space (gsplat.h, gs_adam_rows_raw_device and the calls around it): Adam on log-scales, the logit of
    // the opacity and the rotation before normalisation, with the listed rows of records rewritten as act(raw); the two
    // conversions; the INRIA opacity reset.  All DEVICE pointers, enqueued on the context's stream without waiting.
    static gs_adam_params defaultAdamParamsRaw() {
        gs_adam_params p;
        gs_default_adam_params_raw(&p);
        return p;
    }
    int adamRowsRaw(float* raw, float* records, float* m, float* v, uint32_t n, const uint32_t* ids, const float* grad_rows,
                    const uint32_t* count, uint32_t max_rows, const gs_adam_params& params) {
        const int rc = gs_adam_rows_raw_device(ctx_, raw, records, m, v, n, ids, grad_rows, count, max_rows, &params);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }
    int recordsFromRaw(const float* raw, float* records, uint32_t n) {
        const int rc = gs_records_from_raw_device(ctx_, raw, records, n);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }
    int rawFromRecords(const float* records, float* raw, uint32_t n) {
        const int rc = gs_raw_from_records_device(ctx_, records, raw, n);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }
    int resetOpacityRaw(float* raw, float* records, float* m, float* v, uint32_t n, float max_opacity = 0.01f) {
        const int rc = gs_reset_opacity_raw_device(ctx_, raw, records, m, v, n, max_opacity);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }
    // rows [n][84] on the HOST -> a .ply gs_load_ply reads; space = GS_PLY_FROM_RECORDS or GS_PLY_FROM_RAW (no context needed)
    static int writePly(const char* path, const float* rows, uint32_t n, uint32_t space) { return gs_write_ply(path, rows, n, space); }

    // Adaptive density control (gsplat.h, gs_densify_stats_device and gs_densify_device): the statistics of the step just
    // differentiated into the caller's DEVICE arrays [n], and the new cloud -- clones and split children beside their
    // parents -- into records_out / m_out / v_out [max_out][84]; counts_out[4] (device) = outputs, cloned, split, pruned.
    // Both are enqueued on the context's stream without waiting.
    static gs_densify_params defaultDensifyParams() {
        gs_densify_params p;
        gs_default_densify_params(&p);
        return p;
    }
    int densifyStats(const uint32_t* ids, const uint32_t* count, uint32_t max_rows, uint32_t n, float* grad_accum,
                     uint32_t* seen, float* max_radius) {
        const int rc = gs_densify_stats_device(ctx_, ids, count, max_rows, n, grad_accum, seen, max_radius);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }
    int densify(const float* records, const float* m, const float* v, uint32_t n, const float* grad_accum, const uint32_t* seen,
                const float* max_radius, const gs_densify_params& params, float* records_out, float* m_out, float* v_out,
                uint32_t max_out, uint32_t* counts_out) {
        const int rc = gs_densify_device(ctx_, records, m, v, n, grad_accum, seen, max_radius, &params, records_out, m_out, v_out,
                                         max_out, counts_out);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }

    // Absolute screen gradients (gsplat.h, gs_set_abs_gradients): with the switch on every backward also leaves the sums of
    // |dL_p/dsx|, |dL_p/dsy| per list element; absScreenGradient writes the pair of ids[i] to abs_out[i] (DEVICE
    // [max_rows][2]), densifyStatsAbs adds its norm in NDC units into grad_accum_abs (DEVICE [n]) beside densifyStats.
    int setAbsGradients(bool enable) {
        const int rc = gs_set_abs_gradients(ctx_, enable ? 1u : 0u);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }
    int absScreenGradient(const uint32_t* ids, const uint32_t* count, uint32_t max_rows, float* abs_out) {
        const int rc = gs_abs_screen_gradient_device(ctx_, ids, count, max_rows, abs_out);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }
    int densifyStatsAbs(const uint32_t* ids, const uint32_t* count, uint32_t max_rows, uint32_t n, float* grad_accum_abs) {
        const int rc = gs_densify_stats_abs_device(ctx_, ids, count, max_rows, n, grad_accum_abs);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }

    // Pruning by contribution (gsplat.h, gs_contrib_device and gs_prune_below_device): the blend weights of the last frame
    // accumulated per splat into the caller's DEVICE arrays wmax / wsum / pixels [n] (wsum and pixels may be null), and the
    // rows whose score reaches the threshold copied, in order, into records_out / raw_out / m_out / v_out [max_out][84] (raw,
    // m and v each null together with its output); counts_out[2] (device) = kept, dropped.  Both are enqueued on the
    // context's stream without waiting.
    int contrib(uint32_t n, float* wmax, float* wsum, uint32_t* pixels) {
        const int rc = gs_contrib_device(ctx_, n, wmax, wsum, pixels);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }
    int pruneBelow(const float* score, float threshold, uint32_t n, const float* records, const float* raw, const float* m,
                   const float* v, float* records_out, float* raw_out, float* m_out, float* v_out, uint32_t max_out,
                   uint32_t* counts_out) {
        const int rc = gs_prune_below_device(ctx_, score, threshold, n, records, raw, m, v, records_out, raw_out, m_out, v_out,
                                             max_out, counts_out);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }

    // MCMC (gsplat.h, gs_relocate_device, gs_grow_device and gs_position_noise_device): dead splats moved onto live ones in
    // place (ids_out / counts_out[3] = changed, dead, sources: what uploadRows takes), the cloud grown by n_add rows into
    // records_out / raw_out / m_out / v_out [max_out][84] (counts_out[2] = outputs, sources), and covariance-shaped noise on
    // the positions of the listed rows (ids null: every row).  All arrays on the DEVICE; enqueued on the context's stream
    // without waiting.
    int relocate(float* records, float* raw, float* m, float* v, uint32_t n, float min_opacity, uint64_t seed, uint32_t* ids_out,
                 uint32_t max_rows, uint32_t* counts_out) {
        const int rc = gs_relocate_device(ctx_, records, raw, m, v, n, min_opacity, seed, ids_out, max_rows, counts_out);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }
    int grow(const float* records, const float* raw, const float* m, const float* v, uint32_t n, float min_opacity, uint64_t seed,
             uint32_t n_add, float* records_out, float* raw_out, float* m_out, float* v_out, uint32_t max_out,
             uint32_t* counts_out) {
        const int rc = gs_grow_device(ctx_, records, raw, m, v, n, min_opacity, seed, n_add, records_out, raw_out, m_out, v_out,
                                      max_out, counts_out);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }
    int positionNoise(float* records, float* raw, uint32_t n, const uint32_t* ids, const uint32_t* count, uint32_t max_rows,
                      float scale, float gate_k = 100.0f, float gate_x0 = 0.995f, uint64_t seed = 0) {
        const int rc = gs_position_noise_device(ctx_, records, raw, n, ids, count, max_rows, scale, gate_k, gate_x0, seed);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }

    // Several views per optimiser step (gsplat.h, gs_rows_accumulate_device and gs_rows_collect_device): the listed rows of a
    // frame, times weight, summed into the caller's DEVICE accumulator acc [n][84] with a touch count per splat in mark [n]
    // (zeros before the first frame of a batch), then the touched rows as one ascending (ids, rows, count) list for adamRows
    // and uploadRows, with mark cleared.  Both are enqueued on the context's stream without waiting and need no scene.
    int rowsAccumulate(float* acc, uint32_t* mark, uint32_t n, const uint32_t* ids, const float* grad_rows, const uint32_t* count,
                       uint32_t max_rows, float weight) {
        const int rc = gs_rows_accumulate_device(ctx_, acc, mark, n, ids, grad_rows, count, max_rows, weight);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }
    int rowsCollect(const float* acc, uint32_t* mark, uint32_t n, uint32_t* ids_out, float* rows_out, uint32_t max_rows,
                    uint32_t* count_out) {
        const int rc = gs_rows_collect_device(ctx_, acc, mark, n, ids_out, rows_out, max_rows, count_out);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }

    // A cloud from points (gsplat.h, gs_knn_mean_dist2_device and gs_records_from_points_device): the exact mean squared
    // distance to the three nearest other points, in input order, and the first records of a training run -- rows in the
    // loader's Morton order, order_out[k] (may be null) = the input index of row k.  All arrays on the DEVICE; both are
    // enqueued on the context's stream without waiting and need no scene.
    static gs_init_params defaultInitParams() {
        gs_init_params p;
        gs_default_init_params(&p);
        return p;
    }
    int knnMeanDist2(const float* points, uint32_t n, float* dist2_out) {
        const int rc = gs_knn_mean_dist2_device(ctx_, points, n, dist2_out);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }
    int recordsFromPoints(const float* points, const float* colors, uint32_t n, const gs_init_params& params, float* records_out,
                          uint32_t* order_out = nullptr) {
        const int rc = gs_records_from_points_device(ctx_, points, colors, n, &params, records_out, order_out);
        if (rc < 0) error_ = gs_last_error(ctx_);
        return rc;
    }

    // Renderer::cleanup (Renderer.cpp:230-270).  gs_destroy always frees the context (gsplat.h), so the handle is
    // dropped before the call and never touched afterwards.
    int cleanup() {
        gs_ctx* c = ctx_;
        ctx_ = nullptr;
        return c ? gs_destroy(c) : GS_OK;
    }

    // RECORD_CPU_TIMES figures of the last draw (Renderer.cpp:399-456)
    gs_host_timings hostTimings() const { gs_host_timings t{}; if (ctx_) gs_get_host_timings(ctx_, &t); return t; }

    const gs_timings& lastTimings() const { return last_; }
    // avgInitSortListMs, avgSortMs, avgFindRangesMs, avgRenderGaussiansMs, avgTotalGpuTimeMs (Renderer.h): running means
    // over every frame after the warm-up (Renderer.cpp:477-488); averagesComplete() is where the reference reports them
    // (ALERT_FINAL_AVERAGE, Renderer.cpp:500-510: warm-up + framesForAvg frames have elapsed)
    const double* averages() const { return avg_; }
    // avgWaitForFenceMs, avgRecordCommandBufferMs, avgPresentMs, avgCpuFrameTimeMs (RECORD_CPU_TIMES, Renderer.cpp:399-456)
    const double* hostAverages() const { return havg_; }
    bool averagesComplete() const { return elapsedFrames_ >= (uint64_t)warmupFrames_ + avgFrames_; }
    uint64_t elapsedFrames() const { return elapsedFrames_; }
    const std::string& lastError() const { return error_; }
    gs_ctx* handle() const { return ctx_; }

    static uint32_t getCeilPowTwo(uint32_t x) { uint32_t n = 1; while (n < x) n *= 2; return n; }   // Renderer.cpp:703-710
    uint32_t getNumTiles() const { return ((width_ + 15) / 16) * ((height_ + 15) / 16); }            // Renderer.cpp:696-701

private:
    void resetAverages() {
        elapsedFrames_ = 0;
        for (double& a : avg_) a = 0.0;
        for (double& a : havg_) a = 0.0;
    }
    // Renderer.cpp:458-497: after the frame has been waited for, read the timestamps and fold them into the running means
    int frameDone(int rc) {
        if (rc < 0) { error_ = gs_last_error(ctx_); return rc; }
        gs_get_timings(ctx_, &last_);
        if (elapsedFrames_ >= warmupFrames_) {
            const double t = 1.0 / double(elapsedFrames_ - warmupFrames_ + 1);
            const double v[5] = {last_.init_sort_list_ms, last_.radix_sort_ms, last_.find_ranges_ms, last_.render_ms, last_.total_ms};
            for (int i = 0; i < 5; ++i) avg_[i] = (1.0 - t) * avg_[i] + t * v[i];
            const gs_host_timings h = hostTimings();
            const double hv[4] = {h.wait_ms, h.record_ms, h.present_ms, h.cpu_frame_ms};
            for (int i = 0; i < 4; ++i) havg_[i] = (1.0 - t) * havg_[i] + t * hv[i];
        }
        ++elapsedFrames_;
        return rc;
    }

    gs_ctx* ctx_ = nullptr;
    uint32_t width_, height_;
    uint32_t warmupFrames_, avgFrames_;
    gs_timings last_{};
    double avg_[5] = {0, 0, 0, 0, 0};
    double havg_[4] = {0, 0, 0, 0};
    uint64_t elapsedFrames_ = 0;
    std::string error_;
};

}  // namespace gsplat
