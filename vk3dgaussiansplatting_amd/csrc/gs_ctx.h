// gs_ctx.h -- the context behind the opaque gs_ctx handle of include/gsplat.h, the owner of its device memory
// (DeviceOwner), what the last frame left behind (LastFrame) and the one error exit of the host code (fail / HIP_TRY).
// Internal: shared by the host files of the library (gs_api.cpp: context, scene, resolution, frame; gs_train.cpp: the training
// calls; gs_debug.cpp: read-backs and micro-benchmarks; gs_dist.cpp) and the tuning probes of tools/probe (libgsplat_probe.so),
// which are built from this tree against the same layout.
#pragma once

#include "../../include/gsplat.h"
#include "gs_internal.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

// The device allocations of one lifetime.  The structs the kernels take by value (SceneBuffers, SortBuffers, ...) stay
// plain pointers; the owner beside them remembers which of their slots it filled and frees them together, so that a
// pointer added to such a struct cannot be forgotten by the code that ends its lifetime.  The slots must not move.
struct DeviceOwner {
    std::vector<void**> slots;
    template <typename T> hipError_t alloc(T*& slot, size_t bytes) {
        const hipError_t e = hipMalloc((void**)&slot, bytes);
        if (e == hipSuccess) slots.push_back((void**)&slot); else slot = nullptr;
        return e;
    }
    template <typename T> hipError_t alloc_zeroed(T*& slot, size_t bytes, hipStream_t stream) {
        const hipError_t e = alloc(slot, bytes);
        return e == hipSuccess ? hipMemsetAsync(slot, 0, bytes, stream) : e;
    }
    template <typename T> void free(T*& slot) {      // one slot inside the lifetime (no-op for a slot that is not held)
        const auto it = std::find(slots.begin(), slots.end(), (void**)&slot);
        if (it == slots.end()) return;
        (void)hipFree(slot);
        slot = nullptr;
        slots.erase(it);
    }
    void release() {
        for (void** s : slots) { (void)hipFree(*s); *s = nullptr; }
        slots.clear();
    }
};

// The uploaded gaussian arrays (read-only on the path), reference-counted so that the contexts that render them
// (gs_share_scene: frame slots, tile-row bands) can be destroyed in any order; the last reference releases `mem`.
struct SharedScene {
    gs::SceneBuffers b{};
    DeviceOwner mem;
    uint32_t n = 0;
    std::atomic<uint32_t> refs{1};
};

using HostClock = std::chrono::steady_clock;

#define GS_HIDDEN __attribute__((visibility("hidden")))

// What the last call that launched a sort list left behind.  Only the transitions behind gs_ctx write it; a call that is
// about to launch a list first says so (list_launching), so nothing of an earlier frame stays readable or differentiable
// when that call fails half way.
struct LastFrame {
    enum Kind : uint8_t { kNone, kUnsortedList, kFrame };
    Kind kind = kNone;            // kUnsortedList: gs_debug_init_sort_list ran last; kFrame: a frame was enqueued last
    bool differentiable = false;  // kFrame, and no upload or tile-row change since: gs_backward* may run
    bool has_backward = false;    // bwd.rows holds a backward of this frame (a gs_backward* form ran the blend): what
                                  // gs_densify_stats_device and gs_backward_camera* sum
    bool has_abs_backward = false;  // ... and that blend ran with gs_set_abs_gradients on: bwd.abs_rows holds the absolute pairs
                                  // of this frame, what gs_abs_screen_gradient_device and gs_densify_stats_abs_device sum
    int sorted_index = 0;         // kFrame: which ping-pong half holds the sorted list
    gs::FrameParams fp{};         // of the InitSortList launch (gs_debug_read(GS_BUF_COLOR) evaluates colours on demand)
};

// A captured run of launches and what its capture returned (the ping-pong half that holds the sorted list)
struct FrameGraph {
    hipGraphExec_t exec = nullptr;
    int result = 0;
};

// The five buckets of gs_timings a frame's intervals are booked under (Renderer.cpp:458-475)
enum FrameBucket : uint8_t { kBucketNone, kBucketInit, kBucketSort, kBucketRanges, kBucketRender };
// marks of the longest frame (splat-first): begin, splat list, depth passes, gather + emit, tile passes, ranges, render
constexpr int kMaxFrameMarks = 7;

struct gs_ctx {
    gs_config cfg{};
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // record_timings: one timeline per frame -- an event at every bucket boundary, and the bucket the interval that ends
    // there is booked under (the reference's 7 timestamp points, Renderer.cpp:540-629, per sorter)
    hipEvent_t marks[kMaxFrameMarks] = {};
    uint8_t mark_bucket[kMaxFrameMarks] = {};
    uint32_t num_marks = 0;
    hipEvent_t scatter_ev[32] = {};   // record_timings == 2: a pair per pass (<= 16 passes), the frame's runs one after the other
    hipStream_t helper_stream = nullptr;   // GS_SORT_TILE_BUCKET: big size classes run beside the small ones
    hipEvent_t fork_ev = nullptr, join_ev = nullptr;
    std::string last_error;

    // scene
    uint32_t n = 0;
    gs::SceneBuffers scene{};
    gs::SplatScratch scratch{};
    DeviceOwner scene_mem;            // of `scratch` (the gaussian arrays belong to `shared`)
    uint32_t num_blocks = 0;
    uint32_t emit_parity = 0;     // FrameParams::parity of the last InitSortList launch
    SharedScene* shared = nullptr;    // owner of `scene`'s arrays (this context holds one reference)

    // resolution-dependent
    uint32_t width = 0, height = 0, grid_w = 0, grid_h = 0;
    // tile rows of this context: first_row + k * row_stride < row_end, k < rows_owned (FrameParams)
    uint32_t row_begin = 0, row_end = 0, row_stride = 1, first_row = 0, rows_owned = 0;
    bool compact_out = false;
    bool band_gradients = false;      // gs_set_band_gradients: gs_backward* and gs_contrib_device serve a band of tile rows
    bool abs_gradients = false;       // gs_set_abs_gradients: the gs_backward* forms run k_bwd_blend<true> and leave bwd.abs_rows
    bool antialias = false;           // gs_set_antialias: FrameParams::antialias of the frames enqueued from now on (a host flag of the
                                      // context, not of the scene; nothing but make_frame_params reads it)
    uint32_t capacity = 0, num_sort_bits = 0;
    // what the sort of the owned tiles runs over: compact tile ids, so ceil((32 + bits(T_owned - 1)) / 4) passes
    // (the reference's formula, RadixSort.cpp:203-204, for the context's own tile count)
    uint32_t band_sort_bits = 0;
    bool hi16 = false;   // the frame's sort list stores the compact tile ids as uint16 (at most 65535 owned tiles)
    gs::SortBuffers sort{};
    DeviceOwner res_mem;              // of everything sized by the resolution: sort, ranges, tile_order, framebuffer, outputs
    // gs_set_outputs: the optional per-pixel outputs, addressed like the RGBA8 image (the view depths of the splats live in
    // scratch.view_z, which follows the mask and the scene)
    uint32_t outputs = 0;             // GS_OUTPUT_* mask
    float* out_rgba32f = nullptr;     // [H][W][4] while GS_OUTPUT_RGBA32F is on and a resolution is set
    float* out_depth = nullptr;       // [H][W] while GS_OUTPUT_DEPTH is on and a resolution is set
    bool outputs_valid = false;       // a frame has been enqueued since the mask or the resolution last changed
    // gs_backward*: scratch allocated on the first call (rows sized by the list capacity; abs_rows, 8 bytes per list element,
    // on the first call with gs_set_abs_gradients on), freed with the resolution
    gs::BackwardBuffers bwd{};
    DeviceOwner bwd_mem;              // of bwd and bwd_host_in / _out / bwd_vis_out / bwd_cam_partials / bwd_cam_out
    float* bwd_host_in = nullptr;     // gs_backward (host pointers): dL/dRGBA32F [H][W][4] + dL/dDEPTH [H][W] on the device
    float* bwd_host_out = nullptr;    // ... and the record gradients [N][84]
    float* bwd_vis_out = nullptr;     // gs_backward_visible (host pointers): bwd_vis_rows record gradients, grown on demand
    uint32_t bwd_vis_rows = 0;
    float* bwd_cam_partials = nullptr;   // gs_backward_camera*: [35][blocks of 256 gaussians], allocated on its first call
    float* bwd_cam_out = nullptr;        // gs_backward_camera (host pointer): the 35 floats on the device
    // gs_contrib_device: 12 bytes per list element of capacity, and slot offsets of its own (K = 1) while no backward has
    // allocated bwd.scan, which it shares from then on; both owned by bwd_mem (allocated on first use, freed with the resolution)
    uint32_t* contrib_rows = nullptr;
    gs::SplatScan contrib_scan{};
    // gs_densify_device (K = 4), gs_rows_collect_device and gs_prune_below_device (K = 2): their scan for densify_cap splats; grown on demand, freed at gs_destroy
    gs::SplatScan densify_scan{};
    uint32_t densify_cap = 0;
    DeviceOwner densify_mem;
    // gs_relocate_device / gs_grow_device: the sampler's scratch for mcmc_cap splats (12 bytes per splat + 16 bytes per 256
    // splats + the two tables); grown on demand, freed at gs_destroy.  Their per-splat scan is densify_scan.
    gs::McmcScratch mcmc{};
    uint32_t mcmc_cap = 0;
    DeviceOwner mcmc_mem;
    // gs_knn_mean_dist2_device / gs_records_from_points_device: scratch and sort buffers for init_cap points; grown on
    // demand, freed at gs_destroy
    gs::InitScratch init{};
    gs::SortBuffers init_sort{};
    uint32_t init_cap = 0;
    DeviceOwner init_mem;
    // gs_photometric_loss*: scratch allocated on the first call (9 floats per pixel + 8 bytes per tile), freed with the
    // resolution; loss_host = the device copies of the host form's arguments (rgba, target, gradient, the three numbers)
    gs::LossBuffers loss{};
    DeviceOwner loss_mem;             // of loss and loss_host
    float* loss_host = nullptr;
    uint32_t* ranges = nullptr;
    uint32_t* tile_order = nullptr;   // [tiles] RenderGaussians' dispatch order (GS_TILE_ORDER_LONGEST_FIRST)
    uint8_t* framebuffer = nullptr;
    // The radix passes of a frame (3 launches per pass, parameters fixed once resolution and band are) replayed
    // as one hipGraph launch: 36 launches -> 1 on the host side.  Built lazily, dropped when anything it baked in
    // changes.  Not used while per-Scatter events are recorded (record_timings == 2).
    gs::SortRun runs[2] = {};         // the runs of passes the last frame launched (splat-first: depth passes, tile passes)
    uint32_t num_runs = 0;
    FrameGraph run_graph[2];          // with timers: each run replays alone
    FrameGraph chain_graph;           // without timers: every camera-free stage up to FindRanges as one graph
    bool sort_graph_failed = false;
    uint32_t* elems_note = nullptr;   // pinned host word k_scan_blocks writes (element count + 1 of the latest list; 0: none
                                      // since the rows were set) -- what GS_COUNT_AUTO goes by
    bool sort_fed = false;        // the captured radix passes are the fed kind (k_scatter<.., FED>)
    bool sort_packed = false;     // ... and carry the packed payload through the depth passes (SortRun::packed)
    bool sort_pass0 = false;      // ... and start behind pass 0, which k_emit does (SortRun::passes_done; GS_EMIT_PASS0)
    bool last_pass0 = false;      // the last frame was enqueued that way: gs_debug_read(GS_BUF_PASS0_OFFSETS) has its table

    gs_timings timings{};
    gs_host_timings host{};           // RECORD_CPU_TIMES (Renderer.cpp:299-456)
    HostClock::time_point last_entry{};
    bool have_entry = false;
    LastFrame last;

    // gs_dist_init: the RCCL communicator of a multi-GPU frame (gs_dist.cpp)
    void* dist_comm = nullptr;
    int dist_rank = 0, dist_world = 1;
    // gs_dist_shard_rows: how the tile rows are dealt, and the buffers of a sharded frame -- two slots, so that the gather
    // of frame f (on dist_stream) runs beside the kernels of frame f + 1 (on the context's stream)
    uint32_t dist_dealing = 0;            // GS_ROWS_*
    bool dist_sharded = false;
    std::vector<uint32_t> dist_edges;     // contiguous / balanced: R + 1 band edges (tile rows), the same on every rank
    uint32_t dist_rows_sig[5] = {};       // row_begin, row_end, row_stride, first_row, compact_out the buffers were set up for
    void* dist_strip[2] = {};             // this rank's rows (not on the root of a contiguous dealing: it renders into the frame)
    void* dist_gathered[2] = {};          // root, interleaved rows: the ranks' packed strips before they are re-ordered
    void* dist_image[2] = {};             // root: the assembled frame, left in HBM
    size_t dist_strip_bytes = 0;          // interleaved: bytes of one rank's packed strip (the same on every rank)
    hipStream_t dist_stream = nullptr;
    hipEvent_t dist_begin[2] = {}, dist_rendered[2] = {}, dist_done[2] = {};
    bool dist_used[2] = {false, false};   // the slot's events have been recorded
    int dist_next = 0;                    // slot of the next gs_render_sharded_async
    int dist_recent[2] = {-1, -1};        // slots of the last and the last-but-one sharded frame
    void* dist_xchg = nullptr;            // gs_dist_rebalance: R x (tiles_y + 1) words
    std::vector<std::pair<double, double>> dist_history;   // ... (elements, ms) of every rank over the last epochs
};


// Text of gs_last_error(NULL): what failed without a context at hand; hidden: not an export.
__attribute__((visibility("hidden"))) inline thread_local std::string gsi_create_error;

// The error exit of every entry point: the text for gs_last_error, the code for the caller.
inline int fail(gs_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->last_error = msg; else gsi_create_error = msg;
    return code;
}

#define HIP_TRY(ctx, expr)                                                                       \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess)                                                                    \
            return fail((ctx), GS_ERR_HIP,                                                       \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                      \
    } while (0)

// ---- the transitions of gs_ctx::last (and of outputs_valid, which lives as long as the mask: gs_set_outputs and the end of
//      a resolution clear it too)
// First statement of a call that launches a sort list: until it succeeds nothing is readable or differentiable
GS_HIDDEN inline void list_launching(gs_ctx* c) {
    c->last.kind = LastFrame::kNone;
    c->last.differentiable = c->last.has_backward = c->last.has_abs_backward = c->outputs_valid = false;
}
GS_HIDDEN inline void frame_enqueued(gs_ctx* c, const gs::FrameParams& fp, int sorted_index) {
    c->last = {LastFrame::kFrame, true, false, false, sorted_index, fp};
    c->outputs_valid = c->outputs != 0u;
}
// gs_debug_init_sort_list succeeded; the list touches no output buffer: those are as valid as they were before it
GS_HIDDEN inline void unsorted_list_ready(gs_ctx* c, const gs::FrameParams& fp, bool outputs_valid) {
    c->last.kind = LastFrame::kUnsortedList;
    c->last.fp = fp;
    c->outputs_valid = outputs_valid;
}
// An in-place upload or a change of the tile rows: the lists stay readable, the frame is no longer the scene's
GS_HIDDEN inline void scene_or_rows_changed(gs_ctx* c) {
    c->last.differentiable = c->last.has_backward = c->last.has_abs_backward = false;
}
// The blend of a gs_backward* form was enqueued: bwd.rows is this frame's, and bwd.abs_rows with the switch on (a blend with
// the switch off leaves the pairs of an earlier one, which belong to other image gradients: they no longer count)
GS_HIDDEN inline void backward_ran(gs_ctx* c) {
    c->last.has_backward = true;
    c->last.has_abs_backward = c->abs_gradients;
}
GS_HIDDEN inline void resolution_freed(gs_ctx* c) { list_launching(c); }      // (its output buffers are gone with it)

// gs_dist.cpp: frees the buffers of a sharded frame (they are sized by the resolution).
GS_HIDDEN void gsi_dist_free_buffers(gs_ctx* c);
// Renderer.cpp:458-475 for a frame enqueued with gs_render_device_async: wait, read the timestamps, fill gs_get_timings.
GS_HIDDEN int gsi_finish_frame(gs_ctx* c);
// gs_api.cpp, for gs_train.cpp and gs_debug.cpp: the error of the launches just made, under the name `what`
GS_HIDDEN int check_launch(gs_ctx* ctx, const char* what);
// ... the sort buffers of a list of `capacity` elements, owned by `mem` (which the caller releases, after a failure too)
GS_HIDDEN int alloc_sort(gs_ctx* ctx, DeviceOwner& mem, gs::SortBuffers& s, uint32_t capacity);
// ... the run of the stand-alone sorters: the whole key over a list of n elements, nothing dropped
GS_HIDDEN gs::SortRun whole_list_run(const gs_ctx* c, uint32_t n, uint32_t num_sort_bits);
GS_HIDDEN uint32_t num_sort_bits_for(uint32_t num_tiles);      // RadixSort.cpp:7-16 + 203-204
// ... which: one GS_OUTPUT_* bit that is enabled and allocated -> its buffer and size; else fails
GS_HIDDEN int output_buffer(gs_ctx* c, uint32_t which, const char* who, void** dev, size_t* size);

namespace gs {

// the five GS_SH_* modes; 3 names none (refused before the degrees existed, and still) -- what gs_render* and
// gs_debug_init_sort_list refuse with GS_SH_MODE_REFUSAL behind their own name
inline bool sh_mode_known(uint32_t sh_mode) { return sh_mode <= GS_SH_ONLY_FIRST_BAND || sh_mode == GS_SH_DEGREE_2 || sh_mode == GS_SH_DEGREE_1; }
#define GS_SH_MODE_REFUSAL "sh_mode must be one of GS_SH_* (0, 1, 2, 4, 5)"

inline FrameParams make_frame_params(const gs_ctx* c, const float* view, const float* proj,
                              const float* cam_pos, uint32_t sh_mode) {
    FrameParams fp{};
    std::memcpy(fp.view, view, sizeof(fp.view));
    std::memcpy(fp.proj, proj, sizeof(fp.proj));
    std::memcpy(fp.cam_pos, cam_pos, sizeof(fp.cam_pos));
    fp.sh_mode = sh_mode;
    fp.width = c->width; fp.height = c->height;
    fp.grid_w = c->grid_w; fp.grid_h = c->grid_h;
    fp.row_begin = c->row_begin; fp.row_end = c->row_end;
    fp.row_stride = c->row_stride; fp.first_row = c->first_row; fp.rows_owned = c->rows_owned;
    fp.compact_out = c->compact_out ? 1u : 0u;
    fp.num_gaussians = c->n;
    fp.capacity = c->capacity;
    fp.near_plane = c->cfg.near_plane; fp.far_plane = c->cfg.far_plane;
    fp.ndc_cull = c->cfg.ndc_cull; fp.in_view_limit = c->cfg.in_view_limit;
    fp.tan_fov_y = (float)std::tan((double)(c->cfg.fov_y * 0.5f));   // Common.glsl:53, host-folded
    fp.hi16 = c->hi16 ? 1u : 0u;
    fp.parity = 0u;       // set by the InitSortList launch sites
    fp.antialias = c->antialias ? 1u : 0u;
    // |W|_2^2 <= min(trace, largest absolute row sum) of M = W^T W (Gershgorin); exactly 1 (+ rounding) for a rigid view
    double m[3][3], tr = 0.0, gersh = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            m[i][j] = 0.0;
            for (int k = 0; k < 3; ++k) m[i][j] += (double)view[i * 4 + k] * (double)view[j * 4 + k];
        }
    for (int i = 0; i < 3; ++i) {
        tr += m[i][i];
        gersh = std::max(gersh, std::fabs(m[i][0]) + std::fabs(m[i][1]) + std::fabs(m[i][2]));
    }
    fp.w_norm2 = (float)(std::min(tr, gersh) * (1.0 + 1e-5));
    return fp;
}

} // namespace gs
