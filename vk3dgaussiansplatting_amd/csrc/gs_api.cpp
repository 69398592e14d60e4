// gs_api.cpp -- host side of libgsplat_hip.so: the C-ABI of include/gsplat.h over the HIP kernels.
// Mirrors the reference's frame orchestration (Engine/Graphics/Renderer.cpp, Subrenderer.cpp,
// Sort/RadixSort.cpp) with HIP streams/events in place of Vulkan command buffers/timestamps.
// There is NO CPU fallback: without a GPU every entry point that computes fails with
// GS_ERR_NO_DEVICE / GS_ERR_HIP.
#include "../../include/gsplat.h"
#include "gs_internal.h"
#include "gs_ctx.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <iterator>
#include <limits>
#include <new>
#include <string>
#include <vector>

using namespace gs;

namespace {

void free_scene(gs_ctx* c) {
    if (c->shared) {                  // drop this context's reference; the last one frees the arrays
        if (c->shared->refs.fetch_sub(1) == 1) {
            c->shared->mem.release();
            delete c->shared;
        }
        c->shared = nullptr;
    }
    c->scene = SceneBuffers{};
    c->scene_mem.release();
    c->n = 0;
}

void drop_sort_graph(gs_ctx* c) {
    for (FrameGraph* g : {&c->run_graph[0], &c->run_graph[1], &c->chain_graph})
        if (g->exec) { (void)hipGraphExecDestroy(g->exec); g->exec = nullptr; }
    c->sort_graph_failed = false;
}

void free_resolution(gs_ctx* c) {
    c->bwd_mem.release();
    c->bwd_vis_rows = 0;
    c->loss_mem.release();
    c->bwd_frame = false; c->bwd_rows = false;
    drop_sort_graph(c);
    c->res_mem.release();
    c->sort = SortBuffers{};          // fed[1], fed[2] point into the allocation of fed[0]
    c->outputs_valid = false;
    // the strips of a sharded frame are sized by the resolution: gs_dist_shard_rows must be called again
    gsi_dist_free_buffers(c);
    c->capacity = 0; c->width = c->height = 0;
    c->have_frame = false;
    if (c->elems_note) *(volatile uint32_t*)c->elems_note = 0u;     // (free_resolution's callers have waited for the stream)
}

// Renderer.cpp:703-710
uint32_t ceil_pow2(uint32_t x) { uint32_t v = 1; while (v < x) v *= 2; return v; }

// RadixSort.cpp:7-16 + 203-204
uint32_t num_sort_bits_for(uint32_t num_tiles) {
    uint32_t x = num_tiles - 1u, bits = 0;
    for (int i = 31; i >= 0; --i) if ((x >> i) & 1u) { bits = (uint32_t)i + 1u; break; }
    return ((32u + bits + kRadixBits - 1u) / kRadixBits) * kRadixBits;
}

inline bool sorts_splat_first(uint32_t algo) { return algo == GS_SORT_RADIX4_SPLAT_FIRST || algo == GS_SORT_RADIX8_SPLAT_FIRST; }
inline uint32_t digit_bits_of(uint32_t algo) { return algo == GS_SORT_RADIX8 || algo == GS_SORT_RADIX8_SPLAT_FIRST ? 8u : (uint32_t)kRadixBits; }

// the sort buffers of a list of `capacity` elements, owned by `mem` (which the caller releases, after a failure too)
int alloc_sort(gs_ctx* ctx, DeviceOwner& mem, SortBuffers& s, uint32_t capacity) {
    const size_t bytes = (size_t)capacity * sizeof(uint32_t);
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(ctx, mem.alloc(s.lo[k], bytes));
        HIP_TRY(ctx, mem.alloc(s.hi[k], bytes));
        HIP_TRY(ctx, mem.alloc(s.id[k], bytes));
    }
    s.digit_bits = digit_bits_of(ctx->cfg.sort_algorithm);
    if (s.digit_bits == 8u) {   // gs_sort8.hip: [groups][256] counts; segment counts + their scan
        const uint32_t max_groups = (capacity + kSort8TileSmall - 1) / kSort8TileSmall;   // the smaller of the two group sizes
        HIP_TRY(ctx, mem.alloc(s.table, (size_t)kBins8 * max_groups * sizeof(uint32_t)));
        HIP_TRY(ctx, mem.alloc(s.seg_sum, (size_t)2 * kBins8 * kSegments * sizeof(uint32_t)));
    } else {
        const uint32_t max_groups = (capacity + kSortTile - 1) / kSortTile;
        HIP_TRY(ctx, mem.alloc(s.table, (size_t)kBins * max_groups * sizeof(uint32_t)));
        HIP_TRY(ctx, mem.alloc(s.seg_sum, (size_t)kBins * kSegments * sizeof(uint32_t)));
        // fed counts: three rotating sets of [groups][16] rows (k_scatter<.., FED>); every row a pass reads was written or
        // cleared earlier in the same sort, so no initial clear
        const size_t set_words = (size_t)kBins * max_groups;
        HIP_TRY(ctx, mem.alloc(s.fed[0], 3 * set_words * sizeof(uint32_t)));
        s.fed[1] = s.fed[0] + set_words;
        s.fed[2] = s.fed[1] + set_words;
    }
    HIP_TRY(ctx, mem.alloc(s.params, sizeof(SortParams)));
    HIP_TRY(ctx, hipMemset(s.params, 0, sizeof(SortParams)));
    HIP_TRY(ctx, mem.alloc(s.coarse, (size_t)kMaxSortPasses * kBins * kCoarse * sizeof(uint32_t)));
    return GS_OK;
}

// The run of the stand-alone sorters: the whole key over a list of n elements, nothing dropped.  They know their element
// count: fed counts (gs_sort.hip) for short lists of the 4-bit sorter.
SortRun whole_list_run(const gs_ctx* c, uint32_t n, uint32_t num_sort_bits) {
    const bool fed = digit_bits_of(c->cfg.sort_algorithm) == (uint32_t)kRadixBits &&
                     (c->cfg.count_launches == GS_COUNT_FED ||
                      (c->cfg.count_launches == GS_COUNT_AUTO && n <= kFedMaxGroups * (uint32_t)kSortTile));
    return {.capacity = n, .num_sort_bits = num_sort_bits, .fed = fed};
}

int check_launch(gs_ctx* ctx, const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, GS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return GS_OK;
}

// ---- the stages of a frame behind project + scan (Renderer::recordCommandBuffer, Renderer.cpp:540-629), once per sorter:
//      what a stage launches, the bucket of gs_timings its interval is booked under, the name check_launch reports it by,
//      and whether its arguments are free of the camera (such stages can be captured once and replayed)
enum StageKind : uint8_t { kStageSplatList, kStageGatherEmit, kStageEmit, kStagePasses, kStageRanges, kStageTileSort };
struct Stage {
    StageKind kind;
    uint32_t run;            // kStagePasses: which of gs_ctx::runs
    FrameBucket bucket;
    const char* name;
    bool camera_free;
};
// GS_SORT_RADIX*_SPLAT_FIRST: the depth passes run over the list of emitting splats, the emit walks that list in depth order,
// the tile-word passes finish.  InitSortList = project + lists + emit, RadixSort = all passes.
const Stage kSplatFirstFrame[] = {
    {kStageSplatList, 0, kBucketInit, "InitSortList", true},
    {kStagePasses, 0, kBucketSort, "RadixSort", true},
    {kStageGatherEmit, 0, kBucketInit, "InitSortList", true},
    {kStagePasses, 1, kBucketSort, "RadixSort", true},
    {kStageRanges, 0, kBucketRanges, "FindRanges", true},    // computeRanges (Subrenderer.cpp:172-216)
};
// GS_SORT_RADIX4 / _RADIX8: computeInitSortList (Subrenderer.cpp:37-170), gpuSort->computeSort (RadixSort.cpp:207-653), ranges
const Stage kPlainFrame[] = {
    {kStageEmit, 0, kBucketInit, "InitSortList", false},
    {kStagePasses, 0, kBucketSort, "RadixSort", true},
    {kStageRanges, 0, kBucketRanges, "FindRanges", true},
};
// GS_SORT_TILE_BUCKET: the tile-word passes alone, then -- it needs the ranges -- the per-tile depth sort, booked under
// RadixSort.  That sort forks onto helper_stream, so nothing of this frame is captured as a chain.
const Stage kBucketFrame[] = {
    {kStageEmit, 0, kBucketInit, "InitSortList", false},
    {kStagePasses, 0, kBucketSort, "RadixSort", false},
    {kStageRanges, 0, kBucketRanges, "FindRanges", false},
    {kStageTileSort, 0, kBucketSort, "TileSort", false},
};

// What the stages of one enqueue_frame share
struct Frame {
    gs_ctx* c;
    FrameParams fp;          // the frame's own
    FrameParams fixed;       // what the camera-free stages take
    bool ordered;
    bool direct;             // record_timings >= 2: nothing is captured
    int sorted;              // ping-pong half of the list the last run of passes left
};

// `launch` enqueues launches whose arguments never change and returns the ping-pong half of the list they leave (< 0:
// not enqueued).  Captured once into `g` (nothing executes during capture) and replayed; direct launches where the frame
// asks for them or a capture has failed.
template <typename F>
int capture_or_replay(Frame& f, FrameGraph& g, F&& launch) {
    gs_ctx* c = f.c;
    hipStream_t st = c->stream;
    if (!f.direct && !g.exec && !c->sort_graph_failed) {
        hipGraph_t graph = nullptr;
        bool ok = hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed) == hipSuccess;
        if (ok) {
            g.result = launch();
            ok = hipStreamEndCapture(st, &graph) == hipSuccess && graph != nullptr;
        }
        if (ok) ok = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0) == hipSuccess;
        if (graph) (void)hipGraphDestroy(graph);
        if (!ok) { g.exec = nullptr; c->sort_graph_failed = true; (void)hipGetLastError(); }
    }
    if (!f.direct && g.exec) return hipGraphLaunch(g.exec, st) == hipSuccess ? g.result : -1;
    return launch();
}

// One stage onto the stream -> the half that holds the list behind it, < 0 when launch_radix_sort refused its run.
// graphs: a run of passes replays as its own graph (else it is being captured as part of a longer one).
int launch_stage(Frame& f, const Stage& s, bool graphs) {
    gs_ctx* c = f.c;
    hipStream_t st = c->stream;
    switch (s.kind) {
        case kStageSplatList: launch_splat_list(f.fixed, c->scratch, c->sort, st); break;
        case kStageGatherEmit:
            launch_gather_sorted(f.fixed, c->scratch, c->sort, f.sorted, st);
            launch_emit_sorted(f.fixed, c->scratch, c->sort, f.sorted, st);
            break;
        case kStageEmit: launch_emit(f.fp, c->scratch, c->sort, st); break;
        case kStagePasses: {
            auto passes = [&] { return launch_radix_sort(c->sort, c->runs[s.run], st); };
            f.sorted = graphs ? capture_or_replay(f, c->run_graph[s.run], passes) : passes();
            break;
        }
        case kStageRanges:
            launch_find_ranges(f.fixed, c->sort.hi[f.sorted], c->sort.params, c->ranges, st);
            if (f.ordered) launch_tile_order(f.fixed, c->ranges, c->tile_order, st);
            break;
        case kStageTileSort:
            launch_tile_sort(f.fp, c->ranges, c->sort.lo[f.sorted], c->sort.id[f.sorted], c->sort.lo[f.sorted ^ 1],
                             c->sort.id[f.sorted ^ 1], st, c->helper_stream, c->fork_ev, c->join_ev);
            break;
    }
    return f.sorted;
}

// record_timings: the interval that ends here belongs to bucket b
int mark(gs_ctx* c, FrameBucket b) {
    HIP_TRY(c, hipEventRecord(c->marks[c->num_marks], c->stream));
    c->mark_bucket[c->num_marks++] = b;
    return GS_OK;
}

int enqueue_frame(gs_ctx* c, const float* view, const float* proj, const float* cam_pos,
                  uint32_t sh_mode, uint8_t* out_dev) {
    if (!c->n) return fail(c, GS_ERR_NO_SCENE, "gs_render: no gaussians uploaded");
    if (!c->capacity) return fail(c, GS_ERR_NO_SCENE, "gs_render: gs_set_resolution not called");
    if (!view || !proj || !cam_pos) return fail(c, GS_ERR_INVALID, "gs_render: null camera argument");
    if (sh_mode > 2u) return fail(c, GS_ERR_INVALID, "gs_render: sh_mode must be 0, 1 or 2");
    Frame f{c, make_frame_params(c, view, proj, cam_pos, sh_mode)};
    FrameParams& fp = f.fp;
    if (!out_dev) fp.compact_out = 0u;   // the internal framebuffer is always a whole frame in real rows
    const bool tm = c->cfg.record_timings != 0;
    hipStream_t st = c->stream;

    c->unsorted_valid = false;
    c->bwd_rows = false;          // from here on the rows scratch belongs to a frame that is no longer the current one
    c->num_marks = 0;
    if (tm) if (int r = mark(c, kBucketNone)) return r;
    // computeInitSortList (Subrenderer.cpp:37-170): per-frame resets, then the dispatch.  Only the
    // ranges need clearing here: the 0xFF sentinel fill of both lists (Subrenderer.cpp:42-46,
    // RadixSort.cpp:676-692) is unobservable once every later stage runs over E instead of C.
    // (the ranges and the sort's coarse totals are cleared inside k_scan_blocks: no fill launches in a frame)
    fp.parity = (c->emit_parity ^= 1u);
    c->last_fp = fp;
    const bool splat_first = sorts_splat_first(c->cfg.sort_algorithm);
    fp.splat_first = splat_first ? 1u : 0u;
    const bool bucket = c->cfg.sort_algorithm == GS_SORT_TILE_BUCKET;
    const float tile_share = c->grid_h ? (float)c->rows_owned / (float)c->grid_h : 1.0f;
    f.ordered = c->cfg.tile_order == GS_TILE_ORDER_LONGEST_FIRST;
    f.direct = c->cfg.record_timings >= 2;
    hipEvent_t* const pass_events = f.direct ? c->scatter_ev : nullptr;
    launch_project(fp, c->scene, c->scratch, st);
    launch_scan_blocks(fp, c->scratch, c->sort.params, c->ranges, c->sort.coarse, st);
    f.fixed = fp;
    if (splat_first) {
        // Nothing between the first scan and RenderGaussians depends on the camera: those kernels take a FrameParams
        // without it (and with a fixed helper counter, cleared by the first kernel of the chain), so their arguments
        // never change and the whole chain -- FindRanges included -- replays as ONE graph when no timers are asked for.
        FrameParams& fps = f.fixed;
        std::memset(fps.view, 0, sizeof(fps.view)); std::memset(fps.proj, 0, sizeof(fps.proj));
        std::memset(fps.cam_pos, 0, sizeof(fps.cam_pos));
        fps.sh_mode = 0u; fps.w_norm2 = 0.0f; fps.compact_out = 0u;
        fps.parity = 0u;
        // the frame's own depth passes (shrinking depth words, payload as wide as the tile ids) over the splat list in
        // half 1, then the tile-word passes over the emitted list in half 0
        c->runs[0] = {.capacity = c->n, .num_sort_bits = 32u, .start = 1, .params = c->scratch.aux_params,
                      .drop_depth_payload = true, .hi16 = c->hi16, .scatter_events = pass_events};
        c->runs[1] = {.capacity = c->capacity, .first_bit = 32u, .num_sort_bits = c->band_sort_bits, .coarse_pass = 8,
                      .drop_depth_payload = true, .hi16 = c->hi16, .share = tile_share,
                      .scatter_events = pass_events ? pass_events + 2 * sort_pass_count(c->runs[0], c->sort.digit_bits) : nullptr};
        c->num_runs = 2;
    } else {
        // The passes' arguments are fixed once resolution and tile rows are: captured once, replayed as a hipGraph.
        // Without timers FindRanges (same property) rides in the same graph.
        // fed counts (gs_sort.hip): for the contractual sorter, when the list is short.  The host enqueues a frame without
        // knowing its element count, so GS_COUNT_AUTO goes by the count of a recent frame, which k_scan_blocks leaves in
        // a pinned host word (nothing waits for it; none yet: a Count launch per pass); a change of mind re-captures
        // the graph.  Speed only: the sorted list is the same either way and at any length.
        bool fed = false;
        if (c->cfg.sort_algorithm == GS_SORT_RADIX4) {
            const uint32_t limit = kFedMaxGroups * (uint32_t)kSortTile;
            const uint32_t note = c->elems_note ? *(volatile const uint32_t*)c->elems_note : 0u;   // count + 1 of a recent frame
            fed = c->cfg.count_launches == GS_COUNT_FED ||
                  (c->cfg.count_launches == GS_COUNT_AUTO && note != 0u &&
                   note - 1u <= (c->sort_fed ? limit : limit - limit / 16u));
        }
        if (fed != c->sort_fed) {
            if (c->run_graph[0].exec || c->chain_graph.exec) HIP_TRY(c, hipStreamSynchronize(st));   // the graph may still be executing (rare: the mode flips)
            drop_sort_graph(c);
            c->sort_fed = fed;
        }
        // the bucket sorter runs the tile-word passes alone and carries the depth words through them
        c->runs[0] = {.capacity = c->capacity, .first_bit = bucket ? 32u : 0u, .num_sort_bits = c->band_sort_bits,
                      .drop_depth_payload = !bucket, .hi16 = c->hi16, .share = tile_share, .fed = fed,
                      .scatter_events = pass_events};
        c->num_runs = 1;
    }
    const Stage* stages = splat_first ? kSplatFirstFrame : bucket ? kBucketFrame : kPlainFrame;
    const size_t num_stages = splat_first ? std::size(kSplatFirstFrame) : bucket ? std::size(kBucketFrame) : std::size(kPlainFrame);
    // With timers (and for the bucket sorter) the stages go to the stream one by one, with a mark behind each.  Without:
    // everything from the first camera-free stage through FindRanges is ONE graph.
    for (size_t i = 0; i < num_stages; ++i) {
        const Stage& s = stages[i];
        const bool chain = !tm && s.camera_free;
        f.sorted = chain ? capture_or_replay(f, c->chain_graph, [&] {
                               for (size_t j = i; j < num_stages; ++j)
                                   if (launch_stage(f, stages[j], false) < 0) return -1;
                               return f.sorted;
                           })
                         : launch_stage(f, s, true);
        if (f.sorted < 0) return fail(c, GS_ERR_HIP, "gs_render: the radix passes could not be enqueued (hipGraphLaunch failed or the sort buffers cannot serve them)");
        if (int r = check_launch(c, chain ? "RadixSort" : s.name)) return r;
        if (chain) break;
        if (tm) if (int r = mark(c, s.bucket)) return r;
    }
    c->sorted_index = f.sorted;
    c->depth_dropped = !bucket;
    // computeRenderGaussians (Subrenderer.cpp:218-346), with the outputs of gs_set_outputs beside the image
    const RenderOutputs outs{reinterpret_cast<float4*>(c->out_rgba32f), c->out_depth, c->scratch.view_z};
    launch_render(fp, c->scratch.raster, c->sort.id[c->sorted_index], c->ranges, f.ordered ? c->tile_order : nullptr,
                  out_dev ? out_dev : c->framebuffer, c->cfg.render_mode, c->cfg.render_kernel, st, outs);
    if (int r = check_launch(c, "RenderGaussians")) return r;
    if (c->outputs) c->outputs_valid = true;
    if (tm) if (int r = mark(c, kBucketRender)) return r;
    c->have_frame = true;
    c->bwd_frame = true;
    return GS_OK;
}

double ms_since(HostClock::time_point t0) {
    return std::chrono::duration<double, std::milli>(HostClock::now() - t0).count();
}

// RECORD_CPU_TIMES (Renderer.cpp:299-314, 399-456): "CPU frame time" = entry of this draw - entry of the previous one
void host_frame_begin(gs_ctx* c) {
    const HostClock::time_point now = HostClock::now();
    c->host.cpu_frame_ms = c->have_entry ? (float)std::chrono::duration<double, std::milli>(now - c->last_entry).count() : 0.0f;
    c->last_entry = now;
    c->have_entry = true;
    c->host.wait_ms = 0.0f;
    c->host.present_ms = 0.0f;
}

// Renderer.cpp:458-475: wait, read the timestamps, compute the five buckets.
int finish_frame(gs_ctx* c) {
    const HostClock::time_point t_wait = HostClock::now();
    hipError_t sync_err = hipStreamSynchronize(c->stream);
    c->host.wait_ms = (float)ms_since(t_wait);       // the reference's waitForFences + waitIdle
    HIP_TRY(c, sync_err);
    SortParams sp{};
    HIP_TRY(c, hipMemcpy(&sp, c->sort.params, sizeof(sp), hipMemcpyDeviceToHost));
    gs_timings t{};
    if (c->cfg.record_timings && c->num_marks >= 2) {
        // every interval of the frame's timeline into the bucket its closing mark names; the total spans them all
        float* const bucket_ms[] = {nullptr, &t.init_sort_list_ms, &t.radix_sort_ms, &t.find_ranges_ms, &t.render_ms};
        for (uint32_t i = 1; i < c->num_marks; ++i) {
            float ms = 0.0f;
            HIP_TRY(c, hipEventElapsedTime(&ms, c->marks[i - 1], c->marks[i]));
            *bucket_ms[c->mark_bucket[i]] += ms;
        }
        HIP_TRY(c, hipEventElapsedTime(&t.total_ms, c->marks[0], c->marks[c->num_marks - 1]));
    }
    if (c->cfg.record_timings >= 2) {
        // [0]: the passes that move depth bytes (splat-first: over the SPLAT list, so per splat of that list); [1]: the
        // tile-word passes of a frame that leave the depth words behind.  Averaged apart.
        float sum_ms[2] = {}, sum_bytes[2] = {};
        uint32_t n[2] = {};
        for (uint32_t r = 0; r < c->num_runs; ++r) {
            const SortRun& run = c->runs[r];
            const uint32_t passes = sort_pass_count(run, c->sort.digit_bits);
            for (uint32_t k = 0; k < passes; ++k) {
                float ms = 0.0f;
                HIP_TRY(c, hipEventElapsedTime(&ms, run.scatter_events[2 * k], run.scatter_events[2 * k + 1]));
                const SortPass p = sort_pass(run, c->sort.digit_bits, k);
                const int which = p.lo_in == 0 && p.lo_out == 0 ? 1 : 0;
                sum_ms[which] += ms;
                sum_bytes[which] += (float)(p.lo_in + p.lo_out) + 2.0f * (run.hi16 ? 2.0f : 4.0f) + 8.0f;   // depth + tile + id, r + w
                ++n[which];
            }
        }
        t.scatter_launches = n[0];
        t.scatter_ms_avg = n[0] ? sum_ms[0] / (float)n[0] : 0.0f;
        t.scatter_bytes_per_elem = n[0] ? sum_bytes[0] / (float)n[0] : 0.0f;
        t.scatter_tile_launches = n[1];
        t.scatter_tile_ms_avg = n[1] ? sum_ms[1] / (float)n[1] : 0.0f;
        t.scatter_tile_bytes_per_elem = n[1] ? sum_bytes[1] / (float)n[1] : 0.0f;
    }
    t.num_sort_elements = sp.num_elems;
    t.overflowed = sp.overflow;
    t.emitted_elements = sp.counter;
    c->timings = t;
    return sp.overflow ? GS_WARN_OVERFLOW : GS_OK;
}

} // namespace

// gs_dist.cpp: the buckets and the element count of the frame gs_render_sharded has just waited for (hidden: not an export)
int gsi_finish_frame(gs_ctx* c) { return finish_frame(c); }

extern "C" {

uint32_t gs_api_version(void) { return GS_API_VERSION; }

int gs_runtime_versions(int* hip_build, int* hip_runtime, int* hip_driver) {
    if (hip_build) *hip_build = HIP_VERSION;
    int v = 0;
    if (hip_runtime) { if (hipRuntimeGetVersion(&v) != hipSuccess) return GS_ERR_HIP; *hip_runtime = v; }
    if (hip_driver) { if (hipDriverGetVersion(&v) != hipSuccess) return GS_ERR_HIP; *hip_driver = v; }
    return GS_OK;
}

void gs_default_config(gs_config* cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (uint32_t)sizeof(*cfg);
    cfg->device_ordinal = 0;
    cfg->tile_size = 16;            // Renderer.h:146
    cfg->near_plane = 0.1f;         // Camera.cpp:4
    cfg->far_plane = 100.0f;        // Camera.cpp:5
    cfg->ndc_cull = 1.3f;           // Common.glsl:5
    cfg->in_view_limit = 0.8f;      // Common.glsl:9
    cfg->fov_y = 3.1415f * 0.5f;    // Common.glsl:2
    cfg->sort_algorithm = GS_SORT_RADIX4;
    cfg->render_mode = GS_RENDER_EXACT;
    cfg->record_timings = 0;        // RECORD_GPU_TIMES is commented out in the reference (GfxSettings.h:7)
    cfg->render_kernel = GS_RENDER_KERNEL_AUTO;
    cfg->tile_order = GS_TILE_ORDER_LONGEST_FIRST;
    cfg->count_launches = GS_COUNT_AUTO;
}

// n events of gs_create (those created before a failure stay for gs_destroy) and their end in gs_destroy
static hipError_t create_events(hipEvent_t* ev, int n, unsigned flags) {
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ev[i], flags);
    return e;
}
static void destroy_events(hipEvent_t* ev, int n) {
    for (int i = 0; i < n; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]);
}

int gs_create(const gs_config* cfg_in, gs_ctx** out) {
    if (!out) return fail(nullptr, GS_ERR_INVALID, "gs_create: out is null");
    *out = nullptr;
    gs_config cfg;
    gs_default_config(&cfg);
    if (cfg_in) {
        // struct_size says how much of the struct the caller's header knows: fields beyond it keep their defaults, a
        // struct from a NEWER header than this library is refused instead of being read past what is understood
        if (cfg_in->struct_size < offsetof(gs_config, tile_order) + sizeof(uint32_t) || cfg_in->struct_size > sizeof(gs_config))
            return fail(nullptr, GS_ERR_INVALID, "gs_create: gs_config.struct_size does not match this library (call gs_default_config first; "
                                                 "compare GS_API_VERSION with gs_api_version())");
        std::memcpy(&cfg, cfg_in, cfg_in->struct_size);
        cfg.struct_size = (uint32_t)sizeof(cfg);
    }
    if (cfg.tile_size != 16) return fail(nullptr, GS_ERR_INVALID, "gs_create: only tile_size 16 is supported");
    if (cfg.sort_algorithm > GS_SORT_RADIX8_SPLAT_FIRST) return fail(nullptr, GS_ERR_INVALID, "gs_create: unknown sort_algorithm");
    if (cfg.render_mode > GS_RENDER_FAST) return fail(nullptr, GS_ERR_INVALID, "gs_create: unknown render_mode");
    if (cfg.render_kernel != GS_RENDER_KERNEL_AUTO && cfg.render_kernel != GS_RENDER_KERNEL_WAVE_1PX &&
        cfg.render_kernel != GS_RENDER_KERNEL_WAVE_2PX && cfg.render_kernel != GS_RENDER_KERNEL_WAVE_4PX &&
        cfg.render_kernel != GS_RENDER_KERNEL_WORKGROUP && cfg.render_kernel != GS_RENDER_KERNEL_WORKGROUP_8X8)
        return fail(nullptr, GS_ERR_INVALID, "gs_create: unknown render_kernel");
    if (cfg.tile_order > GS_TILE_ORDER_RASTER) return fail(nullptr, GS_ERR_INVALID, "gs_create: unknown tile_order");
    if (cfg.count_launches > GS_COUNT_FED) return fail(nullptr, GS_ERR_INVALID, "gs_create: unknown count_launches");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(nullptr, GS_ERR_NO_DEVICE,
                    "gs_create: no HIP device available (this library has no CPU fallback)");
    if (cfg.device_ordinal < 0 || cfg.device_ordinal >= count)
        return fail(nullptr, GS_ERR_INVALID, "gs_create: device_ordinal out of range");
    gs_ctx* c = new (std::nothrow) gs_ctx();
    if (!c) return fail(nullptr, GS_ERR_INVALID, "gs_create: out of host memory");
    c->cfg = cfg;
    c->device = cfg.device_ordinal;
    if ((e = hipSetDevice(c->device)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess) {
        std::string msg = std::string("gs_create: ") + hipGetErrorString(e);
        delete c;
        return fail(nullptr, GS_ERR_HIP, msg);
    }
    c->stream = c->own_stream;
    // a pinned host word the frames' k_scan_blocks writes their element count to (GS_COUNT_AUTO reads it when it enqueues
    // the next frame); doing without it is no error: the sort then keeps a Count launch per pass
    if (cfg.sort_algorithm == GS_SORT_RADIX4 && cfg.count_launches == GS_COUNT_AUTO) {
        void* note = nullptr;
        if (hipHostMalloc(&note, 64, hipHostMallocMapped) == hipSuccess && note) {
            c->elems_note = (uint32_t*)note;
            *c->elems_note = 0u;
        } else {
            (void)hipGetLastError();
        }
    }
    if (cfg.sort_algorithm == GS_SORT_TILE_BUCKET && init_tile_sort() != 0) {
        gs_destroy(c);
        return fail(nullptr, GS_ERR_HIP, "gs_create: cannot reserve 160 KB of LDS for the per-tile sort");
    }
    // the marks of a frame's timeline; a pair of events per radix pass only where they are recorded; the bucket sorter's
    // helper stream with its fork / join events
    e = create_events(c->marks, kMaxFrameMarks, hipEventDefault);
    if (e == hipSuccess && cfg.record_timings >= 2) e = create_events(c->scatter_ev, 32, hipEventDefault);
    if (e == hipSuccess && cfg.sort_algorithm == GS_SORT_TILE_BUCKET) {
        e = hipStreamCreateWithFlags(&c->helper_stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = create_events(&c->fork_ev, 1, hipEventDisableTiming);
        if (e == hipSuccess) e = create_events(&c->join_ev, 1, hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        std::string msg = std::string("gs_create: ") + hipGetErrorString(e);
        gs_destroy(c);
        return fail(nullptr, GS_ERR_HIP, msg);
    }
    *out = c;
    return GS_OK;
}

int gs_destroy(gs_ctx* c) {
    if (!c) return GS_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->dist_comm) (void)gs_dist_destroy(c);
    free_resolution(c);
    free_scene(c);
    c->densify_mem.release();
    destroy_events(c->marks, kMaxFrameMarks);
    destroy_events(c->scatter_ev, 32);
    destroy_events(&c->fork_ev, 1);
    destroy_events(&c->join_ev, 1);
    if (c->helper_stream) { (void)hipStreamSynchronize(c->helper_stream); (void)hipStreamDestroy(c->helper_stream); }
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->elems_note) (void)hipHostFree(c->elems_note);
    delete c;
    return GS_OK;
}

const char* gs_last_error(const gs_ctx* c) { return c ? c->last_error.c_str() : gsi_create_error.c_str(); }

int gs_set_stream(gs_ctx* c, void* hip_stream) {
    if (!c) return GS_ERR_INVALID;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return GS_OK;
}

// per-context, per-frame outputs of InitSortList's first kernel
static int alloc_scratch(gs_ctx* c, uint32_t n) {
    const size_t N = n;
    DeviceOwner& mem = c->scene_mem;
    SplatScratch& sc = c->scratch;
    hipStream_t st = c->stream;
    HIP_TRY(c, mem.alloc_zeroed(sc.raster, N * sizeof(SplatRaster), st));
    HIP_TRY(c, mem.alloc(sc.depth_key, N * sizeof(uint32_t)));
    HIP_TRY(c, mem.alloc(sc.tiles_touched, N * sizeof(uint32_t)));
    HIP_TRY(c, mem.alloc(sc.extents, N * sizeof(uint2)));
    c->num_blocks = (n + kProjThreads - 1) / kProjThreads;
    // k_scan_blocks reads/writes whole 16-byte groups up to 1024 * per entries: zero-padded
    const size_t padded = (size_t)c->num_blocks + 8192;
    HIP_TRY(c, mem.alloc_zeroed(sc.block_sums, padded * sizeof(uint32_t), st));
    HIP_TRY(c, mem.alloc_zeroed(sc.block_offsets, padded * sizeof(uint32_t), st));
    HIP_TRY(c, mem.alloc_zeroed(sc.wave_wrote, (size_t)c->num_blocks * 4, st));
    HIP_TRY(c, mem.alloc_zeroed(sc.help_list, (size_t)kEmitHelpCap * sizeof(uint2), st));
    HIP_TRY(c, mem.alloc_zeroed(sc.help_count, 4 * sizeof(uint32_t), st));
    sc.elems_note = nullptr;
    if (c->elems_note) {
        void* dev = nullptr;
        if (hipHostGetDevicePointer(&dev, c->elems_note, 0) == hipSuccess) sc.elems_note = (uint32_t*)dev;
        else (void)hipGetLastError();
    }
    HIP_TRY(c, mem.alloc(sc.band_list, (size_t)c->num_blocks * sizeof(uint32_t)));
    HIP_TRY(c, mem.alloc(sc.help_slot, (size_t)c->num_blocks * sizeof(uint32_t)));
    HIP_TRY(c, hipMemsetAsync(sc.help_slot, 0xFF, (size_t)c->num_blocks * sizeof(uint32_t), st));
    // k_project stores the view depths only while the depth output is on
    if (c->outputs & GS_OUTPUT_DEPTH) HIP_TRY(c, mem.alloc_zeroed(sc.view_z, N * sizeof(float), st));
    c->emit_parity = 0;
    if (sorts_splat_first(c->cfg.sort_algorithm)) {
        HIP_TRY(c, mem.alloc_zeroed(sc.block_flags, padded * sizeof(uint32_t), st));
        HIP_TRY(c, mem.alloc_zeroed(sc.flag_offsets, padded * sizeof(uint32_t), st));
        HIP_TRY(c, mem.alloc_zeroed(sc.sorted_sums, padded * sizeof(uint32_t), st));
        HIP_TRY(c, mem.alloc_zeroed(sc.aux_params, 2 * sizeof(SortParams), st));
    }
    return GS_OK;
}

// Frames in flight (GfxSettings::FRAMES_IN_FLIGHT = 3, GfxSettings.h:15): several contexts render the same scene
// on their own streams with their own per-frame buffers; only the read-only gaussian arrays are shared.
int gs_share_scene(gs_ctx* c, gs_ctx* owner) {
    if (!c || !owner || c == owner) return GS_ERR_INVALID;
    if (!owner->n || !owner->shared) return fail(c, GS_ERR_NO_SCENE, "gs_share_scene: the owner has no gaussians uploaded");
    if (owner->device != c->device) return fail(c, GS_ERR_INVALID, "gs_share_scene: contexts are on different devices");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    SharedScene* sh = owner->shared;
    sh->refs.fetch_add(1);            // taken first: c may currently hold the same arrays
    free_resolution(c);
    free_scene(c);
    c->shared = sh;
    c->scene = sh->b;
    if (int r = alloc_scratch(c, sh->n)) { free_scene(c); return r; }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->n = sh->n;
    return GS_OK;
}

// A fresh scene of n records on c: the arrays (shared with nobody yet) and the per-splat scratch; no resolution.
static int new_scene(gs_ctx* c, uint32_t n, const char* who) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    free_resolution(c);   // capacity depends on n (Renderer.cpp:725)
    free_scene(c);        // contexts that share the previous arrays keep them
    c->shared = new (std::nothrow) SharedScene();
    if (!c->shared) return fail(c, GS_ERR_INVALID, std::string(who) + ": out of host memory");
    c->shared->n = n;
    const size_t N = n;
    SceneBuffers& b = c->shared->b;
    DeviceOwner& mem = c->shared->mem;
    hipError_t e = mem.alloc(b.pos, 3 * N * sizeof(float));
    if (e == hipSuccess) e = mem.alloc(b.scale, 3 * N * sizeof(float));
    if (e == hipSuccess) e = mem.alloc(b.rot, 4 * N * sizeof(float));
    if (e == hipSuccess) e = mem.alloc(b.sh, 48 * N * sizeof(float));
    if (e == hipSuccess) e = mem.alloc(b.opacity, N * sizeof(float));
    if (e == hipSuccess) e = mem.alloc(b.sig2, N * sizeof(float));
    if (e == hipSuccess) e = mem.alloc(b.block_bounds, ((size_t)(n + 63u) / 64u + 4u) * 8 * sizeof(float));
    if (e != hipSuccess) {
        free_scene(c);
        return fail(c, GS_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
    c->scene = b;
    if (int r = alloc_scratch(c, n)) { free_scene(c); return r; }
    return GS_OK;
}

int gs_upload_gaussians(gs_ctx* c, const void* aos336, uint32_t n) {
    if (!c) return GS_ERR_INVALID;
    if (!aos336 || n == 0) return fail(c, GS_ERR_INVALID, "gs_upload_gaussians: empty input");
    if (int r = new_scene(c, n, "gs_upload_gaussians")) return r;

    // AoS -> SoA on the device, through a bounded staging buffer
    const uint32_t chunk = n < (1u << 20) ? n : (1u << 20);
    float* staging = nullptr;
    if (hipMalloc((void**)&staging, (size_t)chunk * GS_GAUSSIAN_RECORD_BYTES) != hipSuccess) {
        free_scene(c);
        return fail(c, GS_ERR_HIP, "gs_upload_gaussians: cannot allocate the staging buffer");
    }
    const char* src = static_cast<const char*>(aos336);
    int rc = GS_OK;
    for (uint32_t first = 0; first < n && rc == GS_OK; first += chunk) {
        const uint32_t cnt = (n - first) < chunk ? (n - first) : chunk;
        hipError_t e = hipMemcpyAsync(staging, src + (size_t)first * GS_GAUSSIAN_RECORD_BYTES,
                                      (size_t)cnt * GS_GAUSSIAN_RECORD_BYTES, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) {
            launch_aos_to_soa(staging, first, cnt, n, c->scene, c->stream);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // staging is reused
        if (e != hipSuccess) rc = fail(c, GS_ERR_HIP, std::string("gs_upload_gaussians: ") + hipGetErrorString(e));
    }
    (void)hipFree(staging);
    if (rc == GS_OK) {
        launch_block_bounds(n, c->scene, c->stream);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = fail(c, GS_ERR_HIP, std::string("gs_upload_gaussians: ") + hipGetErrorString(e));
    }
    if (rc != GS_OK) { free_scene(c); return rc; }
    c->n = n;
    return GS_OK;
}

int gs_upload_gaussians_device(gs_ctx* c, const void* aos336_dev, uint32_t n) {
    if (!c) return GS_ERR_INVALID;
    if (!aos336_dev || n == 0) return fail(c, GS_ERR_INVALID, "gs_upload_gaussians_device: empty input");
    HIP_TRY(c, hipSetDevice(c->device));
    const float* src = static_cast<const float*>(aos336_dev);
    if (c->shared && c->n == n) {
        // the same scene size: the planes are rewritten in place behind whatever is enqueued on the stream, and every
        // context that shares them renders the new values; resolution, scratch and captured graphs stay
        launch_aos_to_soa(src, 0, n, n, c->scene, c->stream);
        launch_block_bounds(n, c->scene, c->stream);
        c->bwd_frame = false; c->bwd_rows = false;
        HIP_TRY(c, hipGetLastError());
        return GS_OK;
    }
    if (int r = new_scene(c, n, "gs_upload_gaussians_device")) return r;
    launch_aos_to_soa(src, 0, n, n, c->scene, c->stream);
    launch_block_bounds(n, c->scene, c->stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        free_scene(c);
        return fail(c, GS_ERR_HIP, std::string("gs_upload_gaussians_device: ") + hipGetErrorString(e));
    }
    c->n = n;
    return GS_OK;
}

int gs_upload_rows_device(gs_ctx* c, const void* aos336_dev, uint32_t n, const uint32_t* ids_dev, const uint32_t* count_dev,
                          uint32_t max_rows) {
    if (!c) return GS_ERR_INVALID;
    if (max_rows && (!aos336_dev || !ids_dev || !count_dev))
        return fail(c, GS_ERR_INVALID, "gs_upload_rows_device: null aos336_dev, ids_dev or count_dev with max_rows > 0");
    if (n == 0) return fail(c, GS_ERR_INVALID, "gs_upload_rows_device: n is 0");
    if (!c->shared || !c->n) return fail(c, GS_ERR_NO_SCENE, "gs_upload_rows_device: no gaussians uploaded yet");
    if (c->n != n)
        return fail(c, GS_ERR_INVALID, "gs_upload_rows_device: n differs from the scene's (gs_upload_gaussians_device makes a new scene)");
    if (!max_rows) return GS_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    // the listed planes in place, then the boxes of all blocks (16 bytes per splat read): what the full in-place upload leaves
    launch_upload_rows(static_cast<const float*>(aos336_dev), n, ids_dev, count_dev, max_rows, c->scene, c->stream);
    launch_block_bounds(n, c->scene, c->stream);
    c->bwd_frame = false; c->bwd_rows = false;
    return check_launch(c, "gs_upload_rows_device");
}

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

// what gs_adam_rows_device and gs_adam_rows_raw_device check of their parameters, and the step they hand the kernel
static int adam_step_of(gs_ctx* c, const std::string& who, uint32_t n, const gs_adam_params* p, AdamStep& a) {
    if (!p) return fail(c, GS_ERR_INVALID, who + "null gs_adam_params");
    if (n == 0) return fail(c, GS_ERR_INVALID, who + "n is 0");
    if (p->struct_size != sizeof(gs_adam_params))
        return fail(c, GS_ERR_INVALID, who + "gs_adam_params.struct_size does not match this library (call gs_default_adam_params first)");
    if (p->step == 0) return fail(c, GS_ERR_INVALID, who + "step counts from 1");
    if (!(p->beta1 >= 0.0f && p->beta1 < 1.0f) || !(p->beta2 >= 0.0f && p->beta2 < 1.0f))
        return fail(c, GS_ERR_INVALID, who + "beta1 and beta2 must be in [0, 1)");
    if (!(p->eps >= 0.0f) || !std::isfinite(p->eps)) return fail(c, GS_ERR_INVALID, who + "eps must be finite and not negative");
    a.beta1 = p->beta1; a.beta2 = p->beta2; a.eps = p->eps;
    a.c1 = 1.0f - p->beta1; a.c2 = 1.0f - p->beta2;
    // the bias correction of step t in double, rounded once per group
    const double t = (double)p->step;
    const double root2 = std::sqrt(1.0 - std::pow((double)p->beta2, t)), bias1 = 1.0 - std::pow((double)p->beta1, t);
    for (int g = 0; g < GS_ADAM_GROUPS; ++g) {
        if (!(p->lr[g] >= 0.0f) || !std::isfinite(p->lr[g])) return fail(c, GS_ERR_INVALID, who + "lr must be finite and not negative");
        if (!(p->lo[g] <= p->hi[g])) return fail(c, GS_ERR_INVALID, who + "lo must not exceed hi, and neither may be a NaN");
        a.step[g] = (float)((double)p->lr[g] * root2 / bias1);
        if (!std::isfinite(a.step[g])) return fail(c, GS_ERR_INVALID, who + "lr times the bias correction is not a finite float");
        a.lo[g] = p->lo[g]; a.hi[g] = p->hi[g];
    }
    return GS_OK;
}

int gs_adam_rows_device(gs_ctx* c, float* records_dev, float* m_dev, float* v_dev, uint32_t n, const uint32_t* ids_dev,
                        const float* grad_rows_dev, const uint32_t* count_dev, uint32_t max_rows, const gs_adam_params* p) {
    if (!c) return GS_ERR_INVALID;
    const std::string who = "gs_adam_rows_device: ";
    if (max_rows && (!records_dev || !m_dev || !v_dev || !ids_dev || !grad_rows_dev || !count_dev))
        return fail(c, GS_ERR_INVALID, who + "null records, m, v, ids, grad_rows or count with max_rows > 0");
    AdamStep a;
    if (int r = adam_step_of(c, who, n, p, a)) return r;
    if (!max_rows) return GS_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    launch_adam_rows(records_dev, m_dev, v_dev, n, ids_dev, grad_rows_dev, count_dev, max_rows, a, c->stream);
    return check_launch(c, "gs_adam_rows_device");
}

// ---- the raw parameter space (gs_raw.hip) ----

// two arrays of `bytes` bytes share at least one (a null array shares nothing)
static bool arrays_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && bytes && a0 < b0 + bytes && b0 < a0 + bytes;
}

void gs_default_adam_params_raw(gs_adam_params* p) {
    if (!p) return;
    gs_default_adam_params(p);
    const float inf = std::numeric_limits<float>::infinity();
    for (int g = 0; g < GS_ADAM_GROUPS; ++g) { p->lo[g] = -inf; p->hi[g] = inf; }
}

int gs_adam_rows_raw_device(gs_ctx* c, float* raw_dev, float* records_dev, float* m_dev, float* v_dev, uint32_t n,
                            const uint32_t* ids_dev, const float* grad_rows_dev, const uint32_t* count_dev, uint32_t max_rows,
                            const gs_adam_params* p) {
    if (!c) return GS_ERR_INVALID;
    const std::string who = "gs_adam_rows_raw_device: ";
    if (max_rows && (!raw_dev || !records_dev || !m_dev || !v_dev || !ids_dev || !grad_rows_dev || !count_dev))
        return fail(c, GS_ERR_INVALID, who + "null raw, records, m, v, ids, grad_rows or count with max_rows > 0");
    AdamStep a;
    if (int r = adam_step_of(c, who, n, p, a)) return r;
    const size_t bytes = (size_t)n * GS_GAUSSIAN_RECORD_BYTES;
    if (arrays_overlap(records_dev, raw_dev, bytes) || arrays_overlap(records_dev, m_dev, bytes) || arrays_overlap(records_dev, v_dev, bytes))
        return fail(c, GS_ERR_INVALID, who + "records aliases raw, m or v");
    if (!max_rows) return GS_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    launch_adam_rows_raw(raw_dev, records_dev, m_dev, v_dev, n, ids_dev, grad_rows_dev, count_dev, max_rows, a, c->stream);
    return check_launch(c, "gs_adam_rows_raw_device");
}

static int convert_space(gs_ctx* c, const char* name, const float* src, float* dst, uint32_t n, bool to_raw) {
    if (!c) return GS_ERR_INVALID;
    const std::string who = std::string(name) + ": ";
    if (!src || !dst) return fail(c, GS_ERR_INVALID, who + "null raw or records");
    if (n == 0) return fail(c, GS_ERR_INVALID, who + "n is 0");
    if (arrays_overlap(src, dst, (size_t)n * GS_GAUSSIAN_RECORD_BYTES)) return fail(c, GS_ERR_INVALID, who + "raw aliases records");
    HIP_TRY(c, hipSetDevice(c->device));
    launch_convert_space(src, dst, n, to_raw, c->stream);
    return check_launch(c, name);
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
    const std::string who = "gs_reset_opacity_raw_device: ";
    if (!raw_dev || !records_dev) return fail(c, GS_ERR_INVALID, who + "null raw or records");
    if (!m_dev != !v_dev) return fail(c, GS_ERR_INVALID, who + "m and v must be given together or not at all");
    if (n == 0) return fail(c, GS_ERR_INVALID, who + "n is 0");
    if (!(max_opacity > 0.0f && max_opacity < 1.0f)) return fail(c, GS_ERR_INVALID, who + "max_opacity must lie strictly between 0 and 1");
    const float logit = (float)std::log((double)max_opacity / (1.0 - (double)max_opacity));
    HIP_TRY(c, hipSetDevice(c->device));
    launch_reset_opacity_raw(raw_dev, records_dev, m_dev, v_dev, n, max_opacity, logit, c->stream);
    return check_launch(c, "gs_reset_opacity_raw_device");
}

static hipError_t alloc_outputs(gs_ctx* c);

int gs_set_resolution(gs_ctx* c, uint32_t width, uint32_t height) {
    if (!c) return GS_ERR_INVALID;
    if (!c->n) return fail(c, GS_ERR_NO_SCENE, "gs_set_resolution: upload gaussians first");
    if (width == 0 || height == 0 || width > 65535u * 16u || height > 65535u * 16u)
        return fail(c, GS_ERR_INVALID, "gs_set_resolution: bad extent");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    free_resolution(c);
    const uint32_t gw = (width + kTile - 1) / kTile, gh = (height + kTile - 1) / kTile; // Renderer.cpp:696-701
    const uint64_t want = (uint64_t)c->n + 64ull * 16ull * gw * gh;                       // Renderer.cpp:725
    if (want > (1ull << 31)) return fail(c, GS_ERR_INVALID, "gs_set_resolution: sort list would exceed 2^31 elements");
    c->width = width; c->height = height; c->grid_w = gw; c->grid_h = gh;
    c->row_begin = 0; c->row_end = gh; c->row_stride = 1; c->first_row = 0; c->rows_owned = gh;
    c->compact_out = false;
    c->capacity = ceil_pow2((uint32_t)want);
    c->num_sort_bits = num_sort_bits_for(gw * gh);
    c->band_sort_bits = c->num_sort_bits;
    c->hi16 = (uint64_t)gw * gh <= 65535u;
    int rc = alloc_sort(c, c->res_mem, c->sort, c->capacity);
    if (rc != GS_OK) { free_resolution(c); return rc; }
    // any failure from here on leaves the context without a resolution (capacity 0), never half set up
    DeviceOwner& mem = c->res_mem;
    hipError_t e = mem.alloc(c->ranges, ((size_t)gw * gh * 2 * sizeof(uint32_t) + 15) & ~(size_t)15);   // cleared 16 bytes at a time
    if (e == hipSuccess) e = mem.alloc(c->tile_order, tile_order_words(gw, gh) * sizeof(uint32_t));   // table + scratch of the two kernels
    if (e == hipSuccess) e = mem.alloc(c->framebuffer, (size_t)width * height * 4);
    if (e == hipSuccess) e = hipMemset(c->ranges, 0, (size_t)gw * gh * 2 * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(c->framebuffer, 0, (size_t)width * height * 4);
    if (e == hipSuccess) e = alloc_outputs(c);
    if (e != hipSuccess) {
        free_resolution(c);
        return fail(c, GS_ERR_HIP, std::string("gs_set_resolution: ") + hipGetErrorString(e));
    }
    return GS_OK;
}

// The output buffers of the mask at the current resolution, zero-filled (rows a context does not own stay zero)
static hipError_t alloc_outputs(gs_ctx* c) {
    const size_t px = (size_t)c->width * c->height;
    hipError_t e = hipSuccess;
    if (px && (c->outputs & GS_OUTPUT_RGBA32F)) {
        e = c->res_mem.alloc(c->out_rgba32f, px * 4 * sizeof(float));
        if (e == hipSuccess) e = hipMemset(c->out_rgba32f, 0, px * 4 * sizeof(float));
    }
    if (e == hipSuccess && px && (c->outputs & GS_OUTPUT_DEPTH)) {
        e = c->res_mem.alloc(c->out_depth, px * sizeof(float));
        if (e == hipSuccess) e = hipMemset(c->out_depth, 0, px * sizeof(float));
    }
    return e;
}

// the three buffers of the mask, inside the lifetimes that hold them
static void free_outputs(gs_ctx* c) {
    c->res_mem.free(c->out_rgba32f);
    c->res_mem.free(c->out_depth);
    c->scene_mem.free(c->scratch.view_z);
}

int gs_set_outputs(gs_ctx* c, uint32_t mask) {
    if (!c) return GS_ERR_INVALID;
    if (mask & ~(GS_OUTPUT_RGBA32F | GS_OUTPUT_DEPTH)) return fail(c, GS_ERR_INVALID, "gs_set_outputs: unknown output bit in the mask");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // no frame in flight may still write the buffers
    // k_project and RenderGaussians are launched outside the captured graphs (enqueue_frame): no graph depends on the mask
    free_outputs(c);
    c->outputs = mask;
    c->outputs_valid = false;
    hipError_t e = hipSuccess;
    if (c->n && (mask & GS_OUTPUT_DEPTH)) {
        e = c->scene_mem.alloc(c->scratch.view_z, (size_t)c->n * sizeof(float));
        if (e == hipSuccess) e = hipMemset(c->scratch.view_z, 0, (size_t)c->n * sizeof(float));
    }
    if (e == hipSuccess) e = alloc_outputs(c);
    if (e != hipSuccess) {   // back to RGBA8-only frames rather than half set up
        free_outputs(c);
        c->outputs = 0;
        return fail(c, GS_ERR_HIP, std::string("gs_set_outputs: ") + hipGetErrorString(e));
    }
    return GS_OK;
}

// which: one GS_OUTPUT_* bit that is enabled and allocated -> its buffer and size; else fails
static int output_buffer(gs_ctx* c, uint32_t which, const char* who, void** dev, size_t* size) {
    if (which != GS_OUTPUT_RGBA32F && which != GS_OUTPUT_DEPTH)
        return fail(c, GS_ERR_INVALID, std::string(who) + ": which must be GS_OUTPUT_RGBA32F or GS_OUTPUT_DEPTH");
    if (!(c->outputs & which)) return fail(c, GS_ERR_INVALID, std::string(who) + ": that output is not enabled (gs_set_outputs)");
    if (!c->capacity) return fail(c, GS_ERR_INVALID, std::string(who) + ": gs_set_resolution not called");
    const size_t px = (size_t)c->width * c->height;
    *dev = which == GS_OUTPUT_RGBA32F ? (void*)c->out_rgba32f : (void*)c->out_depth;
    *size = px * (which == GS_OUTPUT_RGBA32F ? 4 * sizeof(float) : sizeof(float));
    return GS_OK;
}

int gs_read_output(gs_ctx* c, uint32_t which, void* dst, size_t bytes) {
    if (!c) return GS_ERR_INVALID;
    if (!dst) return fail(c, GS_ERR_INVALID, "gs_read_output: dst is null");
    void* dev = nullptr;
    size_t size = 0;
    if (int r = output_buffer(c, which, "gs_read_output", &dev, &size)) return r;
    if (!c->outputs_valid)
        return fail(c, GS_ERR_INVALID, "gs_read_output: no frame rendered since the outputs were enabled or resized");
    if (bytes < size) return fail(c, GS_ERR_INVALID, "gs_read_output: bytes is smaller than the buffer (H * W * 16 or H * W * 4)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(dst, dev, size, hipMemcpyDeviceToHost));
    return GS_OK;
}

int gs_output_device(gs_ctx* c, uint32_t which, void** dev_out, size_t* bytes) {
    if (!c) return GS_ERR_INVALID;
    if (!dev_out) return fail(c, GS_ERR_INVALID, "gs_output_device: dev_out is null");
    *dev_out = nullptr;
    void* dev = nullptr;
    size_t size = 0;
    if (int r = output_buffer(c, which, "gs_output_device", &dev, &size)) return r;
    if (!c->outputs_valid)
        return fail(c, GS_ERR_INVALID, "gs_output_device: no frame rendered since the outputs were enabled or resized");
    *dev_out = dev;
    if (bytes) *bytes = size;
    return GS_OK;
}

// The buffers of a per-splat scan (gs_splat_scan.h) of K sums over n splats, into the lifetime `mem`
static hipError_t alloc_splat_scan(DeviceOwner& mem, SplatScan& s, uint32_t n, uint32_t K) {
    const size_t rows = (size_t)K * backward_blocks(n) * sizeof(uint32_t);
    hipError_t e = mem.alloc(s.offsets, (size_t)n * sizeof(uint32_t));
    if (e == hipSuccess) e = mem.alloc(s.block_sums, rows);
    if (e == hipSuccess) e = mem.alloc(s.block_offsets, rows);
    if (e == hipSuccess) e = mem.alloc(s.totals, K * sizeof(uint32_t));
    return e;
}

// gs_backward*: the refusals (nothing enqueued), then the scratch of the first call
static int backward_prepare(gs_ctx* c, const char* who) {
    if (c->cfg.render_mode != GS_RENDER_EXACT)
        return fail(c, GS_ERR_INVALID, std::string(who) + ": only GS_RENDER_EXACT frames can be differentiated");
    if (c->dist_sharded)
        return fail(c, GS_ERR_INVALID, std::string(who) + ": a sharded context (gs_dist_shard_rows) cannot be differentiated");
    if (!c->capacity || !c->n || !c->bwd_frame)
        return fail(c, GS_ERR_INVALID, std::string(who) + ": no frame since the last gs_set_resolution, gs_set_tile_rows* or upload");
    if (c->row_begin != 0u || c->row_end != c->grid_h || c->row_stride != 1u)
        return fail(c, GS_ERR_INVALID, std::string(who) + ": the context owns a subset of the tile rows");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->bwd.rows) {
        DeviceOwner& mem = c->bwd_mem;
        hipError_t e = mem.alloc(c->bwd.rows, backward_row_bytes(c->capacity));
        if (e == hipSuccess) e = alloc_splat_scan(mem, c->bwd.scan, c->n, 2);
        if (e == hipSuccess) e = mem.alloc(c->bwd.vis_ids, (size_t)c->n * sizeof(uint32_t));
        if (e != hipSuccess) {
            mem.release();
            c->bwd_vis_rows = 0;
            c->bwd_rows = false;
            return fail(c, GS_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
        }
    }
    return GS_OK;
}

// The last frame as the backward launchers take it
static BackwardFrame backward_frame(const gs_ctx* c) {
    return BackwardFrame{c->last_fp, c->scene, c->scratch, c->sort.id[c->sorted_index], c->ranges, c->bwd};
}

// Host gradients onto the device (bwd_host_in, allocated on first use), enqueued on the context's stream: the two host
// pointers are replaced by their device copies (a null grad_depth stays null)
static int stage_host_grads(gs_ctx* c, const float*& grad_rgba32f, const float*& grad_depth) {
    const size_t px = (size_t)c->width * c->height;
    if (!c->bwd_host_in) HIP_TRY(c, c->bwd_mem.alloc(c->bwd_host_in, px * 5 * sizeof(float)));
    float* din = c->bwd_host_in;
    HIP_TRY(c, hipMemcpyAsync(din, grad_rgba32f, px * 4 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (grad_depth) HIP_TRY(c, hipMemcpyAsync(din + px * 4, grad_depth, px * sizeof(float), hipMemcpyHostToDevice, c->stream));
    grad_rgba32f = din;
    if (grad_depth) grad_depth = din + px * 4;
    return GS_OK;
}

// V of the last frame into bwd.vis_ids and |V| into *count, on the host: the scan, then a wait for the stream
static int visible_count_sync(gs_ctx* c, const char* who, uint32_t* count) {
    launch_backward_visible_scan(backward_frame(c), nullptr, 0u, nullptr, c->stream);
    if (int r = check_launch(c, who)) return r;
    HIP_TRY(c, hipMemcpyAsync(count, visible_count_of(c->bwd), 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GS_OK;
}

int gs_backward_device(gs_ctx* c, const float* grad_rgba32f, const float* grad_depth, float* grad_records) {
    if (!c) return GS_ERR_INVALID;
    if (!grad_rgba32f || !grad_records) return fail(c, GS_ERR_INVALID, "gs_backward_device: null gradient pointer");
    if (int r = backward_prepare(c, "gs_backward_device")) return r;
    launch_backward(backward_frame(c), grad_rgba32f, grad_depth, grad_records, c->stream);
    c->bwd_rows = true;
    return check_launch(c, "gs_backward_device");
}

int gs_backward(gs_ctx* c, const float* grad_rgba32f, const float* grad_depth, float* grad_records) {
    if (!c) return GS_ERR_INVALID;
    if (!grad_rgba32f || !grad_records) return fail(c, GS_ERR_INVALID, "gs_backward: null gradient pointer");
    if (int r = backward_prepare(c, "gs_backward")) return r;
    if (!c->bwd_host_out) HIP_TRY(c, c->bwd_mem.alloc(c->bwd_host_out, (size_t)c->n * GS_GAUSSIAN_RECORD_BYTES));
    if (int r = stage_host_grads(c, grad_rgba32f, grad_depth)) return r;
    launch_backward(backward_frame(c), grad_rgba32f, grad_depth, c->bwd_host_out, c->stream);
    c->bwd_rows = true;
    if (int r = check_launch(c, "gs_backward")) return r;
    HIP_TRY(c, hipMemcpyAsync(grad_records, c->bwd_host_out, (size_t)c->n * GS_GAUSSIAN_RECORD_BYTES, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GS_OK;
}

// gs_photometric_loss*: the refusals (nothing enqueued), the image the call reads (rgba32f, or the context's own
// GS_OUTPUT_RGBA32F buffer for NULL), then the scratch of the first call
static int loss_prepare(gs_ctx* c, const char* who, const float*& rgba32f, const float* target_rgb, float lambda,
                        const float* bg, const float* loss_out, const float* grad_rgba32f) {
    if (!target_rgb || !loss_out) return fail(c, GS_ERR_INVALID, std::string(who) + ": null target_rgb or loss_out");
    if (!(lambda >= 0.0f && lambda <= 1.0f)) return fail(c, GS_ERR_INVALID, std::string(who) + ": lambda must be a finite value in [0, 1]");
    if (bg && !(std::isfinite(bg[0]) && std::isfinite(bg[1]) && std::isfinite(bg[2])))
        return fail(c, GS_ERR_INVALID, std::string(who) + ": bg must be finite");
    if (!c->capacity) return fail(c, GS_ERR_INVALID, std::string(who) + ": gs_set_resolution not called");
    if (c->dist_sharded)
        return fail(c, GS_ERR_INVALID, std::string(who) + ": a sharded context (gs_dist_shard_rows) has no whole frame to compare");
    if (c->row_begin != 0u || c->row_end != c->grid_h || c->row_stride != 1u)
        return fail(c, GS_ERR_INVALID, std::string(who) + ": the context owns a subset of the tile rows");
    if (!rgba32f) {
        void* dev = nullptr;
        size_t size = 0;
        if (int r = output_buffer(c, GS_OUTPUT_RGBA32F, who, &dev, &size)) return r;
        if (!c->outputs_valid)
            return fail(c, GS_ERR_INVALID, std::string(who) + ": no frame rendered since the outputs were enabled or resized");
        rgba32f = static_cast<const float*>(dev);
    }
    if (grad_rgba32f && grad_rgba32f == rgba32f)
        return fail(c, GS_ERR_INVALID, std::string(who) + ": grad_rgba32f must not be the image it differentiates");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->loss.maps) {
        hipError_t e = c->loss_mem.alloc(c->loss.maps, loss_map_bytes(c->width, c->height));
        if (e == hipSuccess) e = c->loss_mem.alloc(c->loss.tile_sums, loss_tile_bytes(c->width, c->height));
        if (e != hipSuccess) {
            c->loss_mem.release();
            return fail(c, GS_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
        }
    }
    return GS_OK;
}

int gs_photometric_loss_device(gs_ctx* c, const float* rgba32f, const float* target_rgb, float lambda, const float bg[3],
                               float* loss_out, float* grad_rgba32f) {
    if (!c) return GS_ERR_INVALID;
    if (int r = loss_prepare(c, "gs_photometric_loss_device", rgba32f, target_rgb, lambda, bg, loss_out, grad_rgba32f)) return r;
    launch_photometric_loss(c->loss, rgba32f, target_rgb, lambda, bg, c->width, c->height, loss_out, grad_rgba32f, c->stream);
    return check_launch(c, "gs_photometric_loss_device");
}

int gs_photometric_loss(gs_ctx* c, const float* rgba32f, const float* target_rgb, float lambda, const float bg[3],
                        float loss_out[3], float* grad_rgba32f) {
    if (!c) return GS_ERR_INVALID;
    const float* image = rgba32f;      // host, or (NULL form) the context's device buffer after loss_prepare
    if (int r = loss_prepare(c, "gs_photometric_loss", image, target_rgb, lambda, bg, loss_out, grad_rgba32f)) return r;
    // device copies: rgba [px][4] | gradient [px][4] | target [px][3] | the three numbers (+ 1: 16-byte multiples)
    const size_t px = (size_t)c->width * c->height;
    if (!c->loss_host) HIP_TRY(c, c->loss_mem.alloc(c->loss_host, (px * 11 + 4) * sizeof(float)));
    float* d_rgba = c->loss_host, *d_grad = d_rgba + px * 4, *d_target = d_grad + px * 4, *d_loss = d_target + px * 3;
    if (rgba32f) {
        HIP_TRY(c, hipMemcpyAsync(d_rgba, rgba32f, px * 4 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        image = d_rgba;
    }
    HIP_TRY(c, hipMemcpyAsync(d_target, target_rgb, px * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    launch_photometric_loss(c->loss, image, d_target, lambda, bg, c->width, c->height, d_loss, grad_rgba32f ? d_grad : nullptr,
                            c->stream);
    if (int r = check_launch(c, "gs_photometric_loss")) return r;
    HIP_TRY(c, hipMemcpyAsync(loss_out, d_loss, 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (grad_rgba32f) HIP_TRY(c, hipMemcpyAsync(grad_rgba32f, d_grad, px * 4 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GS_OK;
}

int gs_visible_count(gs_ctx* c, uint32_t* count_out) {
    if (!c) return GS_ERR_INVALID;
    if (!count_out) return fail(c, GS_ERR_INVALID, "gs_visible_count: null count_out");
    if (int r = backward_prepare(c, "gs_visible_count")) return r;
    return visible_count_sync(c, "gs_visible_count", count_out);
}

static int backward_visible_refusals(gs_ctx* c, const char* who, const float* grad_rgba32f, const uint32_t* ids_out,
                                     const float* grad_rows_out, uint32_t max_rows, const uint32_t* count_out) {
    if (!grad_rgba32f) return fail(c, GS_ERR_INVALID, std::string(who) + ": null gradient pointer");
    if (!count_out) return fail(c, GS_ERR_INVALID, std::string(who) + ": null count_out");
    if (max_rows && (!ids_out || !grad_rows_out))
        return fail(c, GS_ERR_INVALID, std::string(who) + ": null ids_out or grad_rows_out with max_rows > 0");
    return backward_prepare(c, who);
}

int gs_backward_visible_device(gs_ctx* c, const float* grad_rgba32f, const float* grad_depth, uint32_t* ids_out,
                               float* grad_rows_out, uint32_t max_rows, uint32_t* count_out) {
    if (!c) return GS_ERR_INVALID;
    if (int r = backward_visible_refusals(c, "gs_backward_visible_device", grad_rgba32f, ids_out, grad_rows_out, max_rows, count_out))
        return r;
    const BackwardFrame f = backward_frame(c);
    launch_backward_visible_scan(f, ids_out, max_rows, count_out, c->stream);
    if (max_rows) {
        launch_backward_visible_rows(f, grad_rgba32f, grad_depth, max_rows, grad_rows_out, c->stream);
        c->bwd_rows = true;
    }
    return check_launch(c, "gs_backward_visible_device");
}

int gs_backward_visible(gs_ctx* c, const float* grad_rgba32f, const float* grad_depth, uint32_t* ids_out,
                        float* grad_rows_out, uint32_t max_rows, uint32_t* count_out) {
    if (!c) return GS_ERR_INVALID;
    if (int r = backward_visible_refusals(c, "gs_backward_visible", grad_rgba32f, ids_out, grad_rows_out, max_rows, count_out))
        return r;
    // V and its size first (the count has to reach the host anyway), then exactly min(|V|, max_rows) rows
    if (int r = visible_count_sync(c, "gs_backward_visible", count_out)) return r;
    const uint32_t count = *count_out, k = count < max_rows ? count : max_rows;
    if (k) {
        if (c->bwd_vis_rows < k) {
            c->bwd_mem.free(c->bwd_vis_out);
            c->bwd_vis_rows = 0;
            HIP_TRY(c, c->bwd_mem.alloc(c->bwd_vis_out, (size_t)k * GS_GAUSSIAN_RECORD_BYTES));
            c->bwd_vis_rows = k;
        }
        if (int r = stage_host_grads(c, grad_rgba32f, grad_depth)) return r;
        launch_backward_visible_rows(backward_frame(c), grad_rgba32f, grad_depth, k, c->bwd_vis_out, c->stream);
        c->bwd_rows = true;
        if (int r = check_launch(c, "gs_backward_visible")) return r;
        HIP_TRY(c, hipMemcpyAsync(ids_out, c->bwd.vis_ids, (size_t)k * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(grad_rows_out, c->bwd_vis_out, (size_t)k * GS_GAUSSIAN_RECORD_BYTES, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    const bool count_only = !max_rows && !ids_out && !grad_rows_out;      // asked for no row: none is missing
    return count > max_rows && !count_only ? GS_WARN_OVERFLOW : GS_OK;
}

int gs_densify_stats_device(gs_ctx* c, const uint32_t* ids_dev, const uint32_t* count_dev, uint32_t max_rows, uint32_t n,
                            float* grad_accum, uint32_t* seen, float* max_radius) {
    if (!c) return GS_ERR_INVALID;
    const std::string who = "gs_densify_stats_device";
    if (max_rows && (!ids_dev || !count_dev || !grad_accum || !seen || !max_radius))
        return fail(c, GS_ERR_INVALID, who + ": null ids, count, grad_accum, seen or max_radius with max_rows > 0");
    if (int r = backward_prepare(c, who.c_str())) return r;
    if (!c->bwd_rows) return fail(c, GS_ERR_INVALID, who + ": no gs_backward* on this frame");
    if (n != c->n) return fail(c, GS_ERR_INVALID, who + ": n differs from the scene's");
    if (!max_rows) return GS_OK;
    const DensifyStatsArgs a{ids_dev, count_dev, max_rows, n, c->scratch.tiles_touched, c->bwd.scan.offsets, c->bwd.rows,
                             c->scratch.raster, c->last_fp.capacity, c->last_fp.width, c->last_fp.height,
                             grad_accum, seen, max_radius};
    launch_densify_stats(a, c->stream);
    return check_launch(c, who.c_str());
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

// the scratch of gs_densify_device for n splats, kept from call to call and grown when a larger cloud comes
static int densify_scratch(gs_ctx* c, uint32_t n, const std::string& who) {
    if (c->densify_cap >= n) return GS_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // an earlier call may still be running on the old arrays
    DeviceOwner& mem = c->densify_mem;
    mem.release();
    c->densify_cap = 0;
    const hipError_t e = alloc_splat_scan(mem, c->densify_scan, n, 4);
    if (e != hipSuccess) {
        mem.release();
        return fail(c, GS_ERR_HIP, who + hipGetErrorString(e));
    }
    c->densify_cap = n;
    return GS_OK;
}

int gs_densify_device(gs_ctx* c, const float* records, const float* m, const float* v, uint32_t n, const float* grad_accum,
                      const uint32_t* seen, const float* max_radius, const gs_densify_params* p, float* records_out,
                      float* m_out, float* v_out, uint32_t max_out, uint32_t* counts_out) {
    if (!c) return GS_ERR_INVALID;
    const std::string who = "gs_densify_device: ";
    if (!records || !grad_accum || !seen || !max_radius || !counts_out)
        return fail(c, GS_ERR_INVALID, who + "null records, grad_accum, seen, max_radius or counts_out");
    if (max_out && !records_out) return fail(c, GS_ERR_INVALID, who + "null records_out with max_out > 0");
    if (!p) return fail(c, GS_ERR_INVALID, who + "null gs_densify_params");
    if (n == 0) return fail(c, GS_ERR_INVALID, who + "n is 0");
    if (n >= 0x80000000u) return fail(c, GS_ERR_INVALID, who + "n must be below 2^31 (the outputs are counted in 32 bits)");
    if (p->struct_size != sizeof(gs_densify_params))
        return fail(c, GS_ERR_INVALID, who + "gs_densify_params.struct_size does not match this library (call gs_default_densify_params first)");
    if (p->grad_threshold != p->grad_threshold) return fail(c, GS_ERR_INVALID, who + "grad_threshold is a NaN");
    if (!(p->split_shrink > 0.0f)) return fail(c, GS_ERR_INVALID, who + "split_shrink must be greater than 0");
    const bool moments = m || v || m_out || v_out;
    if (moments && !(m && v && (!max_out || (m_out && v_out))))
        return fail(c, GS_ERR_INVALID, who + "m, v, m_out and v_out must be given all together or not at all");
    // no output may share bytes with an input, or with another output
    struct Span { const void* at; size_t bytes; };
    const size_t in_bytes = (size_t)n * GS_GAUSSIAN_RECORD_BYTES, out_bytes = (size_t)max_out * GS_GAUSSIAN_RECORD_BYTES;
    const Span ins[] = {{records, in_bytes}, {m, in_bytes}, {v, in_bytes}, {grad_accum, (size_t)n * 4}, {seen, (size_t)n * 4},
                        {max_radius, (size_t)n * 4}};
    const Span outs[] = {{records_out, out_bytes}, {m_out, out_bytes}, {v_out, out_bytes}, {counts_out, 16}};
    auto overlap = [](const Span& a, const Span& b) {
        const uintptr_t a0 = (uintptr_t)a.at, b0 = (uintptr_t)b.at;
        return a.at && b.at && a.bytes && b.bytes && a0 < b0 + b.bytes && b0 < a0 + a.bytes;
    };
    for (const Span& o : outs)
        for (const Span& i : ins)
            if (overlap(o, i)) return fail(c, GS_ERR_INVALID, who + "an output array aliases an input");
    for (size_t o = 0; o < std::size(outs); ++o)
        for (size_t k = o + 1; k < std::size(outs); ++k)
            if (overlap(outs[o], outs[k])) return fail(c, GS_ERR_INVALID, who + "two output arrays alias each other");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = densify_scratch(c, n, who)) return r;
    DensifyArgs a{};
    a.records = records; a.m = m; a.v = v; a.n = n;
    a.grad_accum = grad_accum; a.seen = seen; a.max_radius = max_radius;
    a.rule = DensifyRule{p->grad_threshold, p->split_scale, p->prune_opacity, p->prune_scale, p->prune_radius};
    a.split_shrink = p->split_shrink; a.seed = p->seed;
    a.records_out = records_out; a.m_out = m_out; a.v_out = v_out; a.max_out = max_out;
    a.scan = c->densify_scan;
    launch_densify(a, counts_out, c->stream);
    return check_launch(c, "gs_densify_device");
}

static int apply_tile_rows(gs_ctx* c, uint32_t row_begin, uint32_t row_end, uint32_t stride, uint32_t phase,
                           bool compact_out) {
    c->row_begin = row_begin; c->row_end = row_end; c->row_stride = stride;
    c->first_row = row_begin + phase;
    c->rows_owned = c->first_row < row_end ? (row_end - c->first_row + stride - 1u) / stride : 0u;
    c->compact_out = compact_out;
    c->bwd_frame = false; c->bwd_rows = false;
    if (c->elems_note) {           // another band: another list length (GS_COUNT_AUTO learns it from the next frame)
        HIP_TRY(c, hipStreamSynchronize(c->stream));   // no frame in flight may still write the old one
        *(volatile uint32_t*)c->elems_note = 0u;
    }
    const uint32_t owned_tiles = c->rows_owned * c->grid_w;
    c->band_sort_bits = num_sort_bits_for(owned_tiles ? owned_tiles : 1u);
    c->hi16 = owned_tiles <= 65535u;
    if (c->run_graph[0].exec || c->run_graph[1].exec || c->chain_graph.exec) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));   // the graph may still be executing
        drop_sort_graph(c);
    }
    return GS_OK;
}

int gs_set_tile_rows(gs_ctx* c, uint32_t row_begin, uint32_t row_end) {
    if (!c) return GS_ERR_INVALID;
    if (!c->capacity) return fail(c, GS_ERR_NO_SCENE, "gs_set_tile_rows: gs_set_resolution not called");
    if (row_begin > row_end || row_end > c->grid_h)
        return fail(c, GS_ERR_INVALID, "gs_set_tile_rows: need row_begin <= row_end <= tiles_y");
    return apply_tile_rows(c, row_begin, row_end, 1u, 0u, false);
}

int gs_set_tile_rows_interleaved(gs_ctx* c, uint32_t phase, uint32_t stride, uint32_t compact_output) {
    if (!c) return GS_ERR_INVALID;
    if (!c->capacity) return fail(c, GS_ERR_NO_SCENE, "gs_set_tile_rows_interleaved: gs_set_resolution not called");
    if (stride == 0u || phase >= stride)
        return fail(c, GS_ERR_INVALID, "gs_set_tile_rows_interleaved: need 0 <= phase < stride");
    return apply_tile_rows(c, 0u, c->grid_h, stride, phase, compact_output != 0u);
}

int gs_get_scene_info(const gs_ctx* c, gs_scene_info* out) {
    if (!c || !out) return GS_ERR_INVALID;
    out->num_gaussians = c->n;
    out->width = c->width; out->height = c->height;
    out->tiles_x = c->grid_w; out->tiles_y = c->grid_h;
    out->capacity = c->capacity; out->num_sort_bits = c->num_sort_bits;
    out->row_begin = c->row_begin; out->row_end = c->row_end;
    out->tile_word_bytes = c->hi16 ? 2u : 4u;
    out->row_stride = c->row_stride; out->first_row = c->first_row; out->rows_owned = c->rows_owned;
    return GS_OK;
}

int gs_render_device_async(gs_ctx* c, const float view[16], const float proj[16],
                           const float cam_pos[3], uint32_t sh_mode, void* rgba_out_device) {
    if (!c) return GS_ERR_INVALID;
    host_frame_begin(c);
    HIP_TRY(c, hipSetDevice(c->device));
    const HostClock::time_point t_rec = HostClock::now();
    const int rc = enqueue_frame(c, view, proj, cam_pos, sh_mode, static_cast<uint8_t*>(rgba_out_device));
    c->host.record_ms = (float)ms_since(t_rec);      // recordCommandBuffer + submit
    return rc;
}

int gs_render_device(gs_ctx* c, const float view[16], const float proj[16], const float cam_pos[3],
                     uint32_t sh_mode, void* rgba_out_device) {
    int rc = gs_render_device_async(c, view, proj, cam_pos, sh_mode, rgba_out_device);
    if (rc != GS_OK) return rc;
    return finish_frame(c);
}

int gs_render(gs_ctx* c, const float view[16], const float proj[16], const float cam_pos[3],
              uint32_t sh_mode, uint8_t* rgba_out) {
    if (!c) return GS_ERR_INVALID;
    if (!rgba_out) return fail(c, GS_ERR_INVALID, "gs_render: rgba_out is null");
    int rc = gs_render_device_async(c, view, proj, cam_pos, sh_mode, nullptr);
    if (rc != GS_OK) return rc;
    rc = finish_frame(c);
    if (rc < 0) return rc;
    const HostClock::time_point t_present = HostClock::now();
    hipError_t e = hipMemcpy(rgba_out, c->framebuffer, (size_t)c->width * c->height * 4, hipMemcpyDeviceToHost);
    c->host.present_ms = (float)ms_since(t_present);   // where the reference presents, this sink copies the frame out
    HIP_TRY(c, e);
    return rc;
}

int gs_debug_init_sort_list(gs_ctx* c, const float view[16], const float proj[16],
                            const float cam_pos[3], uint32_t sh_mode) {
    if (!c) return GS_ERR_INVALID;
    if (!c->n || !c->capacity) return fail(c, GS_ERR_NO_SCENE, "gs_debug_init_sort_list: scene/resolution not set");
    if (!view || !proj || !cam_pos || sh_mode > 2u) return fail(c, GS_ERR_INVALID, "gs_debug_init_sort_list: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    FrameParams fp = make_frame_params(c, view, proj, cam_pos, sh_mode);
    fp.parity = (c->emit_parity ^= 1u);
    c->last_fp = fp;
    c->bwd_frame = false; c->bwd_rows = false;
    launch_project(fp, c->scene, c->scratch, c->stream);
    launch_scan_blocks(fp, c->scratch, c->sort.params, c->ranges, c->sort.coarse, c->stream);
    launch_emit(fp, c->scratch, c->sort, c->stream);
    if (int r = check_launch(c, "InitSortList")) return r;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->have_frame = false;
    c->unsorted_valid = true;
    SortParams sp{};
    HIP_TRY(c, hipMemcpy(&sp, c->sort.params, sizeof(sp), hipMemcpyDeviceToHost));
    return sp.overflow ? GS_WARN_OVERFLOW : GS_OK;
}

int gs_synchronize(gs_ctx* c) {
    if (!c) return GS_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GS_OK;
}

int gs_get_timings(const gs_ctx* c, gs_timings* out) {
    if (!c || !out) return GS_ERR_INVALID;
    *out = c->timings;
    return GS_OK;
}

int gs_get_host_timings(const gs_ctx* c, gs_host_timings* out) {
    if (!c || !out) return GS_ERR_INVALID;
    *out = c->host;
    return GS_OK;
}

// The sort list holds compact tile ids (uint16 or uint32, FrameParams) -> the uint32 GLOBAL tile ids callers expect
static int read_tile_words(gs_ctx* c, const uint32_t* dev, uint32_t num_elems, void* dst, size_t bytes) {
    if (bytes > (size_t)num_elems * sizeof(uint32_t)) return fail(c, GS_ERR_INVALID, "gs_debug_read: size exceeds buffer");
    const size_t cnt = bytes / sizeof(uint32_t);
    uint32_t* out = static_cast<uint32_t*>(dst);
    if (c->hi16) {
        std::vector<uint16_t> h(num_elems);
        if (num_elems) HIP_TRY(c, hipMemcpy(h.data(), dev, (size_t)num_elems * sizeof(uint16_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < cnt; ++i) out[i] = h[i];
    } else if (cnt) {
        HIP_TRY(c, hipMemcpy(out, dev, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i < cnt; ++i) {
        const uint32_t k = out[i] / c->grid_w, x = out[i] - k * c->grid_w;
        out[i] = (c->first_row + k * c->row_stride) * c->grid_w + x;
    }
    return GS_OK;
}

int gs_debug_read(gs_ctx* c, int which, void* dst, size_t bytes) {
    if (!c || !dst) return GS_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!c->have_frame && !c->unsorted_valid && which != GS_BUF_IMAGE) return fail(c, GS_ERR_NO_SCENE, "gs_debug_read: no frame rendered yet");
    SortParams sp{};
    HIP_TRY(c, hipMemcpy(&sp, c->sort.params, sizeof(sp), hipMemcpyDeviceToHost));
    const size_t e_bytes = (size_t)sp.num_elems * sizeof(uint32_t);
    const void* src = nullptr;
    size_t avail = 0;
    const int si = c->sorted_index;
    switch (which) {
        case GS_BUF_SORTED_TILE:
            return read_tile_words(c, c->sort.hi[si], sp.num_elems, dst, bytes);
        case GS_BUF_SORTED_DEPTH:
            if (c->depth_dropped && c->have_frame && !c->unsorted_valid) {
                // the frame path stops moving the depth words once they are sorted: rebuild them from the ids
                if (bytes > e_bytes) return fail(c, GS_ERR_INVALID, "gs_debug_read: size exceeds buffer");
                std::vector<uint32_t> ids(sp.num_elems), depth(c->n);
                if (sp.num_elems) HIP_TRY(c, hipMemcpy(ids.data(), c->sort.id[si], e_bytes, hipMemcpyDeviceToHost));
                HIP_TRY(c, hipMemcpy(depth.data(), c->scratch.depth_key, (size_t)c->n * sizeof(uint32_t), hipMemcpyDeviceToHost));
                uint32_t* out = static_cast<uint32_t*>(dst);
                for (size_t i = 0; i < bytes / sizeof(uint32_t); ++i) out[i] = ids[i] < c->n ? depth[ids[i]] : 0u;
                return GS_OK;
            }
            src = c->sort.lo[si]; avail = e_bytes; break;
        case GS_BUF_SORTED_ID: src = c->sort.id[si]; avail = e_bytes; break;
        case GS_BUF_RANGES: src = c->ranges; avail = (size_t)c->grid_w * c->grid_h * 8; break;
        case GS_BUF_COUNT: {
            if (bytes > sizeof(uint64_t)) return fail(c, GS_ERR_INVALID, "gs_debug_read: size");
            std::memcpy(dst, &sp.counter, bytes);
            return GS_OK;
        }
        case GS_BUF_IMAGE: src = c->framebuffer; avail = (size_t)c->width * c->height * 4; break;
        case GS_BUF_UNSORTED_TILE:
        case GS_BUF_UNSORTED_DEPTH:
        case GS_BUF_UNSORTED_ID:
            // the list as emitted lives in ping-pong half 0 and is overwritten by the second pass
            if (!c->unsorted_valid)
                return fail(c, GS_ERR_INVALID, "gs_debug_read: unsorted list only valid after gs_debug_init_sort_list");
            if (which == GS_BUF_UNSORTED_TILE) return read_tile_words(c, c->sort.hi[0], sp.num_elems, dst, bytes);
            src = which == GS_BUF_UNSORTED_DEPTH ? c->sort.lo[0] : c->sort.id[0];
            avail = e_bytes;
            break;
        case GS_BUF_COLOR:
        case GS_BUF_COV: {
            const size_t need = (size_t)c->n * 4 * sizeof(float);
            if (bytes > need) return fail(c, GS_ERR_INVALID, "gs_debug_read: size exceeds buffer");
            std::vector<SplatRaster> host(c->n);
            HIP_TRY(c, hipMemcpy(host.data(), c->scratch.raster, (size_t)c->n * sizeof(SplatRaster), hipMemcpyDeviceToHost));
            // color.a as the reference stores it (InitSortList.comp:126) is the opacity itself; the record's copy is
            // already zeroed where the 2x2 determinant vanishes (RenderGaussians.comp:104), so it comes from the scene
            std::vector<float> opacity;
            std::vector<uint32_t> touched;
            // N6 (InitSortList.comp:124-127): the reference stores colour for EVERY splat that passes the culls; the frame
            // evaluates it for the emitting ones only, so the others are evaluated here, on demand, from the last frame's
            // camera (k_debug_colour) -- in a context that owns the whole grid.  A context that owns a subset of the tile rows
            // does not even project the splats that cannot reach its rows: there GS_BUF_COLOR stays what the frame stored.
            std::vector<float> on_demand;
            const bool whole_grid = c->row_begin == 0u && c->row_end == c->grid_h && c->row_stride == 1u;
            if (which == GS_BUF_COLOR) {
                opacity.resize(c->n); touched.resize(c->n);
                HIP_TRY(c, hipMemcpy(opacity.data(), c->scene.opacity, (size_t)c->n * sizeof(float), hipMemcpyDeviceToHost));
                HIP_TRY(c, hipMemcpy(touched.data(), c->scratch.tiles_touched, (size_t)c->n * sizeof(uint32_t), hipMemcpyDeviceToHost));
                if (whole_grid) {
                    float* dev = nullptr;
                    HIP_TRY(c, hipMalloc((void**)&dev, need));
                    launch_debug_colour(c->last_fp, c->scene, c->scratch, dev, c->stream);
                    hipError_t e = hipGetLastError();
                    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
                    on_demand.resize((size_t)c->n * 4);
                    if (e == hipSuccess) e = hipMemcpy(on_demand.data(), dev, need, hipMemcpyDeviceToHost);
                    (void)hipFree(dev);
                    HIP_TRY(c, e);
                }
            }
            // records of a wave (64 consecutive splats) that k_project did not store this frame -- wholly culled, or with
            // nothing to emit into this context's tile rows -- read back as zero, what a culled splat's scratch holds
            std::vector<uint8_t> wrote((size_t)c->num_blocks * 4);
            HIP_TRY(c, hipMemcpy(wrote.data(), c->scratch.wave_wrote, wrote.size(), hipMemcpyDeviceToHost));
            std::vector<float> outv((size_t)c->n * 4, 0.0f);
            for (uint32_t i = 0; i < c->n; ++i) {
                if (!wrote[i / 64u]) continue;
                const SplatRaster& r = host[i];
                float* o = &outv[(size_t)i * 4];
                if (which == GS_BUF_COLOR) {
                    if (touched[i]) { o[0] = r.r; o[1] = r.g; o[2] = r.b; o[3] = opacity[i]; }       // what the frame stored and blended
                    else if (!on_demand.empty() && on_demand[(size_t)i * 4 + 3] != 0.0f) {           // passed the culls, touched no tile
                        o[0] = on_demand[(size_t)i * 4]; o[1] = on_demand[(size_t)i * 4 + 1]; o[2] = on_demand[(size_t)i * 4 + 2]; o[3] = opacity[i];
                    }
                }
                else { o[0] = r.cx; o[1] = r.cy; o[2] = r.cz; o[3] = 0.0f; }
            }
            std::memcpy(dst, outv.data(), bytes);
            return GS_OK;
        }
        default: return fail(c, GS_ERR_INVALID, "gs_debug_read: unknown buffer id");
    }
    if (bytes > avail) return fail(c, GS_ERR_INVALID, "gs_debug_read: size exceeds buffer");
    if (bytes) HIP_TRY(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return GS_OK;
}

// Camera.cpp:7-48 over the glm 0.9.9.8 formulas (lookAtRH, perspectiveRH_ZO, normalize, cross).
int gs_camera_matrices(const float pos[3], float yaw, float pitch, float aspect, float near_plane,
                       float far_plane, float view[16], float proj[16]) {
    if (!pos || !view || !proj) return GS_ERR_INVALID;
    auto normalize3 = [](float v[3]) {
        const float d = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
        const float inv = 1.0f / std::sqrt(d);
        v[0] *= inv; v[1] *= inv; v[2] *= inv;
    };
    auto cross3 = [](const float a[3], const float b[3], float o[3]) {
        o[0] = a[1] * b[2] - b[1] * a[2];
        o[1] = a[2] * b[0] - b[2] * a[0];
        o[2] = a[0] * b[1] - b[0] * a[1];
    };
    auto dot3 = [](const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    float fwd[3] = {(float)(std::sin((double)yaw) * std::cos((double)pitch)), (float)std::sin((double)pitch),
                    (float)(std::cos((double)yaw) * std::cos((double)pitch))};   // Camera.cpp:10-16
    normalize3(fwd);
    const float up[3] = {0.0f, 1.0f, 0.0f};
    const float center[3] = {pos[0] + fwd[0], pos[1] + fwd[1], pos[2] + fwd[2]}; // Camera.cpp:34-38
    float f[3] = {center[0] - pos[0], center[1] - pos[1], center[2] - pos[2]};
    normalize3(f);
    float s[3], u[3];
    cross3(f, up, s);
    normalize3(s);
    cross3(s, f, u);
    std::memset(view, 0, 16 * sizeof(float));
    view[0] = s[0]; view[4] = s[1]; view[8] = s[2];
    view[1] = u[0]; view[5] = u[1]; view[9] = u[2];
    view[2] = -f[0]; view[6] = -f[1]; view[10] = -f[2];
    view[12] = -dot3(s, pos); view[13] = -dot3(u, pos); view[14] = dot3(f, pos);
    view[15] = 1.0f;
    const float fovy = 90.0f * 0.01745329251994329576923690768489f;                // Camera.cpp:42
    const float tan_half = std::tan(fovy / 2.0f);
    std::memset(proj, 0, 16 * sizeof(float));
    proj[0] = 1.0f / (aspect * tan_half);
    proj[5] = 1.0f / tan_half;
    proj[10] = far_plane / (near_plane - far_plane);
    proj[11] = -1.0f;
    proj[14] = -(far_plane * near_plane) / (far_plane - near_plane);
    return GS_OK;
}

int gs_sort_host(gs_ctx* c, uint32_t* tile, uint32_t* depth, uint32_t* id, uint32_t n,
                 uint32_t num_sort_bits) {
    if (!c || !tile || !depth || !id) return GS_ERR_INVALID;
    if (num_sort_bits == 0 || num_sort_bits > 64 || (num_sort_bits % kRadixBits) != 0)
        return fail(c, GS_ERR_INVALID, "gs_sort_host: num_sort_bits must be a multiple of 4 in [4,64]");
    if (n == 0) return GS_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    SortBuffers sb{};
    DeviceOwner mem;
    int rc = alloc_sort(c, mem, sb, n);
    if (rc != GS_OK) { mem.release(); return rc; }
    const size_t bytes = (size_t)n * sizeof(uint32_t);
    hipError_t e = hipMemcpyAsync(sb.hi[0], tile, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(sb.lo[0], depth, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(sb.id[0], id, bytes, hipMemcpyHostToDevice, c->stream);
    int si = 0;
    if (e == hipSuccess) {
        launch_set_sort_params(sb.params, sb.coarse, n, c->stream);
        si = launch_radix_sort(sb, whole_list_run(c, n, num_sort_bits), c->stream);
        e = si < 0 ? hipErrorInvalidValue : hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(tile, sb.hi[si], bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(depth, sb.lo[si], bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(id, sb.id[si], bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    mem.release();
    if (e != hipSuccess) return fail(c, GS_ERR_HIP, std::string("gs_sort_host: ") + hipGetErrorString(e));
    return GS_OK;
}

int gs_sort_bench(gs_ctx* c, uint32_t n, uint32_t num_tiles, uint32_t iters, uint64_t seed,
                  float* ms_per_sort, uint32_t* sorted_ok) {
    if (!c || !ms_per_sort || n == 0 || num_tiles == 0 || iters == 0) return GS_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    SortBuffers sb{};
    DeviceOwner mem;
    int rc = alloc_sort(c, mem, sb, n);
    if (rc != GS_OK) { mem.release(); return rc; }
    const SortRun run = whole_list_run(c, n, num_sort_bits_for(num_tiles));
    uint32_t* bad = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = mem.alloc(bad, sizeof(uint32_t));
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    float total_ms = 0.0f;
    int si = 0;
    for (uint32_t it = 0; it < iters + 1 && e == hipSuccess; ++it) {   // iteration 0 = warm-up
        launch_fill_random_keys(sb.lo[0], sb.hi[0], sb.id[0], n, num_tiles, seed + it, c->stream);
        launch_set_sort_params(sb.params, sb.coarse, n, c->stream);
        e = hipEventRecord(e0, c->stream);
        if (e != hipSuccess) break;
        si = launch_radix_sort(sb, run, c->stream);
        if (si < 0) { si = 0; e = hipErrorInvalidValue; break; }
        e = hipEventRecord(e1, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        float ms = 0.0f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (it > 0) total_ms += ms;
    }
    uint32_t bad_host = 0;
    if (e == hipSuccess) e = hipMemsetAsync(bad, 0, sizeof(uint32_t), c->stream);
    if (e == hipSuccess) {
        launch_check_sorted(sb.lo[si], sb.hi[si], n, bad, c->stream);
        e = hipMemcpyAsync(&bad_host, bad, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    mem.release();
    if (e != hipSuccess) return fail(c, GS_ERR_HIP, std::string("gs_sort_bench: ") + hipGetErrorString(e));
    *ms_per_sort = total_ms / (float)iters;
    if (sorted_ok) *sorted_ok = bad_host == 0 ? 1u : 0u;
    return GS_OK;
}

int gs_membench(gs_ctx* c, int kind, size_t bytes, uint32_t blocks, uint32_t iters, float* gbps, float* ms_out) {
    if (!c || !gbps || bytes < 16 || iters == 0 || kind < 0 || kind > 12) return GS_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    bytes &= ~(size_t)15;
    if (blocks == 0) blocks = 2048;
    char *src = nullptr, *dst = nullptr;
    DeviceOwner mem;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = mem.alloc(src, bytes + 65536);     // slack: the skewed scatter probes write a little past `bytes`
    if (e == hipSuccess) e = mem.alloc(dst, bytes + 65536);
    if (e == hipSuccess) e = hipMemsetAsync(src, 0x5A, bytes, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(dst, 0, bytes, c->stream);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    float ms = 0.0f;
    if (e == hipSuccess) {
        for (int w = 0; w < 3; ++w) launch_stream_probe(kind, src, dst, bytes, blocks, c->stream);
        e = hipEventRecord(e0, c->stream);
        for (uint32_t i = 0; i < iters; ++i) launch_stream_probe(kind, src, dst, bytes, blocks, c->stream);
        if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    mem.release();
    if (e != hipSuccess) return fail(c, GS_ERR_HIP, std::string("gs_membench: ") + hipGetErrorString(e));
    const double moved = (double)bytes * ((kind & 1) || kind >= 4 ? 2.0 : 1.0) * iters;
    *gbps = (float)(moved / (ms * 1e-3) / 1e9);
    if (ms_out) *ms_out = ms / (float)iters;
    return GS_OK;
}

} // extern "C"
