// gs_api.cpp -- host side of libgsplat_hip.so: the C-ABI of include/gsplat.h over the HIP kernels, the part that has a
// counterpart in the reference: context, scene, resolution, outputs, tile rows and the frame.  (gs_train.cpp: the training
// calls; gs_debug.cpp: read-backs and micro-benchmarks.)
// Mirrors the reference's frame orchestration (Engine/Graphics/Renderer.cpp, Subrenderer.cpp,
// Sort/RadixSort.cpp) with HIP streams/events in place of Vulkan command buffers/timestamps.
// There is NO CPU fallback: without a GPU every entry point that computes fails with
// GS_ERR_NO_DEVICE / GS_ERR_HIP.
#include "gs_ctx.h"

#include <cstddef>
#include <iterator>
#include <new>

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
    drop_sort_graph(c);
    c->res_mem.release();
    c->sort = SortBuffers{};          // fed[1], fed[2] point into the allocation of fed[0]
    c->outputs_valid = false;
    // the strips of a sharded frame are sized by the resolution: gs_dist_shard_rows must be called again
    gsi_dist_free_buffers(c);
    c->capacity = 0; c->width = c->height = 0;
    resolution_freed(c);
    if (c->elems_note) *(volatile uint32_t*)c->elems_note = 0u;     // (free_resolution's callers have waited for the stream)
}

// Renderer.cpp:703-710
uint32_t ceil_pow2(uint32_t x) { uint32_t v = 1; while (v < x) v *= 2; return v; }

inline bool sorts_splat_first(uint32_t algo) { return algo == GS_SORT_RADIX4_SPLAT_FIRST || algo == GS_SORT_RADIX8_SPLAT_FIRST; }
inline uint32_t digit_bits_of(uint32_t algo) { return algo == GS_SORT_RADIX8 || algo == GS_SORT_RADIX8_SPLAT_FIRST ? 8u : (uint32_t)kRadixBits; }

} // namespace

// ---- what gs_train.cpp and gs_debug.cpp share with this file (declared in gs_ctx.h)

uint32_t num_sort_bits_for(uint32_t num_tiles) {
    uint32_t x = num_tiles - 1u, bits = 0;
    for (int i = 31; i >= 0; --i) if ((x >> i) & 1u) { bits = (uint32_t)i + 1u; break; }
    return ((32u + bits + kRadixBits - 1u) / kRadixBits) * kRadixBits;
}

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
    HIP_TRY(ctx, mem.alloc(s.params, 2 * sizeof(SortParams)));
    HIP_TRY(ctx, hipMemset(s.params, 0, 2 * sizeof(SortParams)));
    HIP_TRY(ctx, mem.alloc(s.coarse, (size_t)kMaxSortPasses * kBins * kCoarse * sizeof(uint32_t)));
    return GS_OK;
}

// They know their element count: fed counts (gs_sort.hip) for short lists of the 4-bit sorter.
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

namespace {

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
        case kStageEmit: launch_emit(f.fp, c->scratch, c->sort, !sorts_splat_first(c->cfg.sort_algorithm) && c->sort_pass0, st); break;
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
    list_launching(c);
    if (!c->n) return fail(c, GS_ERR_NO_SCENE, "gs_render: no gaussians uploaded");
    if (!c->capacity) return fail(c, GS_ERR_NO_SCENE, "gs_render: gs_set_resolution not called");
    if (!view || !proj || !cam_pos) return fail(c, GS_ERR_INVALID, "gs_render: null camera argument");
    if (!sh_mode_known(sh_mode)) return fail(c, GS_ERR_INVALID, "gs_render: " GS_SH_MODE_REFUSAL);
    Frame f{c, make_frame_params(c, view, proj, cam_pos, sh_mode)};
    FrameParams& fp = f.fp;
    if (!out_dev) fp.compact_out = 0u;   // the internal framebuffer is always a whole frame in real rows
    const bool tm = c->cfg.record_timings != 0;
    hipStream_t st = c->stream;

    c->num_marks = 0;
    if (tm) if (int r = mark(c, kBucketNone)) return r;
    // computeInitSortList (Subrenderer.cpp:37-170): per-frame resets, then the dispatch.  Only the
    // ranges need clearing here: the 0xFF sentinel fill of both lists (Subrenderer.cpp:42-46,
    // RadixSort.cpp:676-692) is unobservable once every later stage runs over E instead of C.
    // (the ranges and the sort's coarse totals are cleared inside k_scan_blocks: no fill launches in a frame)
    fp.parity = (c->emit_parity ^= 1u);
    const FrameParams listed = fp;      // what gs_backward* and the read-backs take the frame by
    const bool splat_first = sorts_splat_first(c->cfg.sort_algorithm);
    fp.splat_first = splat_first ? 1u : 0u;
    const bool bucket = c->cfg.sort_algorithm == GS_SORT_TILE_BUCKET;
    const float tile_share = c->grid_h ? (float)c->rows_owned / (float)c->grid_h : 1.0f;
    f.ordered = c->cfg.tile_order == GS_TILE_ORDER_LONGEST_FIRST;
    f.direct = c->cfg.record_timings >= 2;
    hipEvent_t* const pass_events = f.direct ? c->scatter_ev : nullptr;
    // k_project -- the one kernel of a frame that reads FrameParams::antialias -- goes to the stream here, on every frame and
    // outside every capture (the graphs below start behind the scan): gs_set_antialias has no graph to drop
    launch_project(fp, c->scene, c->scratch, st);
    launch_scan_blocks(fp, c->scratch, c->sort.params, c->ranges, c->sort.coarse, st);
    f.fixed = fp;
    f.fixed.antialias = 0u;             // nothing behind the scan reads it: the captured arguments do not depend on the flag
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
        // the packed payload of the depth passes (gs_sort_words.h): the contractual sorter over 16-bit tile ids and 24-bit
        // splat indices; sort_pass() checks what the run itself must offer.  Like the fed counts it is part of the capture.
        const bool packed = c->cfg.sort_algorithm == GS_SORT_RADIX4 && frame_packs_payload(c->hi16, c->n, c->cfg.record_timings);
        // pass 0 inside InitSortList (k_emit<false, true>): the contractual sorter with a Count launch per pass, over every
        // tile row, without per-pass timers -- a frame with them is what the per-pass profiles and tests/test_parity_gpu.py
        // are stated in (eight depth launches).  Part of the capture as well.
        const bool pass0 = GS_EMIT_PASS0 != 0 && c->cfg.sort_algorithm == GS_SORT_RADIX4 && !fed && c->cfg.record_timings < 2u &&
                           c->row_begin == 0u && c->row_end == c->grid_h && c->row_stride == 1u;
        if (fed != c->sort_fed || packed != c->sort_packed || pass0 != c->sort_pass0) {
            if (c->run_graph[0].exec || c->chain_graph.exec) HIP_TRY(c, hipStreamSynchronize(st));   // the graph may still be executing (rare: the mode flips)
            drop_sort_graph(c);
            c->sort_fed = fed;
            c->sort_packed = packed;
            c->sort_pass0 = pass0;
        }
        fp.packed = packed ? 1u : 0u;
        // the bucket sorter runs the tile-word passes alone and carries the depth words through them
        // (pass0: the list arrives in half 1, in pass 0's order; that pass's launches stay in the chain for a frame that
        // overflows, over the record k_scan_blocks leaves in sort.params[1])
        c->runs[0] = {.capacity = c->capacity, .first_bit = bucket ? 32u : 0u, .num_sort_bits = c->band_sort_bits,
                      .start = pass0 ? 1 : 0, .passes_done = pass0 ? 1u : 0u, .done_params = pass0 ? c->sort.params + 1 : nullptr,
                      .drop_depth_payload = !bucket, .hi16 = c->hi16, .packed = packed, .share = tile_share, .fed = fed,
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
    // computeRenderGaussians (Subrenderer.cpp:218-346), with the outputs of gs_set_outputs beside the image
    const RenderOutputs outs{reinterpret_cast<float4*>(c->out_rgba32f), c->out_depth, c->scratch.view_z};
    launch_render(fp, c->scratch.raster, c->sort.id[f.sorted], c->ranges, f.ordered ? c->tile_order : nullptr,
                  out_dev ? out_dev : c->framebuffer, c->cfg.render_mode, c->cfg.render_kernel, st, outs);
    if (int r = check_launch(c, "RenderGaussians")) return r;
    if (tm) if (int r = mark(c, kBucketRender)) return r;
    frame_enqueued(c, listed, f.sorted);
    c->last_pass0 = !splat_first && c->sort_pass0;
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
                sum_bytes[which] += (float)sort_pass_bytes(p, run.hi16);   // depth + tile + id (or the packed payload), r + w
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

int output_buffer(gs_ctx* c, uint32_t which, const char* who, void** dev, size_t* size) {
    if (which != GS_OUTPUT_RGBA32F && which != GS_OUTPUT_DEPTH)
        return fail(c, GS_ERR_INVALID, std::string(who) + ": which must be GS_OUTPUT_RGBA32F or GS_OUTPUT_DEPTH");
    if (!(c->outputs & which)) return fail(c, GS_ERR_INVALID, std::string(who) + ": that output is not enabled (gs_set_outputs)");
    if (!c->capacity) return fail(c, GS_ERR_INVALID, std::string(who) + ": gs_set_resolution not called");
    const size_t px = (size_t)c->width * c->height;
    *dev = which == GS_OUTPUT_RGBA32F ? (void*)c->out_rgba32f : (void*)c->out_depth;
    *size = px * (which == GS_OUTPUT_RGBA32F ? 4 * sizeof(float) : sizeof(float));
    return GS_OK;
}

extern "C" {

uint32_t gs_api_version(void) { return GS_API_VERSION; }

// the frame mode of an active SH degree (host arithmetic: no context, no GPU)
int gs_sh_mode_of_degree(uint32_t degree, uint32_t* sh_mode_out) {
    static const uint32_t mode[4] = {GS_SH_ONLY_FIRST_BAND, GS_SH_DEGREE_1, GS_SH_DEGREE_2, GS_SH_ALL_BANDS};
    if (degree > 3u || !sh_mode_out) return GS_ERR_INVALID;
    *sh_mode_out = mode[degree];
    return GS_OK;
}

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
    // the five camera constants: every kernel that reads FrameParams divides by far - near, by tan(fov_y / 2) or by a
    // limit derived from them, so a value that cannot be a camera's is refused here rather than rendered
    const struct { const char* name; float value; } constants[5] = {
        {"near_plane", cfg.near_plane}, {"far_plane", cfg.far_plane}, {"ndc_cull", cfg.ndc_cull},
        {"in_view_limit", cfg.in_view_limit}, {"fov_y", cfg.fov_y}};
    for (const auto& k : constants)
        if (!std::isfinite(k.value)) return fail(nullptr, GS_ERR_INVALID, std::string("gs_create: ") + k.name + " is not finite");
    if (cfg.near_plane <= 0.0f) return fail(nullptr, GS_ERR_INVALID, "gs_create: near_plane must be positive");
    if (cfg.far_plane <= cfg.near_plane) return fail(nullptr, GS_ERR_INVALID, "gs_create: far_plane must be beyond near_plane");
    if (cfg.ndc_cull <= 0.0f) return fail(nullptr, GS_ERR_INVALID, "gs_create: ndc_cull must be positive");
    if (cfg.in_view_limit <= 0.0f) return fail(nullptr, GS_ERR_INVALID, "gs_create: in_view_limit must be positive");
    // tan(fov_y / 2) must be finite and positive: the half angle inside (0, pi / 2)
    if (cfg.fov_y <= 0.0f || (double)cfg.fov_y >= 3.14159265358979323846)
        return fail(nullptr, GS_ERR_INVALID, "gs_create: fov_y must lie in (0, pi)");
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
    c->mcmc_mem.release();
    c->init_mem.release();
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
    const size_t padded = (size_t)c->num_blocks + kBlockSumsPad;
    // behind block_sums: pass 0 inside InitSortList -- the rows of the blocks (whole chunks) and the two halves of the chunk
    // sums, which start from zero
    const size_t chunks = pass0_chunks(c->num_blocks);
    HIP_TRY(c, mem.alloc_zeroed(sc.block_sums, (padded + 4 + (chunks * kPass0Chunk + 2 * chunks) * kBins) * sizeof(uint32_t), st));
    sc.pass0_hist = pass0_hist_of(sc.block_sums, c->num_blocks);
    sc.pass0_chunk = pass0_chunk_of(sc.block_sums, c->num_blocks);
    HIP_TRY(c, mem.alloc_zeroed(sc.block_offsets, padded * sizeof(uint32_t), st));
    HIP_TRY(c, mem.alloc_zeroed(sc.wave_wrote, (size_t)c->num_blocks * 4, st));
    HIP_TRY(c, mem.alloc_zeroed(sc.help_list, (size_t)kEmitHelpCap * sizeof(uint2), st));
    HIP_TRY(c, mem.alloc_zeroed(sc.help_count, 4 * sizeof(uint32_t), st));
    // the scanned rows of pass 0 (whole chunks: the totals row lies behind the last block)
    HIP_TRY(c, mem.alloc_zeroed(sc.pass0_offs, chunks * kPass0Chunk * kBins * sizeof(uint32_t), st));
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
    if (e != hipSuccess) { free_scene(c); return fail(c, GS_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e)); }
    c->scene = b;
    if (int r = alloc_scratch(c, n)) { free_scene(c); return r; }
    return GS_OK;
}

// Behind the planes of a fresh scene (e: what writing them returned): the boxes of the blocks and a wait; then the scene is
// the context's, or gone
static int finish_new_scene(gs_ctx* c, uint32_t n, const char* who, hipError_t e) {
    if (e == hipSuccess) launch_block_bounds(n, c->scene, c->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { free_scene(c); return fail(c, GS_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e)); }
    c->n = n;
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
    hipError_t e = hipSuccess;
    for (uint32_t first = 0; first < n && e == hipSuccess; first += chunk) {
        const uint32_t cnt = (n - first) < chunk ? (n - first) : chunk;
        e = hipMemcpyAsync(staging, src + (size_t)first * GS_GAUSSIAN_RECORD_BYTES,
                           (size_t)cnt * GS_GAUSSIAN_RECORD_BYTES, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) {
            launch_aos_to_soa(staging, first, cnt, n, c->scene, c->stream);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // staging is reused
    }
    (void)hipFree(staging);
    return finish_new_scene(c, n, "gs_upload_gaussians", e);
}

int gs_upload_gaussians_device(gs_ctx* c, const void* aos336_dev, uint32_t n) {
    if (!c) return GS_ERR_INVALID;
    if (!aos336_dev || n == 0) return fail(c, GS_ERR_INVALID, "gs_upload_gaussians_device: empty input");
    HIP_TRY(c, hipSetDevice(c->device));
    const float* src = static_cast<const float*>(aos336_dev);
    // the same scene size: the planes are rewritten in place behind whatever is enqueued on the stream, and every
    // context that shares them renders the new values; resolution, scratch and captured graphs stay
    const bool in_place = c->shared && c->n == n;
    if (!in_place) if (int r = new_scene(c, n, "gs_upload_gaussians_device")) return r;
    launch_aos_to_soa(src, 0, n, n, c->scene, c->stream);
    if (!in_place) return finish_new_scene(c, n, "gs_upload_gaussians_device", hipGetLastError());
    launch_block_bounds(n, c->scene, c->stream);
    scene_or_rows_changed(c);
    HIP_TRY(c, hipGetLastError());
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
    scene_or_rows_changed(c);
    return check_launch(c, "gs_upload_rows_device");
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
    // hipMemset returns before a device fill is done, and the null stream it ran on is not ordered with the context's
    // non-blocking stream: wait for the fills, or a short first frame can store its outputs before the zeros land
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        free_resolution(c);
        return fail(c, GS_ERR_HIP, std::string("gs_set_resolution: ") + hipGetErrorString(e));
    }
    return GS_OK;
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
    // hipMemset returns before a device fill is done, and the null stream it ran on is not ordered with the context's
    // non-blocking stream: wait for the fills, or a short first frame can store its outputs before the zeros land
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {   // back to RGBA8-only frames rather than half set up
        free_outputs(c);
        c->outputs = 0;
        return fail(c, GS_ERR_HIP, std::string("gs_set_outputs: ") + hipGetErrorString(e));
    }
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

static int apply_tile_rows(gs_ctx* c, uint32_t row_begin, uint32_t row_end, uint32_t stride, uint32_t phase,
                           bool compact_out) {
    // everything that can fail first: a context that reports an error keeps its old rows, with the sort bits and graphs of those
    const bool graphs = c->run_graph[0].exec || c->run_graph[1].exec || c->chain_graph.exec;
    if (c->elems_note || graphs) HIP_TRY(c, hipStreamSynchronize(c->stream));   // no frame in flight may still write the note or execute a graph
    // another band: another list length (GS_COUNT_AUTO learns it from the next frame)
    if (c->elems_note) *(volatile uint32_t*)c->elems_note = 0u;
    if (graphs) drop_sort_graph(c);
    c->row_begin = row_begin; c->row_end = row_end; c->row_stride = stride;
    c->first_row = row_begin + phase;
    c->rows_owned = c->first_row < row_end ? (row_end - c->first_row + stride - 1u) / stride : 0u;
    c->compact_out = compact_out;
    scene_or_rows_changed(c);
    const uint32_t owned_tiles = c->rows_owned * c->grid_w;
    c->band_sort_bits = num_sort_bits_for(owned_tiles ? owned_tiles : 1u);
    c->hi16 = owned_tiles <= 65535u;
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

} // extern "C"
