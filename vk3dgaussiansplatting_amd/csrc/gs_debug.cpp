// gs_debug.cpp -- the stage-level read-backs (gs_debug_init_sort_list, gs_debug_read) and the micro-benchmarks of the
// stand-alone sorter and the memory system (gs_sort_host, gs_sort_bench, gs_membench).  Nothing here is on a frame's path.
#include "gs_ctx.h"

using namespace gs;

extern "C" {

int gs_debug_init_sort_list(gs_ctx* c, const float view[16], const float proj[16],
                            const float cam_pos[3], uint32_t sh_mode) {
    if (!c) return GS_ERR_INVALID;
    const bool outputs_valid = c->outputs_valid;
    list_launching(c);
    if (!c->n || !c->capacity) return fail(c, GS_ERR_NO_SCENE, "gs_debug_init_sort_list: scene/resolution not set");
    if (!view || !proj || !cam_pos) return fail(c, GS_ERR_INVALID, "gs_debug_init_sort_list: null camera argument");
    if (!sh_mode_known(sh_mode)) return fail(c, GS_ERR_INVALID, "gs_debug_init_sort_list: " GS_SH_MODE_REFUSAL);
    HIP_TRY(c, hipSetDevice(c->device));
    FrameParams fp = make_frame_params(c, view, proj, cam_pos, sh_mode);
    fp.parity = (c->emit_parity ^= 1u);
    launch_project(fp, c->scene, c->scratch, c->stream);
    launch_scan_blocks(fp, c->scratch, c->sort.params, c->ranges, c->sort.coarse, c->stream);
    launch_emit(fp, c->scratch, c->sort, false, c->stream);      // the canonical unsorted list, whatever frames do
    if (int r = check_launch(c, "InitSortList")) return r;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    unsorted_list_ready(c, fp, outputs_valid);
    SortParams sp{};
    HIP_TRY(c, hipMemcpy(&sp, c->sort.params, sizeof(sp), hipMemcpyDeviceToHost));
    return sp.overflow ? GS_WARN_OVERFLOW : GS_OK;
}

// The sort list holds compact tile ids (uint16 or uint32, FrameParams) -> the uint32 GLOBAL tile ids callers expect
// (after a tile-row change without a new list, hi16 and the rows may be the new band's, not the list's)
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
    if (c->last.kind == LastFrame::kNone && which != GS_BUF_IMAGE) return fail(c, GS_ERR_NO_SCENE, "gs_debug_read: no frame rendered yet");
    SortParams sp{};
    HIP_TRY(c, hipMemcpy(&sp, c->sort.params, sizeof(sp), hipMemcpyDeviceToHost));
    const size_t e_bytes = (size_t)sp.num_elems * sizeof(uint32_t);
    const void* src = nullptr;
    size_t avail = 0;
    const int si = c->last.sorted_index;
    switch (which) {
        case GS_BUF_SORTED_TILE:
            return read_tile_words(c, c->sort.hi[si], sp.num_elems, dst, bytes);
        case GS_BUF_SORTED_DEPTH:
            if (c->last.kind == LastFrame::kFrame && c->cfg.sort_algorithm != GS_SORT_TILE_BUCKET) {
                // the frame path (but for the bucket sorter, see k_scatter) stops moving the depth words once they are
                // sorted: rebuild them from the ids
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
            if (c->last.kind != LastFrame::kUnsortedList)
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
            std::vector<uint32_t> touched(c->n);
            HIP_TRY(c, hipMemcpy(touched.data(), c->scratch.tiles_touched, (size_t)c->n * sizeof(uint32_t), hipMemcpyDeviceToHost));
            if (which == GS_BUF_COLOR) {
                opacity.resize(c->n);
                HIP_TRY(c, hipMemcpy(opacity.data(), c->scene.opacity, (size_t)c->n * sizeof(float), hipMemcpyDeviceToHost));
            }
            // N6 (InitSortList.comp:124-127): the reference stores colour and covariance for EVERY splat that passes the culls;
            // the frame stores the records of the chunks with an emitting splat and evaluates the colour of the emitting ones
            // only, so what the others would hold is computed here, on demand, from the last frame's camera (k_debug_records,
            // k_debug_colour) -- in a context that owns the whole grid.  A context that owns a subset of the tile rows does not
            // even project the splats that cannot reach its rows: there both stay what the frame stored.
            std::vector<float> records, on_demand;      // [n][8] (sx, sy, 0, passed | 0, cx, cy, cz), [n][4]: non-emitting splats
            const bool whole_grid = c->row_begin == 0u && c->row_end == c->grid_h && c->row_stride == 1u;
            if (whole_grid) {
                float* dev = nullptr;                    // the records, then the colours
                HIP_TRY(c, hipMalloc((void**)&dev, 3 * need));
                launch_debug_records(c->last.fp, c->scene, c->scratch, dev, c->stream);
                if (which == GS_BUF_COLOR) launch_debug_colour(c->last.fp, c->scene, dev, dev + (size_t)c->n * 8, c->stream);
                hipError_t e = hipGetLastError();
                if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
                records.resize((size_t)c->n * 8);
                if (e == hipSuccess) e = hipMemcpy(records.data(), dev, 2 * need, hipMemcpyDeviceToHost);
                if (which == GS_BUF_COLOR) {
                    on_demand.resize((size_t)c->n * 4);
                    if (e == hipSuccess) e = hipMemcpy(on_demand.data(), dev + (size_t)c->n * 8, need, hipMemcpyDeviceToHost);
                }
                (void)hipFree(dev);
                HIP_TRY(c, e);
            }
            // wave_wrote: the quarter waves (16 consecutive splats) whose records k_project stored this frame.  The whole grid:
            // the record of an emitting splat is this frame's (its chunk was stored), every other splat is recomputed above.  A
            // band: records of a wave that emits nothing into this context's tile rows read back as zero, what a culled
            // splat's scratch holds
            std::vector<uint8_t> wrote((size_t)c->num_blocks * 4);
            HIP_TRY(c, hipMemcpy(wrote.data(), c->scratch.wave_wrote, wrote.size(), hipMemcpyDeviceToHost));
            std::vector<float> outv((size_t)c->n * 4, 0.0f);
            for (uint32_t i = 0; i < c->n; ++i) {
                const bool stored = (wrote[i / 64u] >> ((i / 16u) & 3u)) & 1u;
                const SplatRaster& r = host[i];
                float* o = &outv[(size_t)i * 4];
                if (stored && (touched[i] || !whole_grid)) {
                    if (which == GS_BUF_COV) { o[0] = r.cx; o[1] = r.cy; o[2] = r.cz; o[3] = 0.0f; }
                    else if (touched[i]) { o[0] = r.r; o[1] = r.g; o[2] = r.b; o[3] = opacity[i]; }  // what the frame stored and blended
                } else if (whole_grid && !touched[i] && records[(size_t)i * 8 + 3] != 0.0f) {        // passed the culls, touched no tile
                    const float* rec = &records[(size_t)i * 8];
                    if (which == GS_BUF_COV) { o[0] = rec[5]; o[1] = rec[6]; o[2] = rec[7]; o[3] = 0.0f; }
                    else { o[0] = on_demand[(size_t)i * 4]; o[1] = on_demand[(size_t)i * 4 + 1]; o[2] = on_demand[(size_t)i * 4 + 2]; o[3] = opacity[i]; }
                }
            }
            std::memcpy(dst, outv.data(), bytes);
            return GS_OK;
        }
        case GS_BUF_RASTER_OPACITY: {
            // SplatRaster::a of the splats that emitted an element in the last list: their quarter wave stored its records
            // (wave_wrote; a block k_band_cull rejected has zeros there and stale counts) and their count is not zero
            const size_t need = (size_t)c->n * sizeof(float);
            if (bytes > need) return fail(c, GS_ERR_INVALID, "gs_debug_read: size exceeds buffer");
            std::vector<SplatRaster> host(c->n);
            std::vector<uint32_t> touched(c->n);
            std::vector<uint8_t> wrote((size_t)c->num_blocks * 4);
            HIP_TRY(c, hipMemcpy(host.data(), c->scratch.raster, (size_t)c->n * sizeof(SplatRaster), hipMemcpyDeviceToHost));
            HIP_TRY(c, hipMemcpy(touched.data(), c->scratch.tiles_touched, (size_t)c->n * sizeof(uint32_t), hipMemcpyDeviceToHost));
            HIP_TRY(c, hipMemcpy(wrote.data(), c->scratch.wave_wrote, wrote.size(), hipMemcpyDeviceToHost));
            std::vector<float> outv(c->n, 0.0f);
            for (uint32_t i = 0; i < c->n; ++i)
                if (((wrote[i / 64u] >> ((i / 16u) & 3u)) & 1u) && touched[i]) outv[i] = host[i].a;
            std::memcpy(dst, outv.data(), bytes);
            return GS_OK;
        }
        // The three read-backs of work a frame decided NOT to do (nothing of a frame reads them back: host code only)
        case GS_BUF_WAVE_WROTE:
            // one byte per wave of 64 splats as k_project / k_band_cull left it; the waves past the last splat are not part
            src = c->scratch.wave_wrote; avail = ((size_t)c->n + 63u) / 64u; break;
        case GS_BUF_BAND_BLOCKS: {
            // word 0 = the count, then the records ascending by block (k_band_cull appends them in atomic arrival order)
            const FrameParams& fp = c->last.fp;
            const bool listed = !(fp.row_begin == 0u && fp.row_end == fp.grid_h) && fp.row_stride == 1u;   // launch_project's
            std::vector<uint32_t> rec(1);
            if (listed) {
                uint32_t count = 0;
                HIP_TRY(c, hipMemcpy(&count, c->scratch.help_count + 2u + fp.parity, sizeof(count), hipMemcpyDeviceToHost));
                if (count > c->num_blocks) return fail(c, GS_ERR_INVALID, "gs_debug_read: band list count exceeds the project blocks");
                rec.resize(1u + (size_t)count);
                if (count) HIP_TRY(c, hipMemcpy(rec.data() + 1, c->scratch.band_list, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost));
                std::sort(rec.begin() + 1, rec.end(), [](uint32_t a, uint32_t b) { return (a & 0x0FFFFFFFu) < (b & 0x0FFFFFFFu); });
            } else {
                // every row, or interleaved rows: k_band_cull does not run and k_project takes every block, no wave skipped
                rec.resize(1u + (size_t)c->num_blocks);
                for (uint32_t b = 0; b < c->num_blocks; ++b) rec[1u + b] = b;
            }
            rec[0] = (uint32_t)(rec.size() - 1u);
            if (bytes > rec.size() * sizeof(uint32_t)) return fail(c, GS_ERR_INVALID, "gs_debug_read: size exceeds buffer");
            std::memcpy(dst, rec.data(), bytes);
            return GS_OK;
        }
        case GS_BUF_TILE_ORDER: {
            if (c->last.kind != LastFrame::kFrame)
                return fail(c, GS_ERR_INVALID, "gs_debug_read: the tile order is only valid after a frame");
            const FrameParams& fp = c->last.fp;
            const size_t tiles = (size_t)fp.rows_owned * fp.grid_w;
            if (bytes > tiles * sizeof(uint32_t)) return fail(c, GS_ERR_INVALID, "gs_debug_read: size exceeds buffer");
            const size_t cnt = bytes / sizeof(uint32_t);
            uint32_t* out = static_cast<uint32_t*>(dst);
            if (c->cfg.tile_order == GS_TILE_ORDER_LONGEST_FIRST) {
                if (cnt) HIP_TRY(c, hipMemcpy(out, c->tile_order, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost));
            } else {
                for (size_t i = 0; i < cnt; ++i) out[i] = (uint32_t)i;      // raster order: workgroup k takes compact tile k
            }
            for (size_t i = 0; i < cnt; ++i) {                              // compact -> global, as k_render's TileMap does
                const uint32_t k = out[i] / fp.grid_w, x = out[i] - k * fp.grid_w;
                out[i] = (fp.first_row + k * fp.row_stride) * fp.grid_w + x;
            }
            return GS_OK;
        }
        case GS_BUF_PASS0_OFFSETS: {
            // the scanned rows k_emit went by, then the sixteen digit bases, from the totals row behind them; only a frame
            // that took the path has them (a frame that overflowed wrote the plain list: its pass 0 ran as launches)
            if (c->last.kind != LastFrame::kFrame || !c->last_pass0 || sp.overflow)
                return fail(c, GS_ERR_INVALID, "gs_debug_read: the last frame did not run pass 0 inside InitSortList");
            std::vector<uint32_t> rows(((size_t)c->num_blocks + 1u) * kBins);
            if (bytes > rows.size() * sizeof(uint32_t)) return fail(c, GS_ERR_INVALID, "gs_debug_read: size exceeds buffer");
            HIP_TRY(c, hipMemcpy(rows.data(), c->scratch.pass0_offs, rows.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
            uint32_t* totals = rows.data() + (size_t)c->num_blocks * kBins;
            uint32_t smaller = 0u;
            for (int d = 0; d < kBins; ++d) { const uint32_t t = totals[d]; totals[d] = smaller; smaller += t; }
            std::memcpy(dst, rows.data(), bytes);
            return GS_OK;
        }
        case GS_BUF_BACKWARD_ROWS: {
            // what the chain of the last gs_backward* consumed: the rows of the blend summed per splat by the chain's own
            // splat_row_sum (k_bwd_row_sums, gs_backward.hip), launched here and nowhere else.  has_backward: bwd.rows and
            // bwd.scan.offsets are this frame's (a new frame, an upload or a change of the tile rows clears it)
            if (!c->last.has_backward) return fail(c, GS_ERR_INVALID, "gs_debug_read: no gs_backward* on this frame");
            const size_t need = (size_t)c->n * kRowFloats * sizeof(float);
            if (bytes > need) return fail(c, GS_ERR_INVALID, "gs_debug_read: size exceeds buffer");
            float* dev = nullptr;
            HIP_TRY(c, hipMalloc((void**)&dev, need));
            const BackwardFrame f{c->last.fp, c->scene, c->scratch, c->sort.id[si], c->ranges, c->bwd};
            launch_backward_row_sums(f, dev, c->stream);
            hipError_t e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e == hipSuccess && bytes) e = hipMemcpy(dst, dev, bytes, hipMemcpyDeviceToHost);
            (void)hipFree(dev);
            HIP_TRY(c, e);
            return GS_OK;
        }
        default: return fail(c, GS_ERR_INVALID, "gs_debug_read: unknown buffer id");
    }
    if (bytes > avail) return fail(c, GS_ERR_INVALID, "gs_debug_read: size exceeds buffer");
    if (bytes) HIP_TRY(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
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
