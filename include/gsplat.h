/*
 * gsplat.h -- C-ABI of libgsplat_hip.so, the MI355X-native replacement for the per-frame splat
 * path of SiTronXD/vk3dGaussianSplatting (InitSortList -> 4-bit radix sort over 64-bit
 * tile|depth keys -> FindRanges -> RenderGaussians).
 *
 * The reference has no FFI: the seam this library replaces is the public surface of its
 * `Renderer` class plus the `GpuSort` plug-in interface.  Each entry point cites the reference
 * interface it stands in for; paths are relative to /root/reference/vkGaussianSplatting/.
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions: plain pointers and sizes only; every function returns an int status
 * (0 = GS_OK, > 0 = warning, < 0 = error) and never aborts or throws (the reference reports
 * errors through a modal MessageBox and continues, Engine/Dev/Log.cpp:40-43); the caller owns
 * every host pointer for the duration of the call only; the library owns all device memory.
 * A gs_ctx is bound to one GPU and one HIP stream and is not thread-safe; independent contexts
 * may be used concurrently.  Matrices are column-major float[16] exactly as glm::mat4 lies in
 * memory (CamUBO, Engine/Graphics/ShaderStructs.h:37-41).
 */
#ifndef GSPLAT_H
#define GSPLAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_API_VERSION 7   /* 7: gs_backward / gs_backward_device / gs_upload_gaussians_device.  7 (later): gs_visible_count / gs_backward_visible / gs_backward_visible_device (same version: detect them by the presence of the symbols).  7 (later still): gs_default_adam_params / gs_adam_rows_device / gs_upload_rows_device (GS_ADAM_*, gs_adam_params; same version again: detect them by the presence of the symbols).  6: gs_set_outputs / gs_read_output / gs_output_device (GS_OUTPUT_*).  5: gs_config grew count_launches (GS_COUNT_*).  2: gs_config grew tile_order; 3: gs_config starts with struct_size, gs_api_version(),
                              gs_runtime_versions(), gs_dist_* / gs_gather_strips; 4: GS_ROWS_BALANCED + gs_dist_rebalance /
                              gs_dist_bands, gs_render_sharded_async / gs_sharded_frame / gs_sharded_read (two sharded
                              frames in flight, the assembled frame left in HBM), GS_BUF_COLOR for every non-culled splat */

/* status codes */
#define GS_OK 0
#define GS_WARN_OVERFLOW 1      /* more sort elements than capacity; list truncated like InitSortList.comp:140-148 */
#define GS_ERR_INVALID (-1)     /* bad argument / call order */
#define GS_ERR_HIP (-2)         /* HIP runtime failure, see gs_last_error */
#define GS_ERR_NO_SCENE (-3)    /* gs_upload_gaussians / gs_set_resolution not called yet */
#define GS_ERR_IO (-4)          /* file cannot be opened (ResourceManager.cpp:169-173) */
#define GS_ERR_FORMAT (-5)      /* .ply header/property problem */
#define GS_ERR_NO_DEVICE (-6)   /* no usable GPU: the library has NO CPU fallback */

/* The reference's 336-byte record, Engine/Graphics/ShaderStructs.h:59-70:
 * position.xyz0, scale.xyz0 (already exp'd), rot (permuted unit quaternion, .x scalar part),
 * shCoeffs[16] ([0].w = sigmoid opacity), color, covariance (scratch, ignored on upload). */
#define GS_GAUSSIAN_RECORD_BYTES 336u

/* sort back-ends (the GpuSort seam, Engine/Graphics/Sort/GpuSort.h:8-22, selected at compile
 * time in the reference by GPU_SORT_ALGORITHM, Renderer.h:33) */
#define GS_SORT_RADIX4 0u       /* the contractual nine-stage 4-bit LSD radix sort over all key bits (default) */
#define GS_SORT_TILE_BUCKET 1u  /* alternative back-end, identical output: the global 4-bit passes sort by the tile word
                                   only, then every tile's run is depth-sorted inside LDS (csrc/gs_tilesort.hip) */
#define GS_SORT_RADIX4_SPLAT_FIRST 2u /* the same twelve 4-bit passes in another order, identical output: the depth word
                                     of a key is a property of the SPLAT, so the eight passes over it run on the
                                     (depth, splat) list of the emitting splats BEFORE a splat is replicated into its
                                     tiles; InitSortList's emit then walks the splats in depth order and the four
                                     tile-word passes -- stable -- finish the order by (tile, depth).  Moves a third of
                                     the bytes.  Not the default: the default keeps the reference's stage order. */
#define GS_SORT_RADIX8 3u       /* the A/B slot for an 8-bit-digit variant: the same stable LSD sort over all key bits with
                                   half the passes (Count, Scan, Scatter per pass; csrc/gs_sort8.hip), identical output */
#define GS_SORT_RADIX8_SPLAT_FIRST 4u /* GS_SORT_RADIX4_SPLAT_FIRST's stage order with the 8-bit passes */

/* render arithmetic */
#define GS_RENDER_EXACT 0u      /* bit-identical to the CPU oracle (no contraction, pinned exp) */
#define GS_RENDER_FAST 1u       /* fused multiply-adds + hardware exp2; <= 1 step per 8-bit channel, infinite colours
                                   included (a lane that skips an entry leaves its colour untouched); the same pixels
                                   in every launch shape */

typedef struct gs_ctx gs_ctx;

/* Replaces the compile-time constants of Renderer.h:145-147, RadixSort.h:36-39,
 * Camera.cpp:4-5 and Resources/Shaders/Common/Common.glsl:2-15. */
/* RenderGaussians launch shapes (all bit-identical in GS_RENDER_EXACT).  AUTO = GS_RENDER_KERNEL_WORKGROUP_8X8 (a workgroup
 * per tile, an 8 x 8 quadrant per wave) at every size. */
#define GS_RENDER_KERNEL_AUTO 0u
#define GS_RENDER_KERNEL_WAVE_1PX 1u   /* four independent waves per tile, 1 pixel per lane */
#define GS_RENDER_KERNEL_WAVE_2PX 2u   /* two independent waves per tile, 2 pixels per lane */
#define GS_RENDER_KERNEL_WAVE_4PX 4u   /* one wave per tile, 4 pixels per lane */
#define GS_RENDER_KERNEL_WORKGROUP 16u /* one 256-thread workgroup per tile, one pixel per lane (the reference's launch shape);
                                          its four waves walk the tile's list independently, each for a 16 x 4 strip */
#define GS_RENDER_KERNEL_WORKGROUP_8X8 17u /* the same with an 8 x 8 quadrant per wave */

/* Order in which RenderGaussians' tiles are dispatched (same pixels either way). */
#define GS_TILE_ORDER_LONGEST_FIRST 0u /* by list length, longest first: one small launch behind FindRanges (default) */
#define GS_TILE_ORDER_RASTER 1u        /* row-major, like the reference's dispatch (Subrenderer.cpp:330-333) */

/* The Count stage of the 4-bit radix sort (GS_SORT_RADIX4; RadixSortCount.comp:40-91): one launch per pass, or one launch per
 * SORT with every Scatter launch counting the next pass's digits of the keys it stores ("fed" counts: for short lists -- a
 * tile-row band of a multi-GPU frame, a small frame -- where a pass is two fixed launch latencies and little else).  Same
 * sorted list either way. */
#define GS_COUNT_AUTO 0u      /* fed when a recent frame held at most 1024 groups of 2048 elements = 2.1 M (default) */
#define GS_COUNT_PER_PASS 1u  /* always a Count launch per pass */
#define GS_COUNT_FED 2u       /* always fed (correct at every size; slow for long lists) */

/* near_plane .. fov_y stand in for the reference's compile-time constants and hold for every frame of the context.
 * gs_create refuses, with GS_ERR_INVALID and a message that names the field: any of the five that is not finite,
 * near_plane <= 0, far_plane <= near_plane, ndc_cull <= 0, in_view_limit <= 0, and fov_y outside (0, pi) -- the tangent of
 * its half angle must be finite and positive. */
typedef struct gs_config {
    uint32_t struct_size;     /* sizeof(gs_config) as the CALLER's header declares it (gs_default_config fills it in).
                                 gs_create copies that many bytes and keeps its defaults for fields the caller's
                                 header does not know yet; a struct larger than the library's is refused. */
    int32_t device_ordinal;   /* HIP device index */
    uint32_t tile_size;       /* 16; only 16 is supported (TILE_SIZE) */
    float near_plane;         /* 0.1f   Camera::NEAR_PLANE */
    float far_plane;          /* 100.0f Camera::FAR_PLANE */
    float ndc_cull;           /* 1.3f   CULLING_NDC_LIMIT */
    float in_view_limit;      /* 0.8f   IN_VIEW_LIMIT */
    float fov_y;              /* 3.1415f*0.5f FOV_Y (the covariance one, not the projection's) */
    uint32_t sort_algorithm;  /* GS_SORT_* */
    uint32_t render_mode;     /* GS_RENDER_* */
    uint32_t record_timings;  /* 0 (default, like the reference's commented-out RECORD_GPU_TIMES, GfxSettings.h:7) = no
                                 events; 1 = hipEvents at the reference's 7 timestamp points (Renderer.cpp:557-622);
                                 2 = additionally one event pair around every Scatter launch (roofline measurement) */
    uint32_t render_kernel;   /* GS_RENDER_KERNEL_*: how a tile maps to waves in RenderGaussians; same pixels either way */
    uint32_t tile_order;      /* GS_TILE_ORDER_* */
    uint32_t count_launches;  /* GS_COUNT_*: GS_SORT_RADIX4 frames and the stand-alone 4-bit sorter; ignored by the other sorters */
} gs_config;

/* The five buckets of Renderer.cpp:471-475 (ms) + the sort element count ("Elements To Sort"
 * in README.md:43-93).  InitSortList includes the per-frame clears, RadixSort includes the
 * IndirectSetup-equivalent, exactly like the reference's timestamp placement (Renderer.cpp:557-622).
 * With GS_SORT_RADIX4_SPLAT_FIRST the two stages interleave (project + splat list | depth passes | sums + emit |
 * tile-word passes): init_sort_list_ms and radix_sort_ms are the sums of their two halves, and with
 * record_timings == 2 scatter_* describe the depth passes over the SPLAT list (bytes per splat), scatter_tile_* the
 * tile-word passes over the elements. */
typedef struct gs_timings {
    float init_sort_list_ms;
    float radix_sort_ms;
    float find_ranges_ms;
    float render_ms;
    float total_ms;
    uint32_t num_sort_elements;   /* min(counter, capacity) */
    uint32_t overflowed;          /* counter > capacity this frame */
    uint64_t emitted_elements;    /* un-truncated counter */
    float scatter_ms_avg;         /* record_timings == 2: mean duration of one Scatter launch that moves key + payload
                                     (24 bytes per element; the dominant kernel) */
    uint32_t scatter_launches;    /* number of those launches in the frame (the 8 depth-word passes; all passes
                                     with GS_SORT_TILE_BUCKET) */
    float scatter_tile_ms_avg;    /* mean duration of a tile-word pass of the frame path, which leaves the already
                                     sorted depth words behind (16 bytes per element) */
    uint32_t scatter_tile_launches;
    float scatter_bytes_per_elem;       /* bytes per element really moved (read + written) by the launches above, mean */
    float scatter_tile_bytes_per_elem;
} gs_timings;

/* RECORD_CPU_TIMES (GfxSettings.h:6; Renderer.cpp:299-314, 343-352, 399-456): host-side milliseconds of the last
 * gs_render* call, always recorded (four clock reads per frame).  The reference's four figures map to:
 * waitForFence -> wait_ms (host blocked until the GPU has finished the frame; 0 for the async variant),
 * recordCommandBuffer -> record_ms (enqueueing the frame's launches), present -> present_ms (the copy of the frame to
 * the host in gs_render; 0 for the device variants), CPU frame time -> cpu_frame_ms (entry of this call minus entry of
 * the previous one). */
typedef struct gs_host_timings {
    float wait_ms;
    float record_ms;
    float present_ms;
    float cpu_frame_ms;
} gs_host_timings;

/* Scene-derived sizes: Renderer.cpp:696-701 (tiles), :725 (capacity), RadixSort.cpp:203-204 (bits). */
typedef struct gs_scene_info {
    uint32_t num_gaussians;
    uint32_t width, height;
    uint32_t tiles_x, tiles_y;
    uint32_t capacity;            /* C = ceilPow2(N + 64*16*T) */
    uint32_t num_sort_bits;       /* 4 * P */
    uint32_t row_begin, row_end;  /* tile-row band rendered by this context */
    uint32_t tile_word_bytes;     /* how the frame's sort list stores a tile id: 2 (uint16 index among the context's own
                                     tiles, at most 65535 of them) or 4; callers always see uint32 global ids */
    uint32_t row_stride;          /* the context renders tile rows first_row + k * row_stride < row_end, k < rows_owned */
    uint32_t first_row;
    uint32_t rows_owned;
} gs_scene_info;

/* buffers readable through gs_debug_read (state after the last gs_render*) */
#define GS_BUF_SORTED_TILE 0   /* uint32[num_sort_elements]  high half of the key   */
#define GS_BUF_SORTED_DEPTH 1  /* uint32[num_sort_elements]  low half of the key    */
#define GS_BUF_SORTED_ID 2     /* uint32[num_sort_elements]  gaussian index payload */
#define GS_BUF_RANGES 3        /* uint32[tiles][2]           {start,end} per tile (GaussianTileRangeData.xy) */
#define GS_BUF_COLOR 4         /* float[N][4]                GaussianData.color: rgb + opacity of EVERY splat that passed both culls
                                                             (InitSortList.comp:124-127), zero for the culled ones.  A frame evaluates
                                                             the colour of the splats that emit an element (nothing else is ever read);
                                                             the others are evaluated by this call, on demand, from the last frame's
                                                             camera.  A context that owns a SUBSET of the tile rows (gs_set_tile_rows*)
                                                             does not project splats that cannot reach its rows: there the buffer
                                                             holds the emitting splats only */
#define GS_BUF_COV 5           /* float[N][4]                GaussianData.covariance (w = 0) */
#define GS_BUF_COUNT 6         /* uint64[1]                  un-truncated element counter */
#define GS_BUF_UNSORTED_TILE 7 /* uint32[num_sort_elements]  list as emitted by InitSortList */
#define GS_BUF_UNSORTED_DEPTH 8
#define GS_BUF_UNSORTED_ID 9
#define GS_BUF_IMAGE 10        /* uint8[H][W][4]             internal framebuffer */
#define GS_BUF_RASTER_OPACITY 11 /* float[N]                 the opacity RenderGaussians multiplied in the last frame: of every
                                                             splat that emitted an element its raster opacity (the scene's, 0 where
                                                             the 2 x 2 determinant vanishes, times the anti-aliasing factor under
                                                             gs_set_antialias), 0 for every other splat */
/* The work the last frame decided NOT to do (values never show it: a frame that skips nothing has the same pixels) */
#define GS_BUF_WAVE_WROTE 12   /* uint8[ceil(N / 64)]        per wave of 64 splats, a mask of its four quarters (bit q = splats
                                                             64 w + 16 q ..): InitSortList stored their raster records.  Whole grid
                                                             or interleaved rows: a quarter with a splat that emits an element.  A
                                                             contiguous band of tile rows: 0xF when a splat of the wave emits into
                                                             the band, else 0.  Valid after a frame and after
                                                             gs_debug_init_sort_list */
#define GS_BUF_BAND_BLOCKS 13  /* uint32[1 + count]          word 0 = count, then the blocks of 256 splats InitSortList projected,
                                                             ascending: block | skip mask << 28 (bit w of the mask: wave w of the
                                                             block was not projected).  A caller reads 4 bytes to learn the count,
                                                             then 4 * (1 + count).  A contiguous band of tile rows: what the band
                                                             cull kept.  Every row, or interleaved rows: every block, mask 0 */
#define GS_BUF_TILE_ORDER 14   /* uint32[owned tiles]        the k-th tile RenderGaussians dispatched, a global tile id: longest
                                                             list first by bit length of (end - start), any order among equal bit
                                                             lengths; GS_TILE_ORDER_RASTER: the owned tiles ascending.  Valid after
                                                             a frame only */
#define GS_BUF_PASS0_OFFSETS 15 /* uint32[blocks + 1][16]    pass 0 of the depth sort as InitSortList ran it (blocks of 256 splats):
                                                             row b, word d = the elements with depth_key & 15 == d that the splats
                                                             before block b emit; the last row = the sixteen digit bases (elements
                                                             of smaller digits).  GS_ERR_INVALID unless the last frame took that
                                                             path: GS_SORT_RADIX4 with a Count launch per pass, record_timings < 2,
                                                             every tile row, no overflow */
#define GS_BUF_BACKWARD_ROWS 16 /* float[N][10]              what the per-splat chain of the last gs_backward* / gs_backward_visible*
                                                             on this context consumed: per splat the sum over its list elements of
                                                             the blend's derivatives, in the order and with the bits the chain
                                                             added them.  Columns: dL/d of the screen position (sx, sy), of the
                                                             inverse 2-D covariance (ix, iy, iz), of the colour (r, g, b), of the
                                                             raster opacity and of the view depth.  All zero for a splat that is
                                                             not in the list.  A band context (gs_set_band_gradients): the band's
                                                             partial sums.  GS_ERR_INVALID ("no gs_backward* on this frame") until
                                                             a gs_backward* form has run on the last frame */

/* GS_API_VERSION of the library that is actually loaded: compare with the header's before anything else
 * (gsplat.hpp and the Python binding do). */
uint32_t gs_api_version(void);
/* HIP_VERSION the library was compiled against, and the HIP runtime / driver versions of the libamdhip64 the process
 * really bound (a process holds ONE HIP runtime -- INTEGRATION.md, "One HIP runtime per process"); any pointer may be NULL. */
int gs_runtime_versions(int* hip_build, int* hip_runtime, int* hip_driver);

void gs_default_config(gs_config* cfg);

/* Renderer::init (Renderer.cpp:688-694) + GpuSort::singleInitResources (RadixSort.cpp:23-142). */
int gs_create(const gs_config* cfg, gs_ctx** out);
/* Renderer::cleanup (Renderer.cpp:230-270) + RadixSort::cleanup (RadixSort.cpp:655-674).  Waits for the context's
 * stream, frees everything the context owns and the context itself, and returns GS_OK -- always: there is no failure
 * that leaves the handle alive, so it must not be used (not even for gs_last_error) once this has been called.
 * NULL is accepted.  A scene shared through gs_share_scene lives on while another context holds it. */
int gs_destroy(gs_ctx* ctx);
/* Text of the last error on ctx (ctx may be NULL: last gs_create failure). Log::error, Dev/Log.cpp:40-43. */
const char* gs_last_error(const gs_ctx* ctx);

/* Renderer::initForScene, gaussian upload (Renderer.cpp:712-724): n records of
 * GS_GAUSSIAN_RECORD_BYTES each, as ResourceManager::getGaussians() returns them
 * (ResourceManager.h:53).  Converted once to the device SoA layout. */
int gs_upload_gaussians(gs_ctx* ctx, const void* aos336, uint32_t n);
/* The same from DEVICE memory (e.g. a torch tensor's data_ptr, float32 [n][84]), converted by the upload kernel directly.
 * With the n of the scene the context holds, the planes are rewritten in place: enqueued on the context's stream, no host
 * sync; every context sharing the scene (gs_share_scene) renders the new values; resolution, scratch and captured graphs
 * stay.  The caller orders the writes of aos336_dev before this call (e.g. synchronises the stream that wrote it).  With
 * another n it behaves like gs_upload_gaussians: a new scene (waits), gs_set_resolution must follow. */
int gs_upload_gaussians_device(gs_ctx* ctx, const void* aos336_dev, uint32_t n);
/* Frames in flight (the reference keeps GfxSettings::FRAMES_IN_FLIGHT = 3 command buffers, GfxSettings.h:15,
 * Renderer.cpp:304-310, 514): `ctx` renders the gaussians already uploaded to `owner` -- the read-only arrays
 * are shared, everything a frame writes (sort lists, ranges, raster records, image, stream, timings) stays per
 * context, so F contexts on F streams keep F frames in flight on one GPU.  Follow with gs_set_resolution.
 * The arrays are reference-counted inside the library: the contexts may be destroyed in any order, and a new
 * gs_upload_gaussians / gs_load_ply on one of them leaves the others rendering the arrays they hold. */
int gs_share_scene(gs_ctx* ctx, gs_ctx* owner);

/* ResourceManager::loadGaussians (ResourceManager.cpp:167-300): .ply with the INRIA property names -> records
 * (axis flips, exp, quaternion permutation, sigmoid, SH repack, Morton order) -> upload.  binary_little_endian is the
 * fast path (two sweeps over 16 MB chunks: 2.3 s for a 1.45 GB Garden-size file); binary_big_endian and ascii are
 * accepted; ascii is tokenised twice (chunked std::from_chars: about 0.3 GB of text per second over both sweeps).  The path
 * must name a seekable file. */
int gs_load_ply(gs_ctx* ctx, const char* path);
/* The same conversion without a context: writes up to max_records records to aos336_out (may be
 * NULL to query) and the record count to n_out. */
int gs_convert_ply(const char* path, void* aos336_out, uint32_t max_records, uint32_t* n_out);
/* Text of the last gs_load_ply / gs_convert_ply failure on this thread (happly throws instead,
 * happly.h:1089-1094). */
const char* gs_ply_last_error(void);
/* The way back (no reference counterpart): rows float[n][84] (HOST) -> a .ply gs_load_ply reads: binary_little_endian, one
 * `vertex` element of 62 float properties in the INRIA order -- x y z nx ny nz f_dc_0..2 f_rest_0..44 opacity scale_0..2
 * rot_0..3 -- the normals 0.  Per row r, the inverse of the loader's conversion:
 *   x, y, z = -r[0], -r[1], r[2];   rot_0..3 = r[10], -r[11], -r[8], -r[9];   f_dc_c = r[12 + c];
 *   f_rest_(c + 15 ch) = r[16 + 4 c + ch]                                       (c = 0..14, ch = 0..2)
 *   GS_PLY_FROM_RAW     (rows in the raw space below): scale_k = r[4 + k] and opacity = r[15] as they are -- the file then
 *                       holds the trainer's parameters exactly, a lossless checkpoint;
 *   GS_PLY_FROM_RECORDS (rows as the frame reads them): scale_k = std::log(s < FLT_MIN ? FLT_MIN : s), opacity =
 *                       std::log(c / (1 - c)) with c = the opacity clamped to [2^-24, 1 - 2^-24], in float32 (the host's libm).
 * Rows are written in the order given; the loader's Morton sort is stable, so a cloud that came from the loader (or from
 * gs_densify_device on one) loads again in the same order.  Written in chunks of a few MB: no second copy of the cloud.
 * GS_ERR_IO with a message in gs_ply_last_error when the file cannot be created or a write comes up short; GS_ERR_INVALID
 * for a NULL path or rows, n == 0 or an unknown space. */
#define GS_PLY_FROM_RECORDS 0u
#define GS_PLY_FROM_RAW 1u
int gs_write_ply(const char* path, const float* rows, uint32_t n, uint32_t space);

/* Frame output sink: where the reference's frame goes to the swapchain image
 * (RenderGaussians.comp:150 imageStore, presented by Renderer.cpp:341-397) a windowless host writes the
 * RGBA8 frame of gs_render to disk.  Format by extension: ".ppm" (binary P6, alpha dropped) or ".png"
 * (8-bit RGBA).  GS_ERR_IO when the file cannot be written, GS_ERR_INVALID for another extension. */
int gs_write_image(const char* path, const uint8_t* rgba, uint32_t width, uint32_t height);

/* Swapchain extent -> tile grid, list capacity and pass count (Renderer.cpp:696-701, 725-755;
 * RadixSort::initForScene, RadixSort.cpp:144-205).  Must follow gs_upload_gaussians. */
int gs_set_resolution(gs_ctx* ctx, uint32_t width, uint32_t height);
/* Multi-GPU extension (no reference counterpart): this context emits/sorts/renders only tile rows
 * [row_begin,row_end) with GLOBAL tile ids, so keys, per-tile order and pixels equal the 1-GPU
 * result.  Default after gs_set_resolution: all rows. */
int gs_set_tile_rows(gs_ctx* ctx, uint32_t row_begin, uint32_t row_end);
/* Same extension, interleaved: this context owns tile rows phase, phase + stride, phase + 2 stride, ... of the whole
 * grid (rank r of R: phase = r, stride = R), which evens out the per-rank load when the splat density varies over the
 * height of the frame.  compact_output != 0: gs_render_device* address the image in compact rows -- the pixel rows of
 * the k-th owned tile row start at row 16 k -- i.e. they write the strip a rank contributes to the gather
 * (ceil(rows_owned) * 16 rows of `width` pixels); gs_render (host image) always writes the real rows. */
int gs_set_tile_rows_interleaved(gs_ctx* ctx, uint32_t phase, uint32_t stride, uint32_t compact_output);
int gs_get_scene_info(const gs_ctx* ctx, gs_scene_info* out);

/* Multi-GPU extension, the exchange step (no reference counterpart): one process per GPU, every
 * rank renders its tile rows into a strip (gs_render_device* with gs_set_tile_rows*), and the strips meet on the
 * root over RCCL -- point-to-point transfers over xGMI inside a node, enqueued on the context's stream behind the
 * frame that wrote the strip.  RCCL is bound at gs_dist_init (librccl.so.1 by name, or the copy the process
 * already holds; the environment variable GS_RCCL_LIBRARY names another build by path), not at link time.
 *   gs_dist_unique_id : ncclGetUniqueId -- call on ONE rank, hand the GS_DIST_UNIQUE_ID_BYTES bytes to the others by
 *                       any means (pipe, file, MPI, torch.distributed broadcast);
 *   gs_dist_init      : ncclCommInitRank for this context's GPU; collective over all `world` ranks;
 *   gs_gather_strips  : strip_dev = this rank's `bytes` bytes on the device (the SAME `bytes` and `root` on every
 *                       rank: strips are padded to one size); gathered_dev = world * bytes bytes on the root's device
 *                       (rank r's strip at offset r * bytes; ignored on other ranks, may be NULL there).  Every rank must
 *                       call it, in the same order as the others.  Asynchronous: ordered on the context's stream, wait
 *                       with gs_synchronize;
 *   gs_dist_destroy   : ncclCommDestroy (gs_destroy does it too). */
#define GS_DIST_UNIQUE_ID_BYTES 128
int gs_dist_unique_id(void* id_out);
int gs_dist_init(gs_ctx* ctx, const void* unique_id, int rank, int world);
int gs_gather_strips(gs_ctx* ctx, const void* strip_dev, void* gathered_dev, size_t bytes, int root);
int gs_dist_destroy(gs_ctx* ctx);
/* The same for a host that holds no device memory of its own -- Renderer::draw on R GPUs (Renderer.cpp:297-515):
 *   gs_dist_shard_rows : after gs_set_resolution + gs_dist_init (again after every gs_set_resolution, and after any
 *                        gs_set_tile_rows* of the caller's own: the buffers of the sharded frame belong to the rows dealt
 *                        HERE, and gs_render_sharded* refuse a context whose rows have been changed since).  Rank r of R
 *                        takes its tile rows --
 *                          GS_ROWS_CONTIGUOUS  a band of ceil(Ty / R) rows;
 *                          GS_ROWS_INTERLEAVED rows r, r + R, ...: even load whatever the scene, at the price of
 *                                              InitSortList's block cull (every rank's rows span the whole frame);
 *                          GS_ROWS_BALANCED    contiguous bands whose EDGES follow the scene: equal row counts at first,
 *                                              moved by gs_dist_rebalance towards equal cost --
 *                        and the library allocates the buffers of two sharded frames in flight (every rank its rows; rank 0
 *                        the assembled frames).
 *   gs_render_sharded_async : every rank calls it with the same camera: the rank's rows are rendered on the context's
 *                        stream; the exchange follows on a stream of the library's own behind an event, so it runs beside
 *                        the NEXT frame's kernels; bands land in place in rank 0's frame (interleaved rows: re-ordered by R
 *                        strided copies).  Returns after enqueueing; the assembled frame stays in rank 0's HBM.  A rank
 *                        whose own frame fails still takes part in the exchange before it returns its error, so the others
 *                        are not left waiting.
 *   gs_sharded_frame   : waits (host) until the exchange of the last (which = 0) or the last-but-one (which = 1) sharded
 *                        frame has finished; on rank 0 *frame_dev is the device pointer of that frame (height * width * 4
 *                        bytes, valid until the second gs_render_sharded* call from now), NULL on the other ranks.
 *   gs_sharded_read    : the same, and copies the frame to rgba_out (HOST) on rank 0.
 *   gs_render_sharded  : gs_render_sharded_async + gs_sharded_read(0) + the timings of this rank's own rows
 *                        (gs_get_timings, with record_timings on): the synchronous form.  rgba_out: HOST, height*width*4
 *                        bytes as in gs_render; ignored on the other ranks, may be NULL.  The frame is bit-identical to the
 *                        one-GPU frame of gs_render.
 *   gs_dist_rebalance  : GS_ROWS_BALANCED, collective (every rank, same order as the frames, e.g. every 32 frames): each
 *                        rank contributes the sort-element counts of its tile rows (the last frame's tile ranges) and the
 *                        GPU time of its share; after one exchange of R (R - 1) messages of Ty + 1 words every rank holds
 *                        the same vectors and derives the same new edges: weight(row) = elements(row) x (share time / share
 *                        elements of the rank that rendered it), edges at equal weight prefixes, moved only for a predicted
 *                        gain of 3 % on the slowest rank.  Waits for the frames in flight.  *moved_out (may be NULL) = 1
 *                        when the edges moved (the next frame re-captures its hipGraph).  With GS_REBALANCE_ELEMENTS_ONLY in the
 *                        environment (of every rank) the share times are ignored and the bands are cut by element counts
 *                        alone: for ranks whose times are not comparable, e.g. several ranks sharing one GPU.
 *   gs_dist_bands      : the R + 1 band edges (tile rows) of a contiguous or balanced dealing; count must be R + 1.
 * Collective safety: these calls pair with the other ranks' calls.  A rank that fails a PRECONDITION (no shard, rows changed
 * behind the library's back, a NULL rgba_out on rank 0, an allocation that failed in gs_dist_shard_rows) returns before the
 * exchange and its peers wait in theirs: check the status of gs_dist_shard_rows on every rank (e.g. exchange a flag over the
 * channel that carried the unique id) before the first frame.  A failure of the rank's own FRAME is collective-safe (above), and so
 * is a HIP error of the calls around the exchange (the event / copy calls of gs_render_sharded_async and gs_dist_rebalance once
 * the preconditions have passed): the rank still takes part in the exchange and reports its first error afterwards. */
#define GS_ROWS_CONTIGUOUS 0u
#define GS_ROWS_INTERLEAVED 1u
#define GS_ROWS_BALANCED 2u
int gs_dist_shard_rows(gs_ctx* ctx, uint32_t dealing);
int gs_render_sharded_async(gs_ctx* ctx, const float view[16], const float proj[16], const float cam_pos[3], uint32_t sh_mode);
int gs_sharded_frame(gs_ctx* ctx, uint32_t which, void** frame_dev);
int gs_sharded_read(gs_ctx* ctx, uint32_t which, uint8_t* rgba_out);
int gs_render_sharded(gs_ctx* ctx, const float view[16], const float proj[16], const float cam_pos[3],
                      uint32_t sh_mode, uint8_t* rgba_out);
int gs_dist_rebalance(gs_ctx* ctx, uint32_t* moved_out);
int gs_dist_bands(const gs_ctx* ctx, uint32_t* edges_out, uint32_t count);
/* The partition rule by itself (pure host arithmetic, no context, no GPU): world + 1 edges of contiguous bands over
 * tiles_y rows whose weights are as equal as whole rows allow -- edge r at the row boundary whose weight prefix is nearest
 * to r / world of the total, every band at least one row while there are rows to give; all-zero or non-finite weights
 * count as equal ones.  For hosts that run their own exchange (bench.py's torch path: dist.balanced_row_partition is the
 * same rule in Python). */
int gs_balance_rows(const double* row_weights, uint32_t tiles_y, uint32_t world, uint32_t* edges_out);

/* The sh_mode of a frame: which SH coefficients its colour sums.  0, 1 and 2 are the reference viewer's three
 * (Camera.h:7-12); GS_SH_DEGREE_1 and GS_SH_DEGREE_2 are the degrees between them, which a trainer that raises the active
 * degree step by step needs (no reference counterpart; callers detect them by the symbol gs_sh_mode_of_degree,
 * GS_API_VERSION is unchanged).  The value 3 names no mode: it was refused before the degrees existed, callers were promised
 * that refusal, and it stays refused.  Use the names, or gs_sh_mode_of_degree; the numbers do not follow the degree.
 * With K = 4 (GS_SH_DEGREE_1) or K = 9 (GS_SH_DEGREE_2) the colour is GS_SH_ALL_BANDS's expression with the sum cut at K:
 * res.c = sum over i < K of shCoeffs[i].c * basis[i] in ascending i, then + 0.5f, then max(res, 0) -- same arithmetic, same
 * operand order.  A frame in these modes never reads the coefficients K..15 (no load is issued: a NaN there changes
 * nothing), and neither do its gradients.  Every call that takes an sh_mode accepts all five (gs_render*,
 * gs_render_sharded*, gs_debug_init_sort_list; gs_debug_read(GS_BUF_COLOR) follows the last frame's mode); the value 3 and
 * every value of 6 or more are GS_ERR_INVALID with a message, nothing enqueued. */
#define GS_SH_ALL_BANDS 0u        /* coefficients 0..15 (degree 3) */
#define GS_SH_SKIP_FIRST_BAND 1u  /* coefficients 1..15, the reference's oddity as it is */
#define GS_SH_ONLY_FIRST_BAND 2u  /* coefficient 0 (degree 0) */
#define GS_SH_DEGREE_2 4u         /* coefficients 0..8 */
#define GS_SH_DEGREE_1 5u         /* coefficients 0..3 */
/* The mode of an active SH degree: 0, 1, 2, 3 -> GS_SH_ONLY_FIRST_BAND, GS_SH_DEGREE_1, GS_SH_DEGREE_2, GS_SH_ALL_BANDS.
 * Pure host arithmetic, no context, no GPU.  GS_ERR_INVALID for degree > 3 or a NULL sh_mode_out (nothing written). */
int gs_sh_mode_of_degree(uint32_t degree, uint32_t* sh_mode_out);

/* Renderer::draw (Renderer.cpp:297-515): updateUniformBuffer(view, proj) (:531-538), the push
 * constants of Subrenderer.cpp:152-160 (camPos, shMode as an INTEGER: one of GS_SH_* above), then the recorded
 * frame (:540-629).  rgba_out: height*width*4 bytes on the HOST, row-major, top row first,
 * R,G,B,A with A = 255 (the R8G8B8A8_UNORM storage image of Swapchain.cpp:27).  Synchronous. */
int gs_render(gs_ctx* ctx, const float view[16], const float proj[16], const float cam_pos[3],
              uint32_t sh_mode, uint8_t* rgba_out);
/* Same frame, image left in HBM: rgba_out_device is a DEVICE pointer of height*width*4 bytes
 * (e.g. a torch tensor's data_ptr) or NULL for the internal framebuffer (GS_BUF_IMAGE).
 * Enqueued on the context's stream; returns after the frame has completed (timings valid). */
int gs_render_device(gs_ctx* ctx, const float view[16], const float proj[16],
                     const float cam_pos[3], uint32_t sh_mode, void* rgba_out_device);
/* As gs_render_device but returns right after enqueueing (no host sync, timings not updated):
 * the CPU never waits on the GPU inside a frame, like the reference's single vkQueueSubmit. */
int gs_render_device_async(gs_ctx* ctx, const float view[16], const float proj[16],
                           const float cam_pos[3], uint32_t sh_mode, void* rgba_out_device);
/* Wait for everything enqueued on the context's stream (vkDeviceWaitIdle, Renderer.cpp:459). */
int gs_synchronize(gs_ctx* ctx);

/* computeDiffs buckets of the last synchronous frame (Renderer.cpp:463-475). */
int gs_get_timings(const gs_ctx* ctx, gs_timings* out);
/* RECORD_CPU_TIMES figures of the last gs_render* call (Renderer.cpp:399-456). */
int gs_get_host_timings(const gs_ctx* ctx, gs_host_timings* out);

/* No reference counterpart (its buffers are only visible in a GPU debugger): copies one device
 * buffer of the last frame to dst; bytes must not exceed the buffer's size. */
int gs_debug_read(gs_ctx* ctx, int which, void* dst, size_t bytes);

/* Optional per-pixel outputs of a frame (no reference counterpart: RenderGaussians.comp:147-151 stores vec4(color, 1) and
 * nothing else).  A per-context mask, empty by default; with it empty every frame is exactly what it is without it.
 *   GS_OUTPUT_RGBA32F  float[H][W][4]: r, g, b = the pixel's accumulated colour sum_i T_i * alpha_i * c_i BEFORE the clamp
 *                      (premultiplied); a = 1 - T_end, T_end = the transmittance after the last entry whose colour was added
 *                      -- for a pixel that ends on the early-out of :136-140 (colour added, then break at nextT < 1e-4)
 *                      that is the nextT of the entry, so colour and alpha describe the same entries.  A pixel nothing
 *                      contributes to: (0, 0, 0, 0).
 *   GS_OUTPUT_DEPTH    float[H][W]: sum_i T_i * alpha_i * z_i, z_i = -viewSpacePos.z of the splat (viewMat * vec4(pos, 1), the
 *                      value getDepthKey quantises, InitSortList.comp:70-80: positive in front of the camera), blended
 *                      exactly like a fourth colour channel -- same weights, same entries, same early-out.  The expected
 *                      depth is depth / a, where a > 0 (the caller's division).
 * Both buffers are addressed like the RGBA8 image of the frame: row-major, top row first; a tile-row band
 * (gs_set_tile_rows*) writes the same rows as the image, compact rows under gs_set_tile_rows_interleaved(.., compact_output
 * = 1) with gs_render_device*; rows the context does not own are left untouched (zero after gs_set_outputs or
 * gs_set_resolution).  The RGBA8 frame is byte-identical with or without outputs, for every sorter, render mode and launch
 * shape; quantising the float colour with the UNORM expression floor(clamp(c, 0, 1) * 255 + 0.5) gives its bytes.
 * GS_RENDER_EXACT: alpha and depth use the colour's operation order (d = d + (T * alpha) * z, no contraction, 1 - T at
 * the end): bit-reproducible against a CPU restatement.  GS_RENDER_FAST may contract them, like its colour.
 *   gs_set_outputs   : mask = 0 (RGBA8 only) or any OR of GS_OUTPUT_*; waits for the context's stream, (re)allocates the
 *                      buffers (again at every gs_set_resolution).  GS_ERR_INVALID for unknown bits.
 *   gs_read_output   : which = one enabled GS_OUTPUT_* bit; waits for the context's stream and copies the last frame's
 *                      buffer (H * W * 16 or H * W * 4 bytes) to dst on the HOST; bytes must be at least that.
 *   gs_output_device : the device pointer of that buffer and its size (bytes may be NULL).  Valid until the next
 *                      gs_set_outputs, gs_set_resolution, gs_set_tile_rows* or gs_destroy; it holds the last enqueued frame's
 *                      values once gs_synchronize has returned (gs_render_device_async works).
 * Both fail with GS_ERR_INVALID (message in gs_last_error) for a which that is unknown or not enabled, a bytes that is too
 * small, and when no frame has been rendered since the outputs were enabled or resized.
 * Sharded frames (gs_dist_shard_rows, gs_render_sharded*) do not gather these buffers: a sharded call on a context with a
 * non-zero mask returns GS_ERR_INVALID and enqueues nothing. */
#define GS_OUTPUT_RGBA32F 1u
#define GS_OUTPUT_DEPTH 2u
int gs_set_outputs(gs_ctx* ctx, uint32_t mask);
int gs_read_output(gs_ctx* ctx, uint32_t which, void* dst, size_t bytes);
int gs_output_device(gs_ctx* ctx, uint32_t which, void** dev_out, size_t* bytes);

/* Gradients of a frame (no reference counterpart): how the last frame enqueued on the context changes with its gaussians.
 * Input: dL/dRGBA32F float[H][W][4] (the quantities of GS_OUTPUT_RGBA32F: premultiplied colour before the clamp and
 * alpha = 1 - T_end; the outputs themselves need not be enabled) and dL/dDEPTH float[H][W] (GS_OUTPUT_DEPTH's quantity;
 * NULL = zero), in real rows, top row first.  Output: dL/d(record) float[N][84] in the 336-byte layout and record order of
 * gs_upload_gaussians.  Gradients go to the 59 fields a frame reads -- position.xyz, scale.xyz, rot (all four, used
 * unnormalised as getRotMat uses it), shCoeffs[k].rgb for the coefficients the frame's sh_mode uses (0: all 16, 1: 1..15,
 * 2: 0 only, 4: 0..8, 5: 0..3) and shCoeffs[0].a (opacity); every other float is 0, and so is the whole record of a splat
 * that was culled or emitted no element.  In GS_SH_DEGREE_1 / _2 the coefficient fields K..15 are exactly +0.0f, dL/d(position)
 * carries the direction term of the K active coefficients only, and no inactive SH plane is read.  The camera's gradients
 * are a call of their own behind this one: gs_backward_camera* below.
 * Boundary convention: the frame is piecewise smooth, and the gradient is the derivative of the branch the frame took with
 * every discrete decision held fixed -- the near-plane and NDC culls, tile boxes, depth keys and the sorted order; which
 * entries a pixel blends (f > 0 or alpha < 1/255 skip) and the entry it stops on (nextT < 1e-4, RenderGaussians.comp:127-140);
 * det == 0 (opacity 0: no gradient); max(colour, 0) in getShColor (no derivative where the colour is below 0); the
 * IN_VIEW_LIMIT clamp of x/z and y/z in getCovarianceMatrix (Common.glsl:60-63: a clamped ratio passes no derivative); in
 * an anti-aliased frame (gs_set_antialias) the floor under det0 / det and the cap at 1 (there the factor is a constant,
 * sqrt(2.5e-5) or 1: the opacity gets its share, the covariance nothing).  A
 * frame whose list overflowed (GS_WARN_OVERFLOW) is differentiated as drawn, truncated.  The frame's sorted list, ranges
 * and raster records must still be in HBM (they are until the next frame on the context); the scene's current planes are
 * read.  Bitwise reproducible: no float atomics, the rows of a splat summed in a fixed order -- the same gradients for
 * every sorter, launch shape, tile order and GS_COUNT_* mode.  Scratch: 40 bytes per list element of capacity + 4 bytes
 * per gaussian (+ 4 bytes per gaussian and 8 bytes per 256 gaussians for the visible form below), allocated on the first call
 * and freed with the resolution.
 *   gs_backward        : HOST pointers; synchronous (grad_records is written when it returns).
 *   gs_backward_device : the same arguments as DEVICE pointers; enqueued on the context's stream, no host sync.
 * GS_ERR_INVALID with a message in gs_last_error, nothing enqueued: a NULL grad_rgba32f or grad_records, no frame since the
 * last gs_set_resolution, gs_set_tile_rows*, gs_debug_init_sort_list or upload, a GS_RENDER_FAST context, a context that
 * owns a subset of the tile rows (unless gs_set_band_gradients is on: see there), a sharded context (gs_dist_shard_rows). */
int gs_backward(gs_ctx* ctx, const float* grad_rgba32f, const float* grad_depth, float* grad_records);
int gs_backward_device(gs_ctx* ctx, const float* grad_rgba32f, const float* grad_depth, float* grad_records);

/* Visible-splat form of gs_backward.  V = the splats g with tiles_touched != 0 in the last frame (they passed both culls and
 * their tile box is not empty -- including splats whose elements were all cut by an overflowed list: their rows are zero),
 * in ascending g.  ids_out[i] = the i-th such g; grad_rows_out[i][84] = bit for bit row ids_out[i] of what gs_backward
 * writes for the same frame and the same dL/d(outputs).  Rows of splats outside V are never written anywhere: no
 * N-sized output exists on this path.
 *   gs_visible_count           : |V| of the last frame (HOST uint32); waits for the context's stream.
 *   gs_backward_visible        : HOST pointers, synchronous.  *count_out = |V| always (not clamped).  At most max_rows
 *                                ids / rows are written (the first max_rows of V); nothing beyond them is touched.
 *                                Returns GS_WARN_OVERFLOW when |V| > max_rows, else GS_OK.
 *   gs_backward_visible_device : all pointers DEVICE (count_out: one uint32 on the device); enqueued on the context's
 *                                stream, no host sync; always GS_OK once enqueued -- the caller compares *count_out with
 *                                max_rows after synchronising (or sizes with gs_visible_count first).
 * |V| == 0: GS_OK, count 0, nothing written.  max_rows == 0 is legal (count only; ids_out / grad_rows_out may be NULL, and
 * with both NULL the call is a count query: GS_OK).
 * Refusals: those of gs_backward (same messages, nothing enqueued), plus a NULL count_out, and NULL ids_out /
 * grad_rows_out with max_rows > 0.  Bitwise reproducible like gs_backward; the same for every sorter, launch shape, tile
 * order and GS_COUNT_* mode.  Scratch: that of gs_backward with its visible part (4 bytes per gaussian for the ids of V and
 * two block arrays of 4 bytes per 256 gaussians); gs_backward_visible also stages min(|V|, max_rows) rows on the device. */
int gs_visible_count(gs_ctx* ctx, uint32_t* count_out);
int gs_backward_visible(gs_ctx* ctx, const float* grad_rgba32f, const float* grad_depth,
                        uint32_t* ids_out, float* grad_rows_out, uint32_t max_rows, uint32_t* count_out);
int gs_backward_visible_device(gs_ctx* ctx, const float* grad_rgba32f, const float* grad_depth,
                               uint32_t* ids_out, float* grad_rows_out, uint32_t max_rows, uint32_t* count_out);

/* Camera gradients of a frame (no reference counterpart; callers detect the two calls by their symbols, GS_API_VERSION is
 * unchanged).  The call differentiates the last frame with the dL/d(outputs) the last gs_backward* call on this frame was
 * given: it re-reads the per-element rows that call left in the context's scratch, so it works after any gs_backward* form
 * that computed rows (dense or visible, host or device), and a visible call with max_rows < |V| still gives the full answer
 * (the blend backward writes every element's row whatever max_rows is).
 * Output: 35 floats.  [0..15] dL/dview, [16..31] dL/dproj, [32..34] dL/dcam_pos; element i of each block is the derivative
 * with respect to element i of the float[16] / float[3] argument of gs_render* (column-major, view[c * 4 + r]).  The
 * boundary convention is gs_backward's: every discrete decision of the frame is held fixed -- culls, tile boxes, keys and
 * order, the blended entries and the stop entry, det == 0, max(colour, 0) and the IN_VIEW_LIMIT clamp.
 * Two conventions:
 *   - The view matrix is taken as affine.  Elements 3, 7, 11 and 15 (its bottom row) receive exactly +0.0f: a camera
 *     never moves them.
 *   - dL/dproj covers the screen-position path only.  The covariance's focal lengths come from gs_config.fov_y, not from
 *     proj (the reference's own split, Common.glsl:53), and a frame never reads clip z: elements 2, 6, 10 and 14 of the
 *     proj block (18, 22, 26 and 30 of the 35 floats) are exactly +0.0f.
 * dL/dcam_pos is the SH direction's dependence on the camera position, over the coefficients the frame's sh_mode uses
 * (GS_SH_DEGREE_1 / _2: formed like mode 0's from the K active ones, no inactive plane read): exactly +0.0f in sh_mode 2 only.
 * Bitwise reproducible: no atomics, a fixed-shape sum over the splats -- the same 35 words for every sorter, launch shape,
 * tile order and GS_COUNT_* mode, after the dense and after the visible backward, from both entry points and from call to
 * call.  A frame that drew nothing gives GS_OK and 35 zeros.
 * Cost: a second pass over the rows (two launches); it is not fused into gs_backward*'s own row pass.  Scratch: 140 bytes
 * per 256 gaussians plus 35 floats, allocated on this call's first use and freed with the resolution.
 *   gs_backward_camera        : HOST pointer; synchronous.
 *   gs_backward_camera_device : DEVICE pointer; enqueued on the context's stream, no host sync.
 * GS_ERR_INVALID with a message in gs_last_error, nothing enqueued and nothing written: a NULL grad_camera, everything
 * gs_backward refuses (with its messages), and no gs_backward* form that computed rows on this frame ("no gs_backward* on
 * this frame": gs_visible_count, or a visible call with max_rows == 0, computes none). */
#define GS_CAMERA_GRAD_FLOATS 35u   /* [0..15] dL/dview, [16..31] dL/dproj, [32..34] dL/dcam_pos */
int gs_backward_camera(gs_ctx* ctx, float grad_camera[GS_CAMERA_GRAD_FLOATS]);
int gs_backward_camera_device(gs_ctx* ctx, float* grad_camera_dev);

/* Gradients of a band of tile rows (no reference counterpart; callers detect the call by its symbol, GS_API_VERSION is
 * unchanged).  The loss of a frame is a sum over its pixels, so dL/d(record) is a sum over its tile rows: a context that
 * owns a band (gs_set_tile_rows, any [row_begin, row_end) including the empty one, or gs_set_tile_rows_interleaved)
 * computes the terms of its own pixels, and the rows of the R bands of a frame, summed, are the frame's gradient.  What a
 * band context returns is therefore a PARTIAL SUM, not dL/d(record) -- which is why the calls refuse a band until the caller
 * says so:
 *   gs_set_band_gradients(ctx, 1) : gs_backward, gs_backward_device, gs_visible_count, gs_backward_visible,
 *                                   gs_backward_visible_device, gs_backward_camera, gs_backward_camera_device and
 *                                   gs_contrib_device accept a context that owns a subset of the tile rows;
 *   gs_set_band_gradients(ctx, 0) : (default) they refuse it with "the context owns a subset of the tile rows".
 * A host flag: nothing is enqueued or waited for; legal any time after gs_create; survives gs_set_resolution,
 * gs_set_tile_rows* and uploads.  GS_ERR_INVALID for a NULL ctx (the code alone) and for enable > 1 (with a message).  A
 * context that owns every row computes the same bits with the flag on as off.  Still refused with their messages, flag on
 * or off: a sharded context (gs_dist_shard_rows), a GS_RENDER_FAST context, a context without a frame since the last
 * change, and in a band gs_densify_stats_device (its sqrt(gx^2 + gy^2) and seen += 1 do not decompose over bands: a sum of
 * norms is not the norm of the sum) and gs_photometric_loss* (the 11 x 11 SSIM window crosses the band's edge).
 * The contract of a band:
 *   - Owned pixels: P = the pixels of the owned tile rows that lie in the image.
 *   - What is read: grad_rgba32f and grad_depth are addressed as for the whole frame, float[H][W][4] and float[H][W], real
 *     rows, top row first -- also under gs_set_tile_rows_interleaved(.., compact_output = 1).  Only the values at P are read.
 *   - Dense form: grad_records is the whole frame's gradient with dL/d(outputs) set to zero outside P, in the same
 *     arithmetic and the same order of sums: per splat, the rows of its list elements in the owned tiles are summed in slot
 *     order (tile raster order inside its tile box clipped to the owned rows), and the sum goes through the per-splat chain.
 *     A splat with no element in the band gets an all-zero record.
 *   - Visible form: V_band = the splats with at least one tile in the owned rows in this frame, ascending g.  ids, count
 *     and max_rows follow gs_backward_visible's rules, the rows are the dense band rows bit for bit, gs_visible_count
 *     returns |V_band|.  The union of V_band over the bands of a dealing is V of the whole frame.
 *   - Camera form: the 35 floats from the band's rows, by the same fixed-shape sum over g < N.
 *   - Contributions: gs_contrib_device takes the pairs (pixel of P, entry) alone.  The per-element sums are the whole
 *     frame's bit for bit, S runs over the band's slots in order, and a splat with no pair in the band is not touched.
 *     wmax and pixels accumulated over the bands of a dealing equal the whole frame's; wsum differs by the association of a
 *     float32 sum.
 *   - Overflow: a band whose own list overflowed is differentiated as drawn, by the same slot-below-capacity rule.
 *   - Reproducibility: bitwise, the same for every sorter, launch shape, tile order and GS_COUNT_* mode.
 *   - Scratch: as for the whole frame, sized by the band context's own capacity.
 * Moving the lists of the bands between GPUs is the caller's job; gs_rows_accumulate_device / gs_rows_collect_device sum
 * lists over different splat sets, and gs_adam_rows*_device / gs_upload_rows_device take the result unchanged. */
int gs_set_band_gradients(gs_ctx* ctx, uint32_t enable);

/* Anti-aliased frames (no reference counterpart: the reference adds 0.3 px^2 to the 2-D covariance, Common.glsl:72-75, and
 * blends the splat at its full opacity; this is the opacity compensation of the INRIA trainer's --antialiasing, gsplat's
 * rasterize_mode = "antialiased" and Mip-Splatting's 2-D filter.  Callers detect the call by its symbol, GS_API_VERSION is
 * unchanged).  With the flag on, the opacity RenderGaussians multiplies for a splat that emits an element and whose dilated
 * determinant is not zero is, in float32 and in this order,
 *     det0 = a0 * c0 - b0 * b0            a0, b0, c0: the 2-D covariance BEFORE its 0.3 dilation
 *     r    = det0 / det                   det: the determinant of the dilated covariance, as the frame has it
 *     rho  = sqrt(r > 2.5e-5 ? min(r, 1) : 2.5e-5)        (the INRIA floor; a NaN r takes the floor)
 *     raster opacity = opacity * rho
 * (r <= 1 for every covariance; the cap acts only where both determinants of a needle are float32 cancellation noise below
 * zero and their ratio comes out above 1, so that no splat is ever blended above its own opacity)
 * so a splat much smaller than a pixel, which the dilation blows up to about a pixel, is dimmed by the ratio of the areas
 * instead of being drawn as opaque as before.  Nothing else of a frame changes: covariance (GS_BUF_COV), conic, radius, tile
 * box, depth key, colour and the det == 0 rule (opacity 0) are the plain frame's, hence so are the sorted list and the
 * ranges; GS_BUF_COLOR's alpha stays the scene's opacity; GS_BUF_RASTER_OPACITY shows the compensated value.  Both render
 * modes, every sorter and every launch shape are covered (they read the raster record).
 * Equivalence: a frame of records R with the flag on equals, in every output, the frame with the flag off of R' = R with
 * float 15 (the opacity) of every record replaced by its GS_BUF_RASTER_OPACITY.
 * Gradients (gs_backward*, gs_backward_camera*, bands included) are those of the frame as it was drawn: the record's opacity
 * receives dL/d(raster opacity) * rho, and above the floor dL/d(raster opacity) * opacity flows through r into the
 * covariance, i.e. into scale, rotation, position and the view block; dL/dproj and dL/dcam_pos do not depend on rho.  At the
 * floor rho is a constant (see the boundary convention of gs_backward).  gs_contrib_device replays with the raster opacity.
 * gs_relocate_device / gs_grow_device correct the opacity and scale of copies so that the plain frame's picture stays; with
 * the flag on that correction is only approximate (the copies' rho differs from the source's).
 * A host flag per CONTEXT, not per scene (two contexts that share a scene may differ), 0 by default, legal any time after
 * gs_create; it survives gs_set_resolution, gs_set_tile_rows*, gs_set_outputs and uploads; nothing is enqueued or waited
 * for.  It does not invalidate the last frame: gs_backward*, gs_backward_camera* and gs_contrib_device work on the frame as
 * it was drawn, whatever the flag says by then; the next frame uses the new value.  With the flag off every frame, list and
 * gradient is bit for bit what it is without this call.  GS_ERR_INVALID for a NULL ctx (the code alone) and for enable > 1
 * (with a message; the flag stays as it was). */
int gs_set_antialias(gs_ctx* ctx, uint32_t enable);

/* One optimiser step on the rows gs_backward_visible* lists (no reference counterpart), in two calls that keep no state
 * inside the library: an Adam step on the CALLER's records and moments, and the upload of the changed rows alone.
 *
 * Field groups: the 59 floats of the 84-float record that gs_backward gives gradients to.  The other 25 (3, 7, 19 + 4k for
 * k = 0..14, and 76..83) are never read or written by either call, in records, m or v. */
#define GS_ADAM_POSITION 0   /* floats 0, 1, 2 */
#define GS_ADAM_SCALE 1      /* floats 4, 5, 6 */
#define GS_ADAM_ROTATION 2   /* floats 8..11 */
#define GS_ADAM_SH_DC 3      /* floats 12, 13, 14 */
#define GS_ADAM_OPACITY 4    /* float 15 */
#define GS_ADAM_SH_REST 5    /* floats 16 + 4k + {0, 1, 2}, k = 0..14 */
#define GS_ADAM_GROUPS 6

typedef struct gs_adam_params {
    uint32_t struct_size;          /* sizeof(gs_adam_params) of the caller's header: filled by gs_default_adam_params, checked */
    uint32_t step;                 /* t >= 1 of THIS step (the caller counts) */
    float beta1, beta2, eps;
    float lr[GS_ADAM_GROUPS];      /* per group: learning rate ... */
    float lo[GS_ADAM_GROUPS];      /* ... and the clamp [lo, hi] of the updated value (infinite = none) */
    float hi[GS_ADAM_GROUPS];
} gs_adam_params;
/* step 1, beta1 0.9, beta2 0.999, eps 1e-15; lr: position 1.6e-4, scale 5e-3, rotation 1e-3, SH DC 2.5e-3, opacity 5e-2,
 * SH rest 1.25e-4 -- the rates of the INRIA 3DGS trainer.  NOTE: there they act on log-scales and logit-opacities; with
 * gs_adam_rows_device they act on the record's own values (scale and opacity as the frame reads them), so the clamps below
 * stand in for what exp and sigmoid guarantee, and a caller may want other rates.  The rates fit the raw space:
 * gs_default_adam_params_raw and gs_adam_rows_raw_device, below.  lo / hi: scale [1e-7, +inf], opacity [0, 1], every other
 * group [-inf, +inf]. */
void gs_default_adam_params(gs_adam_params* p);
/* torch.optim.SparseAdam's rule on rows ids[i], i < min(*count_dev, max_rows), of records / m / v (each float[n][84],
 * DEVICE, the caller's; m and v start as zeros) with the gradient rows grad_rows[i][84] -- ids, grad_rows and count_dev
 * as gs_backward_visible_device leaves them.  Every field of a listed row moves, also one with a zero gradient, and eps
 * is added before the bias correction.  All arithmetic is float32, never contracted, in exactly this order, so the
 * result is bitwise reproducible (and restated exactly by NumPy float32: tests/test_adam_cpu.py):
 *   host, per group: step_g = (float)(((double)lr_g * sqrt(1 - pow((double)beta2, t))) / (1 - pow((double)beta1, t)));
 *   host: c1 = 1.0f - beta1, c2 = 1.0f - beta2;
 *   m' = beta1 * m + c1 * g
 *   v' = beta2 * v + (c2 * g) * g
 *   p' = p - step_g * (m' / (sqrtf(v') + eps))
 *   p' = p' < lo_g ? lo_g : (p' > hi_g ? hi_g : p')        (a NaN stays a NaN)
 * An ids[i] >= n is skipped (compared, never dereferenced).  Ids are distinct, as gs_backward_visible* writes them;
 * duplicates are the caller's error.  ids, grad_rows and count_dev are only read; count_dev is never read by the host.
 * Enqueued on the context's stream, no host sync; the grid is sized from max_rows and the blocks past the count exit at
 * once.  max_rows == 0: GS_OK, nothing launched.  The call needs no scene and no resolution: it uses the context's device
 * and stream only.
 * GS_ERR_INVALID with a message in gs_last_error, nothing enqueued (a NULL ctx: the code alone): a NULL pointer with
 * max_rows > 0, n == 0, a struct_size other than sizeof(gs_adam_params), step == 0, a beta outside [0, 1), an lr or eps
 * that is negative or not finite (or an lr whose step_g is not finite), lo_g > hi_g or a NaN bound. */
int gs_adam_rows_device(gs_ctx* ctx, float* records_dev, float* m_dev, float* v_dev, uint32_t n,
                        const uint32_t* ids_dev, const float* grad_rows_dev, const uint32_t* count_dev,
                        uint32_t max_rows, const gs_adam_params* p);
/* The sparse form of the in-place gs_upload_gaussians_device: for every listed g = ids[i], i < min(*count_dev, max_rows),
 * the planes of splat g (position, scale, rotation, the 48 SH values, opacity and the cull bound derived from scale and
 * rotation) are rewritten from record g of aos336_dev (float[n][84], DEVICE), then the per-64-splat boxes are rebuilt:
 * afterwards the scene is bit for bit what gs_upload_gaussians_device makes of records that differ from the uploaded
 * ones in the listed rows only.  An ids[i] >= n is skipped; ids are distinct.  Enqueued on the context's stream, no host
 * sync; every context sharing the scene (gs_share_scene) renders the new values; resolution, scratch and captured graphs
 * stay; gs_backward* needs a new frame, as after the full upload.  max_rows == 0: GS_OK, nothing launched.
 * GS_ERR_INVALID (message, nothing enqueued; a NULL ctx: the code alone): a NULL pointer with max_rows > 0, n == 0, an n
 * that differs from the scene's (this call never makes a new scene).  GS_ERR_NO_SCENE: no gaussians uploaded yet. */
int gs_upload_rows_device(gs_ctx* ctx, const void* aos336_dev, uint32_t n,
                          const uint32_t* ids_dev, const uint32_t* count_dev, uint32_t max_rows);

/* The raw parameter space (no reference counterpart): what a .ply stores and the INRIA trainer optimises, next to the
 * record space the frame reads.  A raw array is float[n][84] in the record's own layout: the same 59 floats are fields, the
 * same 25 are never read or written by any call below.  It differs from a record in three places: floats 4..6 are
 * log-scales, float 15 is the logit of the opacity, floats 8..11 are the rotation before normalisation (the record's
 * component order).  act(raw) is the record it stands for -- float32, never contracted, in exactly this order:
 *   s_k = E(raw[4 + k])                                                                    k = 0, 1, 2
 *   o   = 1.0f / (1.0f + E(-raw[15]))
 *   t_i = raw[8 + i] * raw[8 + i];  inv = 1.0f / sqrtf((t0 + t1) + (t2 + t3));  q_i = raw[8 + i] * inv
 *   every other field: the same bits
 * E is the pinned exp of the frame's blend (exp2(x log2 e) with both clamps, t in [-126, 126], and a degree-6 polynomial;
 * within 1e-6 relative of exp on [-20, 6], and the sigmoid built from it within 1e-6 relative on [-20, 20]).  E(-inf) =
 * 2^-126 and E(+inf) = 2^126, the clamps; a NaN goes to the lower clamp, 2^-126, and is NOT propagated.  The rotation is
 * the loader's expression (glm::normalize), association included: a raw rotation written to a .ply by gs_write_ply and
 * loaded again gives the record's rotation bit for bit.  A zero rotation gives NaN, as it does in the loader.  act is
 * restated exactly by NumPy float32 with that exp (tests/test_raw_cpu.py).
 *
 * All four device calls work on the CALLER's device arrays, are enqueued on the context's stream without a host sync, need
 * no scene and no resolution, keep no state in the library and are bitwise reproducible (gs_raw_from_records_device: up to
 * the device's logf).  Callers detect them, and gs_write_ply, by their symbols (GS_API_VERSION is unchanged).
 *
 * gs_default_adam_params_raw: gs_default_adam_params with every lo = -inf and every hi = +inf -- in raw space the INRIA
 * rates are the right ones and nothing needs a clamp.
 *
 * gs_adam_rows_raw_device: gs_adam_rows_device in raw space, in one kernel.  The listing rules are the same: rows
 * i < min(*count_dev, max_rows), an ids[i] >= n compared and never dereferenced, distinct ids, the grid sized from
 * max_rows, count_dev never read by the host, max_rows == 0: GS_OK and nothing launched.  grad_rows[i] is dL/d(record
 * ids[i]) as gs_backward_visible_device leaves it: with respect to the record's own floats, the rotation as getRotMat
 * reads it.  Per listed row, with g = the gradient row and the record's CURRENT values (what the frame rasterised):
 *   position, SH:  gt = g
 *   scale k:       gt = g[4 + k] * records[4 + k]
 *   opacity:       gt = (g[15] * o) * (1.0f - o)                                           o = records[15]
 *   rotation:      inv = 1.0f / sqrtf((t0 + t1) + (t2 + t3)) of the OLD raw[8..11];        q = records[8..11]
 *                  d = (g8 * q0 + g9 * q1) + (g10 * q2 + g11 * q3);   gt_i = (g[8 + i] - q_i * d) * inv
 * then the rule of gs_adam_rows_device, exactly as it stands, on (raw, m, v, gt) -- the group's step, lo and hi apply to
 * the RAW value --, then records[fields] = act(raw'), the identity fields receiving the bits of raw'.  The chain stands on
 * records == act(raw) in the listed rows, which every call of this block keeps.  Only the 59 fields of listed rows are
 * touched, in raw, m, v and records; ids, grad_rows and count_dev are only read.
 * GS_ERR_INVALID: everything gs_adam_rows_device refuses, with its words behind this call's name, a NULL raw, and a records
 * that shares bytes with raw, m or v.
 *
 * gs_records_from_raw_device: records[fields] = act(raw) for every row g < n.
 * gs_raw_from_records_device: the inverse, with the device's logf (1 ulp), otherwise float32 in this order:
 *   raw_s = logf(s < FLT_MIN ? FLT_MIN : s)
 *   c = o < 0x1p-24f ? 0x1p-24f : (o > 0x1.fffffep-1f ? 0x1.fffffep-1f : o);   raw_o = logf(c / (1.0f - c))
 *   rotation and every other field: the same bits
 * The two clamps keep a record opacity of exactly 0 or 1 trainable: |logit| <= 16.7.  act of the result is the record
 * again up to the rounding of one log and one exp.  Both refuse (GS_ERR_INVALID) a NULL array, n == 0 and arrays that
 * share bytes.
 *
 * gs_reset_opacity_raw_device: the INRIA opacity reset.  For every g < n with records[g][15] > max_opacity:
 * raw[g][15] = L, L = (float)log((double)max_opacity / (1.0 - (double)max_opacity)) computed on the host, and
 * records[g][15] = 1.0f / (1.0f + E(-L)); for every g, reset or not, m[g][15] = v[g][15] = 0.  m and v may be NULL together.
 * No other float is touched.  The caller follows it with a full upload (gs_upload_gaussians_device).  GS_ERR_INVALID: a
 * NULL raw or records, one of m and v without the other, n == 0, a max_opacity that fails 0 < max_opacity < 1. */
void gs_default_adam_params_raw(gs_adam_params* p);
int gs_adam_rows_raw_device(gs_ctx* ctx, float* raw_dev, float* records_dev, float* m_dev, float* v_dev, uint32_t n,
                            const uint32_t* ids_dev, const float* grad_rows_dev, const uint32_t* count_dev,
                            uint32_t max_rows, const gs_adam_params* p);
int gs_records_from_raw_device(gs_ctx* ctx, const float* raw_dev, float* records_dev, uint32_t n);
int gs_raw_from_records_device(gs_ctx* ctx, const float* records_dev, float* raw_dev, uint32_t n);
int gs_reset_opacity_raw_device(gs_ctx* ctx, float* raw_dev, float* records_dev, float* m_dev, float* v_dev, uint32_t n,
                                float max_opacity);

/* Adaptive density control (no reference counterpart): the statistics of a training step, and the new cloud -- clone where
 * the screen gradient is large and the splat small, split where it is large, prune what is transparent or huge.  All arrays
 * are the CALLER's, on the DEVICE; the library keeps no training state.  Callers detect both calls by their symbols
 * (GS_API_VERSION is unchanged).
 *
 * gs_densify_stats_device: ids_dev / count_dev as gs_backward_visible_device left them for the CURRENT frame; for every
 * i < min(*count_dev, max_rows), g = ids_dev[i] (an id >= n is skipped: compared, never dereferenced):
 *   (dsx, dsy) = the splat's dL/d(screen position): its rows of the backward's scratch summed in slot order, clamped at the
 *                list capacity -- the very bits the record gradient was chained from;
 *   gx = dsx * 0.5f * W, gy = dsy * 0.5f * H        (NDC units: the INRIA threshold 2e-4 applies)
 *   grad_accum[g] = grad_accum[g] + sqrtf(gx * gx + gy * gy)      (float32, not contracted)
 *   seen[g]      += 1
 *   radius        = ceilf(3 * sqrtf(max(lambda0, lambda1))) of the frame's 2-D covariance, the expressions of the tile extents
 *   max_radius[g] = radius > max_radius[g] ? radius : max_radius[g]
 * grad_accum, seen, max_radius: float / uint32 / float [n].  Ids are distinct, so there are no atomics and the result is
 * bitwise reproducible, the same for every sorter.  Enqueued on the context's stream, no host sync; count_dev is never read
 * by the host, the grid is sized from max_rows.  max_rows == 0: GS_OK, nothing launched.
 * GS_ERR_INVALID (message in gs_last_error, nothing enqueued): everything gs_backward refuses, with its messages; no
 * gs_backward* form that computed gradient rows has run on this frame ("no gs_backward* on this frame": gs_visible_count
 * alone, a new frame, an upload, a new resolution or tile rows all leave none); a NULL pointer with max_rows > 0; an n other
 * than the scene's. */
int gs_densify_stats_device(gs_ctx* ctx, const uint32_t* ids_dev, const uint32_t* count_dev, uint32_t max_rows,
                            uint32_t n, float* grad_accum, uint32_t* seen, float* max_radius);

typedef struct gs_densify_params {
    uint32_t struct_size;   /* sizeof(gs_densify_params) of the caller's header: filled by gs_default_densify_params, checked */
    float grad_threshold;   /* 2e-4 */
    float split_scale;      /* max scale above which a growing splat is split, not cloned (the caller's percent_dense * extent); 0.01 */
    float prune_opacity;    /* 0.005 */
    float prune_scale;      /* +inf = none (INRIA: 0.1 * extent) */
    float prune_radius;     /* pixels; +inf = none */
    float split_shrink;     /* 1.6 = 0.8 * 2 */
    uint64_t seed;          /* 0 */
} gs_densify_params;
void gs_default_densify_params(gs_densify_params* p);
/* The new cloud from records / m / v (float[n][84]) and the statistics (float / uint32 / float [n]).  Per input splat g, in
 * float32, every comparison exactly as written (a NaN compares false), max(a, b) = a > b ? a : b:
 *   smax   = max(max(s0, s1), s2) over floats 4..6; op = float 15
 *   pruned = op < prune_opacity || smax > prune_scale || max_radius[g] > prune_radius
 *   mean   = seen[g] ? grad_accum[g] / (float)seen[g] : 0
 *   grow   = !pruned && mean >= grad_threshold;  split = grow && smax > split_scale;  clone = grow && !split
 * g has k(g) outputs -- 0 pruned, 2 growing, else 1 -- at rows [o(g), o(g) + k(g)) of records_out / m_out / v_out, o = the
 * exclusive scan of k: the output is stable, and children sit next to their parent (the storage order keeps its locality).
 *   kept  : record, m and v rows copied bit for bit.
 *   clone : output 0 as kept; output 1 the same record with zero m and v rows.
 *   split : two children with zero m and v rows; all 84 floats of the parent except
 *           scale_child[k] = s[k] / split_shrink                                           (floats 4..6)
 *           pos_child[i]   = pos[i] + off[i]                                               (floats 0..2)
 *           off[i] = ((R[i][0] * s[0]) * z[0] + (R[i][1] * s[1]) * z[1]) + (R[i][2] * s[2]) * z[2]
 *           with R = the rotation matrix of the record's own (unnormalised) rot as the frame builds it, R[row][col], i.e. a
 *           draw from the gaussian the frame rasterises, Sigma = M M^T, M = R diag(s).
 * The normals z[axis] of child c are counter-based -- a function of (seed, g, c, axis) alone, uint32 arithmetic:
 *   mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *   h = mix(mix(g ^ (uint32)seed) + (uint32)(seed >> 32));   w(c, a, j) = mix(h + (c * 6 + a * 2 + j + 1) * 0x9E3779B9)
 *   u1 = ((w(c, a, 0) >> 8) + 1) * 2^-24  in (0, 1];   u2 = (w(c, a, 1) >> 8) * 2^-24
 *   z = sqrtf(-2 * logf(u1)) * cosf(6.2831855f * u2)        (the device's logf and cosf: |z| <= 5.77)
 * counts_out[4] (DEVICE): [0] the number of outputs, not truncated; [1], [2], [3] the cloned, split and pruned input splats.
 * Rows with index >= max_out are not written and nothing past the written rows is touched; max_out >= 2 n always fits.
 * m, v, m_out and v_out may be NULL all together, and only all together (records alone).  Bitwise reproducible; enqueued on
 * the context's stream, no host sync; needs no scene and no resolution.  Scratch: 4 bytes per splat + 20 bytes per 256
 * splats, the context's, grown on demand and freed by gs_destroy.
 * GS_ERR_INVALID (message, nothing enqueued): a NULL required pointer (records_out only with max_out > 0), n == 0 or
 * n >= 2^31, a wrong struct_size, a NaN grad_threshold, split_shrink that fails split_shrink > 0, an output array that shares
 * bytes with an input or another output, a partly NULL moment quadruple. */
int gs_densify_device(gs_ctx* ctx, const float* records, const float* m, const float* v, uint32_t n,
                      const float* grad_accum, const uint32_t* seen, const float* max_radius,
                      const gs_densify_params* p,
                      float* records_out, float* m_out, float* v_out, uint32_t max_out, uint32_t* counts_out);

/* Absolute screen gradients (no reference counterpart; the growth statistic of AbsGS, gsplat's absgrad = True.  Callers
 * detect the three calls by their symbols, GS_API_VERSION is unchanged).  The screen gradient dL/d(sx, sy) of a splat is the
 * sum of one term per pixel that blends it.  Over a large, blurry splat on fine texture the terms pull in opposite directions
 * and cancel, so the norm gs_densify_stats_device accumulates stays below the threshold exactly where a split is needed.  The
 * statistic here is the sum of the ABSOLUTE values of the same terms, per component:
 *     abs_x(g) = sum over (pixel p, list element of g that p blends) of |dL_p/dsx|,    abs_y(g) likewise with dsy
 * where dL_p/dsx is the float32 term the backward adds into dsx for that pair -- not a recomputation.
 *
 * gs_set_abs_gradients(ctx, 1): every gs_backward* form (gs_backward, gs_backward_device, gs_backward_visible,
 * gs_backward_visible_device; on a band context too) also leaves the absolute pairs in the context's scratch, one pair per
 * list element in its slot.  Per element the 256 pixels of its tile are summed in the fixed order of the signed columns
 * (per wave a balanced tree over the lanes, then ((W0 + W1) + W2) + W3; a pixel that does not blend the entry adds +0.0f);
 * an element no pixel of its tile reaches gets (0, 0), never what an earlier frame left; an element at or past the list
 * capacity has no slot and no pair.  Everything those calls return is bit for bit what it is with the switch off, and so is
 * whatever gs_backward_camera* and gs_densify_stats_device read afterwards.  Frames are not affected.  Scratch: 8 bytes per
 * list element of capacity, allocated by the first gs_backward* form that runs with the switch on, freed with the resolution.
 * A host flag per context, 0 by default, legal any time after gs_create; it survives gs_set_resolution, gs_set_tile_rows* and
 * uploads; nothing is enqueued or waited for.  With the switch off gs_backward* runs the kernel it ran before this call existed.
 * GS_ERR_INVALID for a NULL ctx (the code alone) and for enable > 1 (with a message; the flag stays as it was).
 *
 * gs_abs_screen_gradient_device: for i < min(*count_dev, max_rows), g = ids_dev[i]:
 *     abs_out[i] = (abs_x(g), abs_y(g)), in pixel units like dsx, dsy: per component S = 0.0f; S = S + pair over the
 *     splat's list elements in slot order (tile raster order inside its box), over the slots below the list capacity;
 *     (0, 0) for a splat with no element in this frame and for an id >= n of the scene (compared, never dereferenced).
 * Rows at or past the count are not touched.  abs_out: float[max_rows][2], DEVICE.  abs_x(g) >= |dsx(g)| and abs_y(g) >=
 * |dsy(g)| as float32 (the same terms in the same tree; rounding is monotone).  Served on a band context while
 * gs_set_band_gradients is on: the band's pairs are the partial sums over its own pixels, and -- unlike the norm -- they add
 * up over the bands of a frame (up to the association of a float32 sum of non-negative numbers).
 *
 * gs_densify_stats_abs_device: gs_densify_stats_device's grad_accum on the absolute pair.  Per listed g < n (an id >= n is
 * skipped), in float32, not contracted:
 *     ax = abs_x(g) * 0.5f * W,  ay = abs_y(g) * 0.5f * H
 *     grad_accum_abs[g] = grad_accum_abs[g] + sqrtf(ax * ax + ay * ay)
 * and nothing else: seen and max_radius stay with gs_densify_stats_device, which is called beside it on the same ids.
 * grad_accum_abs: float[n].  Like that call it is refused on a band.  A caller applies the AbsGS rule with gs_densify_device
 * as it stands by handing it, per splat, grad_accum_abs * (grad_threshold / abs_threshold) where the largest scale exceeds
 * split_scale and grad_accum elsewhere: large splats split by the absolute mean against abs_threshold, small ones clone by
 * the signed mean against grad_threshold.  AbsGS and gsplat's documentation publish abs_threshold = 8e-4; this library has
 * not measured a value.
 *
 * Both read calls: enqueued on the context's stream, no host sync; count_dev is never read by the host, the grid is sized
 * from max_rows; ids are distinct (for the accumulating call), there are no atomics and the result is bitwise reproducible,
 * the same for every sorter.  max_rows == 0: GS_OK, nothing launched.
 * GS_ERR_INVALID (message in gs_last_error, nothing enqueued; a NULL ctx: the code alone): a NULL pointer with max_rows > 0;
 * everything gs_densify_stats_device refuses, with its messages (for gs_abs_screen_gradient_device a band is refused only
 * while gs_set_band_gradients is off, and there is no n to compare); and "no gs_backward* on this frame with
 * gs_set_abs_gradients on": the last blend of a gs_backward* form on this frame did not run with the switch on.  Turning the
 * switch on after the backward does not count; a new frame, an upload, a new resolution or tile rows clear the state. */
int gs_set_abs_gradients(gs_ctx* ctx, uint32_t enable);
int gs_abs_screen_gradient_device(gs_ctx* ctx, const uint32_t* ids_dev, const uint32_t* count_dev, uint32_t max_rows,
                                  float* abs_out);
int gs_densify_stats_abs_device(gs_ctx* ctx, const uint32_t* ids_dev, const uint32_t* count_dev, uint32_t max_rows,
                                uint32_t n, float* grad_accum_abs);

/* Pruning by contribution (no reference counterpart): which splats does any picture ever show?  The blend weight
 * w = T * alpha is known to the blend alone; a splat behind an opaque surface in every view passes the opacity, scale and
 * radius tests of gs_densify_device and is still projected, sorted and walked in every frame.  Two calls: the per-splat blend
 * statistics of a frame, accumulated over any number of frames, and a stable compaction of the cloud by a per-splat score.
 * All arrays are the CALLER's, on the DEVICE; the library keeps no training state.  Callers detect both calls by their symbols
 * (GS_API_VERSION is unchanged).
 *
 * gs_contrib_device works on the last frame enqueued on the context.  Take every pair (pixel p, entry i of the list of p's
 * tile) in which the entry adds its colour to the pixel -- the entry a pixel stops on included, the entries behind it not
 * (tests/host/blend_trace_ref.c flags exactly these 1 or 2).  w = T_i * alpha_i, the float32 product of the forward's own
 * transmittance in front of the entry and its own alpha (same expressions, same pinned exp).  Per splat g with at least one
 * such pair in the frame (wmax, wsum: float[n], pixels: uint32[n], n the scene's):
 *   wmax[g]   = M > wmax[g] ? M : wmax[g]                M = the largest w of g in the frame
 *   wsum[g]   = wsum[g] + S                              S = the frame's sum in the fixed order below
 *   pixels[g] = min(pixels[g] + count, 2^32 - 1)         count = the number of pairs; the sum is formed in 64 bits
 * A splat without such a pair is neither read nor written in any of the three arrays: culled splats, splats that emit no
 * element, splats wholly past an overflowed list, entries with det == 0, entries no pixel reaches and entries behind every
 * pixel's stop.  The arrays start as zeros and accumulate over any number of frames.  wsum_dev and pixels_dev may each be
 * NULL: that statistic is not formed.
 * The fixed order of S (no float atomics; restated bit for bit by tests/host/contrib_ref.c):
 *   per list element  e = ((W0 + W1) + W2) + W3, Ww = the sum over the 64 pixels of wave w of the element's tile: pixel rows
 *                     4 w .. 4 w + 3 of the tile, lane = (ly & 3) * 16 + lx, as a balanced tree -- lanes 2 k and 2 k + 1
 *                     first, then adjacent pair sums, six levels; a pixel that does not blend the entry, or lies outside
 *                     the image, adds +0.0f;
 *   per splat         S = 0.0f; S = S + e over the splat's list elements in slot order = tile raster order inside its box
 *                     (the order of the backward's row sums), over the slots below the list capacity.
 * Weights are finite and positive whenever opacities are finite; with non-finite opacities the call still terminates and
 * the affected splats' values are unspecified.  Enqueued on the context's stream, no host sync; bitwise reproducible, the
 * same for every sorter, launch shape, tile order and GS_COUNT_* mode.  Scratch: the per-splat slot offsets -- the
 * backward's own where a gs_backward* form has allocated them (the values are identical), else 4 bytes per splat of this
 * call's -- plus 12 bytes per list element of capacity, allocated on first use and freed with the resolution; never the
 * backward's 40-byte rows.  The call leaves what a backward left behind as it is: between gs_backward_visible_device and
 * gs_backward_camera_device or gs_densify_stats_device it changes neither result by a bit.
 * GS_ERR_INVALID (message in gs_last_error, nothing enqueued; a NULL ctx: the code alone): everything gs_backward refuses,
 * with its words behind this call's name (no frame since the last gs_set_resolution / gs_set_tile_rows* / upload /
 * gs_debug_init_sort_list, a GS_RENDER_FAST context, a context that owns a subset of the tile rows unless
 * gs_set_band_gradients is on, a sharded context); a NULL wmax_dev; an n other than the scene's. */
int gs_contrib_device(gs_ctx* ctx, uint32_t n, float* wmax_dev, float* wsum_dev, uint32_t* pixels_dev);
/* gs_prune_below_device: keep(g) = score[g] >= threshold, exactly as written (a NaN score is dropped).  The kept rows of
 * records / raw / m / v (float[n][84], all 84 floats) are copied bit for bit to rows [0, kept) of their outputs, in ascending
 * g.  counts_out[2] (DEVICE): [0] the number kept, not truncated; [1] the number dropped.  Rows with index >= max_out are not
 * written and nothing past the written rows is touched.  raw, m and v are optional one by one, each NULL together with its
 * own output; records_out (and the outputs of the arrays given) may be NULL with max_out == 0, a count query.  Bitwise
 * reproducible; enqueued on the context's stream, no host sync; needs no scene and no resolution.  Scratch: the context's
 * per-splat scan buffers, shared with gs_densify_device.
 * GS_ERR_INVALID (message, nothing enqueued; a NULL ctx: the code alone): a NULL score, records or counts_out, a NULL
 * records_out with max_out > 0, n == 0 or n >= 2^31, a NaN threshold, an input NULL without its output or the reverse, an
 * output that shares bytes with an input, with the score or with another output. */
int gs_prune_below_device(gs_ctx* ctx, const float* score_dev, float threshold, uint32_t n,
                          const float* records, const float* raw, const float* m, const float* v,
                          float* records_out, float* raw_out, float* m_out, float* v_out,
                          uint32_t max_out, uint32_t* counts_out_dev /* [2] */);

/* MCMC (no reference counterpart): the other strategy for the set of gaussians, 3DGS-MCMC (Kheradmand et al. 2024).  Dead
 * splats are relocated onto live ones sampled in proportion to their opacity, the cloud grows by a chosen number of rows up to
 * a chosen cap, and noise shaped like each splat's covariance explores the positions.  Relocation keeps n: it runs in place
 * and lists the rows it changed for gs_upload_rows_device, so the scene, the resolution and the scratch stay.  All arrays are
 * the CALLER's, on the DEVICE; every call is enqueued on the context's stream with no host sync, needs no scene and no
 * resolution, keeps no state in the library and is bitwise reproducible, the same for every sorter (up to the device's
 * log1pf / expm1f / logf / cosf).  Callers detect the calls by their symbols (GS_API_VERSION is unchanged).  Scratch: 12 bytes
 * per splat + 16 bytes per 256 splats + 11 KB, beside the per-splat scan buffers shared with gs_densify_device; the
 * context's, grown on demand and freed by gs_destroy.
 *
 * The sampler (gs_relocate_device and gs_grow_device), integer arithmetic throughout:
 *   alive(g) = records[g][15] > min_opacity, exactly as written (a NaN opacity is dead)
 *   w(g)     = alive(g) ? (uint32)(min(o, 1.0f) * 16777216.0f) : 0        (the conversion truncates)
 *   P(g)     = the exclusive prefix sum of w in 64 bits; total = the sum
 *   draw i:    h = mix(mix(i ^ (uint32)seed) + (uint32)(seed >> 32))      (mix: gs_densify_device's)
 *              r64 = ((uint64)mix(h + 0x9E3779B9) << 32) | mix(h + 2 * 0x9E3779B9)
 *              t = (uint64)(((unsigned __int128)r64 * total) >> 64), in [0, total)
 *              the source is the one g with P(g) <= t < P(g) + w(g): never a splat of weight zero
 *   cnt[g]   = the number of draws whose source is g; with total == 0 no draw is made.
 *
 * The relocation values of a source g with cnt[g] > 0: r = min(cnt[g] + 1, 51), o and s_k the record's current opacity and
 * scales, hi = 0x1.fffffep-1f; float32, never contracted, in exactly this order:
 *   o1 = -expm1f(log1pf(-min(o, hi)) / (float)r)          (the device's functions: 1 - (1 - o)^(1 / r), well conditioned)
 *   oc = o1 < min_opacity ? min_opacity : (o1 > hi ? hi : o1)
 *   records alone: o' = oc.  With raw: raw[15] = logf(oc / (1.0f - oc)) and o' = 1.0f / (1.0f + E(-raw[15])) (act).
 *   D = 0;  for i = 1 .. r: { p = o'; sg = 1;  for k = 0 .. i - 1: { D = D + B[i - 1][k] * ((sg * Q[k]) * p);  p = p * o';
 *   sg = -sg } }          B[a][b] = (float)C(a, b) from the exact integer, Q[k] = (float)(1.0 / sqrt((double)(k + 1)))
 *   c = o / D;  s'_k = c * s_k.  Records alone: the record stores s'_k.  With raw: raw[4 + k] = logf(max(s'_k, FLT_MIN)) and
 *   the record stores E(raw[4 + k]).  The record stores o'.
 * For o' in [0.005, hi] and every r, D > 0 and 0 < c <= 1 (tests/test_mcmc_cpu.py).  Two deliberate differences from the CUDA
 * original keep the stored pair consistent: the clamp comes BEFORE the scale -- the scale belongs to the opacity that is
 * stored --, and the opacity is not computed with powf.
 *
 * gs_relocate_device, in place, n fixed.  Every dead d makes draw i = d; call its source src(d).  Then, in this order:
 *   1. every source gets the new opacity and scales, in records and (if given) raw; its m and v rows become zero;
 *   2. every dead d gets all 84 floats of records[src(d)], and of raw[src(d)], as they now stand; its m and v rows become
 *      zero.
 * No other float is touched.  ids_out receives, ascending, the changed rows -- the dead splats and the sources --, at most
 * max_rows of them; counts_out[3] (DEVICE) = {changed (not clamped), dead, sources}: ids_out and counts_out are what
 * gs_upload_rows_device takes.  With total == 0 or no dead splat the counts are {0, dead, 0} and nothing changes.
 * max_rows == 0 with a NULL ids_out is legal (the caller uploads in full).  raw may be NULL; m and v NULL together.
 * GS_ERR_INVALID (message in gs_last_error, nothing enqueued; a NULL ctx: the code alone): a NULL records or counts_out, one of
 * m and v without the other, n == 0 or n >= 2^31, a min_opacity that fails 0x1p-24f <= min_opacity < 1, a NULL ids_out with
 * max_rows > 0, arrays that share bytes.
 *
 * gs_grow_device, out of place like gs_densify_device.  Draws i = 0 .. n_add - 1 give cnt.  Input g has 1 + cnt[g] outputs at
 * rows [o(g), o(g) + 1 + cnt[g]), o = the exclusive scan: the copies sit beside their source, and the storage order keeps its
 * locality.  A g with cnt[g] == 0: its rows of records, raw, m and v copied bit for bit.  A g with cnt[g] > 0: all its
 * outputs identical, the source's row with the relocation values for r = min(cnt[g] + 1, 51), and zero m and v rows.
 * counts_out[2] (DEVICE) = {outputs, sources}; outputs = n + n_add when total > 0, else n.  Rows with index >= max_out are not
 * written.  raw, m and v are each NULL together with their own output; n_add == 0 is a plain copy.
 * GS_ERR_INVALID: what gs_relocate_device refuses of records, counts_out, m, v, n and min_opacity; n + n_add >= 2^31; a NULL
 * records_out with max_out > 0; an input NULL without its output or the reverse; an output that shares bytes with an input or
 * with another output.
 *
 * gs_position_noise_device.  With ids the listing rules of gs_adam_rows_device: rows i < min(*count_dev, max_rows), an id >= n
 * compared and never dereferenced, the grid sized from max_rows, count_dev never read by the host; with a NULL ids every g < n
 * (count_dev and max_rows are ignored).  For a listed g, float32, never contracted:
 *   z_a  = gs_densify_device's normal of (seed, g, child 0, axis a);  R = the rotation matrix of the record's own rot as the
 *          frame builds it, R[row][col];  s = the record's scales, o = its opacity
 *   gate = 1.0f / (1.0f + E(-(gate_k * ((1.0f - o) - gate_x0))))                  (3DGS-MCMC: gate_k = 100, gate_x0 = 0.995)
 *   a_k   = s_k * ((R[0][k] * z_0 + R[1][k] * z_1) + R[2][k] * z_2)
 *   off_i = ((R[i][0] * s_0) * a_0 + (R[i][1] * s_1) * a_1) + (R[i][2] * s_2) * a_2          (Sigma z, Sigma = M M^T)
 *   pos_i = pos_i + (off_i * gate) * scale
 * written to records and, the same bits, to raw (may be NULL).  scale is the caller's noise_lr * lr[GS_ADAM_POSITION].
 * GS_ERR_INVALID: a NULL records, n == 0, a scale, gate_k or gate_x0 that is not finite, a NULL count_dev with ids given and
 * max_rows > 0.  ids with max_rows == 0: GS_OK, nothing launched.
 *
 * Out of scope: the opacity and scale regularisers of the MCMC loss are constant gradients the caller adds to the rows, and
 * no schedule is built in. */
int gs_relocate_device(gs_ctx* ctx, float* records, float* raw, float* m, float* v, uint32_t n,
                       float min_opacity, uint64_t seed,
                       uint32_t* ids_out, uint32_t max_rows, uint32_t* counts_out /* [3] */);
int gs_grow_device(gs_ctx* ctx, const float* records, const float* raw, const float* m, const float* v, uint32_t n,
                   float min_opacity, uint64_t seed, uint32_t n_add,
                   float* records_out, float* raw_out, float* m_out, float* v_out,
                   uint32_t max_out, uint32_t* counts_out /* [2] */);
int gs_position_noise_device(gs_ctx* ctx, float* records, float* raw, uint32_t n, const uint32_t* ids,
                             const uint32_t* count_dev, uint32_t max_rows, float scale, float gate_k, float gate_x0,
                             uint64_t seed);

/* Several views per optimiser step (no reference counterpart): the lists of two frames name different splats, so their rows
 * cannot simply be added.  Two calls sum the (ids, rows, count) lists of any number of frames into one list over the union of
 * their splats, which gs_adam_rows[_raw]_device, gs_upload_rows_device and gs_densify_stats_device take unchanged.  All arrays
 * are the CALLER's, on the DEVICE: acc is float[n][84] in the record layout, mark is uint32[n].  Both calls are enqueued on the
 * context's stream with no host sync, need no scene and no resolution, keep no state in the library and are bitwise
 * reproducible; the host never reads a count.  Callers detect them by their symbols (GS_API_VERSION is unchanged).
 *
 * gs_rows_accumulate_device: ids_dev, grad_rows_dev and count_dev as gs_backward_visible_device leaves them.  For every
 * i < min(*count_dev, max_rows), g = ids[i] (an id >= n is skipped: compared, never dereferenced; ids are distinct), and for
 * each of the 59 fields f of the record (the floats the GS_ADAM_* groups name), float32, a multiply and then an add, never
 * contracted:
 *   mark[g] == 0 :  acc[g][f] = weight * row[i][f]                      (a store: the old value is not read)
 *   otherwise    :  acc[g][f] = acc[g][f] + weight * row[i][f]
 *   then            mark[g] += 1
 * So acc needs no initialisation -- only mark starts as zeros --, a batch of one frame with weight == 1.0f reproduces that
 * frame's rows bit for bit (-0.0f included), and mark[g] counts the lists that named g.  The other 25 floats of an acc row are
 * never read or written; ids, grad_rows and count_dev are only read.  The sum of a batch depends on the order of its calls by
 * float association alone.  The grid is sized from max_rows and the blocks past the count exit at once.  max_rows == 0:
 * GS_OK, nothing launched.
 * GS_ERR_INVALID with a message in gs_last_error, nothing enqueued (a NULL ctx: the code alone): a NULL pointer with
 * max_rows > 0, n == 0, a weight that is not finite, an acc that shares bytes with grad_rows.
 *
 * gs_rows_collect_device: let U = { g < n : mark[g] != 0 }, in ascending g.  *count_out_dev = |U|, not clamped.  For
 * i < min(|U|, max_rows): ids_out[i] = the i-th member of U, and rows_out[i] = the 59 fields of acc[that g] bit for bit with
 * +0.0f in the other 25 floats -- the row shape gs_backward_visible* writes.  Nothing past the written rows is touched.
 * Afterwards mark[g] == 0 for every g < n, the members of U beyond max_rows included: THEIR SUMS ARE DROPPED with the batch
 * (the count says how many there were), so size max_rows for the union, n at most.  acc is only read.  |U| == 0: count 0,
 * nothing written.  max_rows == 0 is a count query that still clears mark; ids_out and rows_out may be NULL then.  Scratch:
 * the context's per-splat scan buffers, shared with gs_densify_device (4 bytes per splat + 20 bytes per 256 splats), grown
 * on demand and freed by gs_destroy.
 * GS_ERR_INVALID (message, nothing enqueued; a NULL ctx: the code alone): a NULL acc, mark or count_out, n == 0 or n >= 2^31,
 * a NULL ids_out or rows_out with max_rows > 0, a rows_out that shares bytes with acc, an ids_out or count_out that shares
 * bytes with mark. */
int gs_rows_accumulate_device(gs_ctx* ctx, float* acc_dev, uint32_t* mark_dev, uint32_t n,
                              const uint32_t* ids_dev, const float* grad_rows_dev, const uint32_t* count_dev,
                              uint32_t max_rows, float weight);
int gs_rows_collect_device(gs_ctx* ctx, const float* acc_dev, uint32_t* mark_dev, uint32_t n,
                           uint32_t* ids_out_dev, float* rows_out_dev, uint32_t max_rows, uint32_t* count_out_dev);

/* A cloud from points (no reference counterpart): the first records of a training run from an SfM or LiDAR point cloud, what
 * the INRIA trainer's create_from_pcd makes -- scale = the root of the mean squared distance to the three nearest other
 * points, opacity 0.1, identity rotation, SH DC from the colour.  Both device calls work on the CALLER's device arrays, are
 * enqueued on the context's stream without a host sync, need no scene and no resolution, keep no state in the library and
 * are bitwise reproducible, the same for every sorter.  Callers detect them by their symbols (GS_API_VERSION is unchanged).
 * Scratch: 45 bytes per point (24 of the sorter's lists, 16 of the sorted positions, 4 of the distances, 1 of the boxes and
 * the sorter's tables together) plus 100 KB, the context's, grown on demand and freed by gs_destroy.
 *
 * gs_knn_mean_dist2_device: points_dev float[n][3]; for every point i, in input order,
 *   d2(i, j) = (dx * dx + dy * dy) + dz * dz with dx = x_j - x_i, float32, never contracted, over all j != i -- a duplicate
 *   point counts, with d2 = 0: only the index itself is excluded;
 *   a <= b <= c the three smallest of those values;   dist2_out[i] = ((a + b) + c) / 3.0f.
 * The result is exact: a function of the multiset of d2 values, so independent of search order and ties, and equal to a
 * NumPy float32 brute force bit for bit (tests/test_init_cpu.py).  The search runs over the points in the loader's Morton
 * order, a wave per 64 of them, and drops a box of 64 points only when a bound computed in the shape of d2 itself -- and so
 * never above the d2 of any member -- exceeds the third best so far.
 *
 * gs_records_from_points_device: what gs_load_ply would make of the .ply an INRIA trainer writes at iteration 0.
 * points_dev is in the .ply's frame; colors_dev is float[n][3] in [0, 1], or NULL.  The output rows are in the loader's
 * Morton order, restated on the device over the flipped positions: bounds from the loader's start values (min from FLT_MAX,
 * max from the smallest positive normal float, as written there), q_a = (pos_a - min_a) / delta_a * 1023.0f truncated to
 * uint32 (a NaN and values <= 0 give 0, values >= 2^32 saturate; a flat axis gives 0 / 0 = NaN, then 0), the code
 * (part(q2) << 2) + (part(q1) << 1) + part(q0), a stable sort over all 32 bits.  A cloud from this call is therefore already
 * in the loader's order: written with gs_write_ply and loaded again, no row moves.  order_out[k] (may be NULL) = the input
 * index of output row k.  Row r = records_out[k] of input i = order_out[k]:
 *   r[0..2]  = (-x, -y, z)
 *   r[4..6]  = s:  d = dist2[i] < min_dist2 ? min_dist2 : dist2[i];  s = sqrtf(d);  s = s > max_scale ? max_scale : s
 *              (dist2 as gs_knn_mean_dist2_device defines it; sqrtf correctly rounded)
 *   r[8..11] = (-0.0f, -0.0f, 1.0f, -0.0f): the loader's record of rot_0..3 = (1, 0, 0, 0), signs of zero included
 *   r[12 + c] = (colour_c - 0.5f) / 0.28209479177387814f, c = 0..2 (correctly rounded); +0.0f with colors_dev == NULL
 *   r[15]    = opacity
 *   every other float of the 84: +0.0f.
 * The call writes records, not raw rows: for the trainer's parameters follow it with gs_raw_from_records_device, then
 * gs_records_from_raw_device ("Starting from points").
 * Points must be finite.  With non-finite coordinates both calls still terminate -- every loop is bounded by n -- and the
 * affected rows are unspecified.
 * GS_ERR_INVALID with a message in gs_last_error, nothing enqueued (a NULL ctx: the code alone): a NULL points_dev,
 * dist2_out_dev or records_out_dev; n < 4 ("fewer than four points have no three neighbours") or n >= 2^31; a NULL
 * gs_init_params or a wrong struct_size; an opacity that fails 0 < opacity < 1; a min_dist2 that is negative or not finite;
 * a max_scale that fails max_scale > 0 (+inf is allowed); an output array that shares bytes with an input or with the other
 * output. */
typedef struct gs_init_params {
    uint32_t struct_size;   /* sizeof(gs_init_params) of the caller's header: filled by gs_default_init_params, checked */
    float opacity;          /* 0.1f: the record's opacity (float 15) */
    float min_dist2;        /* 1e-7f: floor of the mean squared distance (INRIA's clamp_min) */
    float max_scale;        /* +inf = none: cap of the initial scale */
} gs_init_params;
void gs_default_init_params(gs_init_params* p);
int gs_knn_mean_dist2_device(gs_ctx* ctx, const float* points_dev, uint32_t n, float* dist2_out_dev);
int gs_records_from_points_device(gs_ctx* ctx, const float* points_dev, const float* colors_dev, uint32_t n,
                                  const gs_init_params* p, float* records_out_dev, uint32_t* order_out_dev);

/* Photometric loss of a frame against a photograph (no reference counterpart): the number a 3DGS optimisation minimises,
 *   loss = (1 - lambda) * L1 + lambda * DSSIM,
 * and its gradient with respect to the frame, in the layout gs_backward* takes.  H and W are the context's resolution.
 * Input: rgba float[H][W][4] (the quantities of GS_OUTPUT_RGBA32F: premultiplied colour before the clamp and alpha =
 * 1 - T_end), target float[H][W][3], bg[3] (HOST floats in both forms; NULL = black), lambda in [0, 1].
 *   I_c    = rgba_c + (1 - rgba_a) * bg_c, not clamped; with bg == NULL, I = rgb and alpha is not read into the loss;
 *   L1     = the mean over the H * W * 3 values of |I - G|; its derivative is sign(I - G), sign(0) = 0;
 *   SSIM   : per channel, window 11 x 11 separable, w(k) ~ exp(-k^2 / (2 * 1.5^2)), k = -5 .. 5, normalised to sum 1 in
 *            double and rounded once to float; pixels outside the image count as ZERO (what conv2d(padding = 5, groups = 3)
 *            computes).  With conv = that convolution: mu1 = conv(I), mu2 = conv(G), s1 = conv(I I) - mu1 mu1,
 *            s2 = conv(G G) - mu2 mu2, s12 = conv(I G) - mu1 mu2, C1 = 0.01^2, C2 = 0.03^2,
 *            ssim = ((2 mu1 mu2 + C1) (2 s12 + C2)) / ((mu1^2 + mu2^2 + C1) (s1 + s2 + C2));
 *   DSSIM  = 1 - the mean over H * W * 3 of ssim.
 * Output: loss_out[3] = {loss, L1, DSSIM}; grad_rgba32f float[H][W][4] = dloss/d(rgba): r, g, b = dloss/dI_c,
 * a = -sum_c bg_c * dloss/dI_c, exactly 0.0f with bg == NULL.  grad_rgba32f == NULL: the three numbers only (one launch
 * fewer).  rgba32f == NULL: the context's own GS_OUTPUT_RGBA32F buffer of the last frame (no copy), under the conditions
 * and with the messages of gs_output_device.  GS_RENDER_FAST contexts are allowed: the loss does not ask how the image was
 * made.  I == G gives DSSIM = 0 and a zero gradient exactly.
 * Bitwise reproducible: no float atomics; every 16 x 16 tile sums its pixels in a fixed tree and one workgroup sums the
 * tiles in a fixed order (in double) -- the same bits from call to call, from both forms, and after any change of
 * resolution and back.  Scratch: 36 bytes per pixel + 8 bytes per tile, allocated on the first call and freed with the
 * resolution; gs_photometric_loss also stages its arguments on the device (44 bytes per pixel).
 *   gs_photometric_loss        : HOST pointers; synchronous (loss_out and grad_rgba32f are written when it returns).
 *   gs_photometric_loss_device : DEVICE pointers (bg: host); enqueued on the context's stream, no host sync.
 * GS_ERR_INVALID with a message in gs_last_error, nothing enqueued: a NULL target_rgb or loss_out, a lambda outside [0, 1]
 * or not finite, a non-finite bg, no resolution set, a sharded context (gs_dist_shard_rows), a context that owns a subset
 * of the tile rows, grad_rgba32f equal to rgba32f (for rgba32f == NULL: to the context's buffer). */
int gs_photometric_loss(gs_ctx* ctx, const float* rgba32f, const float* target_rgb, float lambda, const float bg[3],
                        float loss_out[3], float* grad_rgba32f);
int gs_photometric_loss_device(gs_ctx* ctx, const float* rgba32f, const float* target_rgb, float lambda, const float bg[3],
                               float* loss_out, float* grad_rgba32f);

/* Runs ONLY the InitSortList stage of a frame (project + count scan + emit) and waits; afterwards
 * GS_BUF_UNSORTED_*, GS_BUF_COLOR, GS_BUF_COV and GS_BUF_COUNT are readable (stage-level parity). */
int gs_debug_init_sort_list(gs_ctx* ctx, const float view[16], const float proj[16],
                            const float cam_pos[3], uint32_t sh_mode);

/* Use a caller-owned hipStream_t (passed as void*) instead of the context's own stream.  NULL switches back
 * to the context's own (non-blocking) stream: the legacy default stream has handle 0 and cannot be selected --
 * a caller that works on it must create a stream of its own and hand that over. */
int gs_set_stream(gs_ctx* ctx, void* hip_stream);

/* Camera::updateDirVectors + updateMatrices (Engine/Graphics/Camera.cpp:7-48): yaw/pitch/position
 * -> view (glm::lookAt) and proj (glm::perspective(radians(90), aspect, near, far), depth 0..1). */
int gs_camera_matrices(const float pos[3], float yaw, float pitch, float aspect, float near_plane,
                       float far_plane, float view_out[16], float proj_out[16]);

/* GpuSort seam used stand-alone (GpuSort.h:8-22: initForScene + gpuClearBuffers + computeSort on
 * caller data): sorts n (tile, depth, id) triples held in HOST arrays, stable, by the low
 * num_sort_bits of (tile<<32 | depth), with the same kernels the frame uses.  In place. */
int gs_sort_host(gs_ctx* ctx, uint32_t* tile, uint32_t* depth, uint32_t* id, uint32_t n,
                 uint32_t num_sort_bits);
/* Stress run for the sorter alone (BASELINE config E): n random triples generated on the device
 * (seeded), sorted `iters` times; returns the mean milliseconds of one full sort and verifies
 * sortedness on the device (sorted_ok = 1). */
int gs_sort_bench(gs_ctx* ctx, uint32_t n, uint32_t num_tiles, uint32_t iters, uint64_t seed,
                  float* ms_per_sort, uint32_t* sorted_ok);

/* Stream-bandwidth probe on the context's GPU (the "measured HBM roofline" denominator): kind 0 =
 * read with 16-byte loads, 1 = device-to-device copy with 16-byte accesses, 2 = read with 4-byte
 * loads, 3 = copy with 4-byte accesses, 4..7 = copy in the radix-scatter write pattern (three arrays,
 * tiles of 3072 / 6144 / 12288 / 49152 dwords written as 16 runs each), 10..12 = copies with four 16-byte loads in
 * flight per lane (10 plain, 11 non-temporal stores, 12 non-temporal loads and stores).  `bytes` per buffer; `blocks`
 * workgroups of 256 threads (0 = 2048).  Returns the mean over `iters` launches of bytes moved (read + written) per second. */
int gs_membench(gs_ctx* ctx, int kind, size_t bytes, uint32_t blocks, uint32_t iters, float* gbytes_per_s,
                float* ms_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* GSPLAT_H */
