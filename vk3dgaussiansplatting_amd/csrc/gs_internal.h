// gs_internal.h -- shared between the HIP kernels and the C-ABI host code of libgsplat_hip.so.
// gfx950 (MI355X / CDNA4) only: wave64, no other targets, no compatibility paths.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gs_record.h"

namespace gs {

constexpr int kWave = 64;
constexpr int kTile = 16;              // TILE_SIZE, Common.glsl:12 / Renderer.h:146
constexpr int kRadixBits = 4;          // RS_BITS_PER_PASS, RadixSort.h:36
constexpr int kBins = 1 << kRadixBits; // RS_BIN_COUNT

// ---- radix-sort tiling -------------------------------------------------------------------
// One workgroup (256 threads = 4 waves) owns kSortTile consecutive keys of the current pass.
// The reference uses 64 keys per group (RS_WORK_GROUP_SIZE, RadixSort.h:38); a 2048-key group
// shrinks the histogram table 32x and makes every global access of a pass a >= 256-byte run.
// 8 keys per thread is the measured optimum on MI355X (12 and 16 keys per thread
// were 3-20 % slower) and what the 16-bit word paths are written for (8 keys per 16-byte load).
constexpr int kSortThreads = 256;
constexpr int kSortKeysPerThread = 8;
constexpr int kSortTile = kSortThreads * kSortKeysPerThread; // 2048 keys
constexpr int kSegments = 512;                // reduce segments = Count workgroups; each owns a contiguous run of groups
                                              // (measured: 512 beats 256 and 1024 at configs A-E)
constexpr int kCoarse = 64;                   // coarse reduce segments (kSegments / kCoarse segments each): second Reduce level
constexpr int kMaxSortPasses = 16;            // 64 key bits / 4
// Fed counts (gs_sort.hip, k_scatter<.., FED>): lists of at most this many groups may sort without per-pass Count
// launches -- every Scatter workgroup then sums the count rows of all groups itself (G x 64 bytes out of L2).
#ifndef GS_FED_MAX_GROUPS
#define GS_FED_MAX_GROUPS 1024    /* measured on MI355X (profiles/r06_fed_probe.txt): fed wins below ~1100 groups, by more the shorter the list */
#endif
constexpr uint32_t kFedMaxGroups = GS_FED_MAX_GROUPS;

// ---- GS_SORT_RADIX8*: the same sort with 8-bit digits (gs_sort8.hip) ------------------------
constexpr int kBins8 = 256;
#ifndef GS_SORT8_SMALL_BELOW
#define GS_SORT8_SMALL_BELOW 12000000   /* lists that cannot hold this many elements sort in 2048-key groups */
#endif
constexpr int kSort8Threads = 256;
constexpr int kSort8KeysPerThread = 16, kSort8KeysSmall = 8;
constexpr int kSort8Tile = kSort8Threads * kSort8KeysPerThread;   // keys per group: 4096 ...
constexpr int kSort8TileSmall = kSort8Threads * kSort8KeysSmall;  // ... or 2048 (launch_radix_sort8 chooses)
constexpr uint32_t kSort8SmallBelow = GS_SORT8_SMALL_BELOW;
static_assert(kBins8 <= kBins * kCoarse, "a pass's 256 digit totals live in its slab of SortBuffers::coarse");

// ---- InitSortList tiling -----------------------------------------------------------------
constexpr int kProjThreads = 256;      // splats per workgroup in project + emit
// Pass 0 of the frame's depth sort inside InitSortList (k_emit<false, true>, gs_project.hip): k_project leaves the digit
// counts of its 256 splats (depth_key & 15, weighted by the tile count) as a row of sixteen, k_scan_blocks scans the sixteen
// columns over the blocks, and k_emit stores every element where the stable counting sort on that digit would put it.
#ifndef GS_EMIT_PASS0
#define GS_EMIT_PASS0 1             /* tuning: 0 = k_emit always writes the plain list and the sort runs its pass 0 */
#endif
constexpr uint32_t kPass0Chunk = 64;   // project blocks per chunk of the column scan: one workgroup of k_scan_blocks each
// chunks that cover the rows 0 .. blocks of SplatScratch::pass0_offs (row `blocks` holds the column totals)
__host__ __device__ inline uint32_t pass0_chunks(uint32_t blocks) { return blocks / kPass0Chunk + 1u; }
// SplatScratch::block_sums is zero-padded by this many words (k_scan_blocks reads whole 16-byte groups per thread); behind
// the padding, in the same allocation, lie pass0_hist (whole chunks of rows) and the two halves of pass0_chunk
constexpr uint32_t kBlockSumsPad = 8192;
__host__ __device__ inline uint32_t* pass0_hist_of(uint32_t* block_sums, uint32_t blocks) {
    return block_sums + ((blocks + kBlockSumsPad + 3u) & ~3u);      // rows are stored and cleared as 16-byte groups
}
__host__ __device__ inline uint32_t* pass0_chunk_of(uint32_t* block_sums, uint32_t blocks) {
    return pass0_hist_of(block_sums, blocks) + (size_t)pass0_chunks(blocks) * kPass0Chunk * kBins;
}

// Per-frame constants: CamUBO (ShaderStructs.h:37-41) + InitSortListPCD (7-12) + the shader
// #defines of Common.glsl:2-15.  Passed by value as a kernel argument.
struct FrameParams {
    float view[16];       // column-major
    float proj[16];
    float cam_pos[3];
    uint32_t sh_mode;     // integer, not float
    uint32_t width, height;
    uint32_t grid_w, grid_h;
    // Tile rows of this context (multi-GPU): rows first_row + k * row_stride < row_end, k = 0 .. rows_owned - 1, with
    // first_row = row_begin + row_phase.  One GPU: [0, grid_h), stride 1.  A contiguous band: [row_begin, row_end), stride 1.
    // Interleaved: every row_stride-th row of the whole grid starting at row_phase.  Inside a frame the sort list holds
    // COMPACT tile ids k * grid_w + x (k = index among the owned rows): same order as the global ids of the owned
    // tiles, no gaps, fewest key bits.
    uint32_t row_begin, row_end;
    uint32_t row_stride, first_row, rows_owned;
    uint32_t compact_out;         // image addressed in compact rows (pixel row of owned row k starts at 16 k): the strip
                                  // a rank contributes to the gather
    uint32_t num_gaussians;
    uint32_t capacity;
    float near_plane, far_plane;
    float ndc_cull, in_view_limit;
    float tan_fov_y;      // tan(FOV_Y*0.5f), folded on the host (Common.glsl:53)
    uint32_t hi16;        // sort list stores the compact tile ids as uint16 (at most 65535 owned tiles)
    float w_norm2;        // upper bound on the squared spectral norm of the upper-left 3x3 of view (host-folded, for the
                          // band bound; 1 for a rigid view matrix)
    uint32_t parity;      // InitSortList launches alternate between the two helper counters of SplatScratch
    uint32_t splat_first; // GS_SORT_RADIX4_SPLAT_FIRST: k_project also counts the emitting splats per block and leaves the
                          // helper records of k_emit to k_gather_sorted
    uint32_t packed;      // k_emit writes the packed payload (SortRun::packed, gs_sort_words.h): pk32 into the id plane, pk8
                          // into a byte plane in the storage of the tile words
    uint32_t antialias;   // gs_set_antialias: the raster opacity of an emitting splat is opacity * sqrt(det Sigma' / det(Sigma' +
                          // 0.3 I)), floored (kAntialiasFloor); k_project picks its instantiation by it, bwd_chain branches on it
};
// The floor under r = det Sigma' / det(Sigma' + 0.3 I) of an anti-aliased frame (the INRIA rasteriser's 0.000025): at or
// below it -- or with a NaN r -- the factor is the constant sqrt(floor) and passes no derivative to the covariance.
constexpr float kAntialiasFloor = 2.5e-5f;

// Device-side dispatch record: the role of RadixIndirectDispatch (ShaderStructs.h:45-57) +
// GaussianCullData (77-82).  Written by the scan kernel (IndirectSetup-equivalent), read by every
// later kernel, so the host never reads the element count back inside a frame.
struct SortParams {
    uint32_t num_elems;      // E' = min(counter, capacity)   (RadixSortIndirectSetup.comp:28)
    uint32_t num_groups;     // G  = ceil(E' / kSortTile)     (countSizeX)
    uint32_t groups_per_seg; // K  = ceil(G / kSegments)      (groups per reduce segment, <= 64)
    uint32_t overflow;       // counter > capacity
    uint64_t counter;        // un-truncated atomic-counter equivalent
    uint32_t pad[2];
};

// What RenderGaussians needs per splat, written once by the project kernel: the reference keeps color / covariance in
// the 336-byte record and redoes the screen position and the 2x2 inverse once per (tile, splat),
// RenderGaussians.comp:88-107; here that setup runs once per emitting splat -- same expressions, same operand order,
// so the same floats.  48 B, 16-aligned; RenderGaussians reads the first 36 bytes, the covariance rides along for
// gs_debug_read(GS_BUF_COV) at no extra traffic (the record is written in whole cache lines either way).
struct alignas(16) SplatRaster {
    float sx, sy;        // getScreenSpacePosition(...).xy                       RenderGaussians.comp:89-90
    float ix, iy, iz;    // gCovInv = (cz, -cy, cx) * (1 / det), 0 when det == 0  :94-107 (emitting splats only)
    float r, g, b;       // GaussianData.color.rgb                                :92
    float a;             // GaussianData.color.a, 0 when det == 0                 :92, :104
    float cx, cy, cz;    // GaussianData.covariance.xyz (raw, +0.3 dilation applied): every non-culled splat
};
static_assert(sizeof(SplatRaster) == 48, "SplatRaster must be 48 bytes");

// Device SoA image of the scene (converted once at upload from the 336-byte AoS records).
struct SceneBuffers {
    float* pos;      // [3][N] planes
    float* scale;    // [3][N]
    float* rot;      // [4][N]
    float* sh;       // [48][N], plane index = coeff*3 + channel
    float* opacity;  // [N]   shCoeffs[0].w
    float* sig2;     // [N]   upper bound of the largest eigenvalue of the 3-D covariance: |R|_F^2 * max(scale)^2,
                     //       computed at upload; lets a tile-row band skip far-away splats early (k_project)
    float* block_bounds; // [ceil(N / 64)][8]  per wave of 64 consecutive splats: min xyz, max xyz of their positions,
                     //       max sig2, pad -- a context with a subset of the tile rows drops a whole wave with one record
};

// Per-splat scratch of one frame.
struct SplatScratch {
    SplatRaster* raster;     // [N]
    uint32_t* depth_key;     // [N]
    uint32_t* tiles_touched; // [N]  0 for culled / zero-extent splats
    uint2* extents;          // [N]  packed u16: .x = minx | miny<<16, .y = maxx | maxy<<16 (row-clamped)
    uint8_t* wave_wrote;     // [4 * ceil(N/kProjThreads)]  one byte per wave of 64 splats, a mask of its four quarters: bit q
                             //       set = this frame's k_project stored the raster records of splats 16 q .. 16 q + 15 of the
                             //       wave (the others are stale -- an earlier frame's -- or zero: nothing behind the frame reads
                             //       them, gs_debug_read recomputes or zero-fills them).  0xF or 0 where whole waves are stored
                             //       (a band context, the GS_PROJECT_* tuning builds)
    uint32_t* block_sums;    // [ceil(N/kProjThreads)]  tile counts per project workgroup
    uint32_t* block_offsets; // same size, exclusive scan
    // k_emit load balance: a project workgroup whose 256 splats emit more than kEmitSlice elements registers one
    // helper record {block, slice} per further slice; k_emit runs them as extra workgroups.
    uint2* help_list;        // [kEmitHelpCap]
    uint32_t* help_count;    // [4]: [p] helper records registered by the InitSortList launch of parity p, [2 + p] its band
                             // survivors (below); k_scan_blocks clears the pair of the next launch (FrameParams::parity)
    uint32_t* help_slot;     // [ceil(N/kProjThreads)]: first record of a heavy block, kEmitNoHelp if the list was full
    // A context that owns a subset of the tile rows: the project blocks k_band_cull could not reject, in arrival order,
    // block | skipped-waves mask << 28.
    uint32_t* band_list;     // [ceil(N/kProjThreads)]
    // GS_SORT_RADIX4_SPLAT_FIRST only (null otherwise)
    uint32_t* block_flags;   // [blocks, padded like block_sums]  emitting splats per project workgroup
    uint32_t* flag_offsets;  // same size, exclusive scan
    uint32_t* sorted_sums;   // [blocks, padded]  tile counts per 256 positions of the sorted splat list
    SortParams* aux_params;  // [2]: the splat list's dispatch record; scratch for the second scan
    uint32_t* elems_note;    // device alias of a pinned host word (or null): k_scan_blocks leaves the frame's element count + 1
                             // there, so that the host knows the length of recent lists without waiting for a frame
    // Pass 0 of the depth sort inside InitSortList (GS_EMIT_PASS0).  Rows of sixteen words, one per value of depth_key & 15:
    // (pass0_hist and pass0_chunk live behind block_sums: pass0_hist_of / pass0_chunk_of, which k_project reaches them by)
    uint32_t* pass0_hist;    // [blocks][16]      elements of each digit the block's splats emit (k_project; zero row: k_band_cull)
    uint32_t* pass0_offs;    // [blocks + 1][16]  column d summed over the blocks before (k_scan_blocks); row `blocks` = the totals
    uint32_t* pass0_chunk;   // [2][chunks][16]   the rows summed per kPass0Chunk blocks, added by the k_project launch of
                             //       parity p into half p; k_scan_blocks clears the half of the next launch
    float* view_z;           // [N] while GS_OUTPUT_DEPTH is on (null otherwise): -viewSpacePos.z of the emitting splats, the
                             //       value getDepthKey quantises (InitSortList.comp:70-80); what the depth output blends
};
#ifndef GS_EMIT_SLICE
#define GS_EMIT_SLICE 4096
#endif
constexpr uint32_t kEmitSlice = GS_EMIT_SLICE;      // output elements per k_emit workgroup (a multiple of its 1024-element round)
constexpr uint32_t kEmitHelpCap = 65536;   // enough for 2^28 elements; beyond that the owner workgroup does the rest itself
constexpr uint32_t kEmitNoHelp = 0xFFFFFFFFu;
// helper workgroups of a k_emit launch = records k_project may register: the slices after the first number at most
// E / kEmitSlice <= capacity / kEmitSlice over all blocks (more only when the list overflows its capacity)
__host__ __device__ inline uint32_t emit_helpers(uint32_t capacity) {
    const uint32_t by_capacity = capacity / kEmitSlice + 1u;
    return by_capacity < kEmitHelpCap ? by_capacity : kEmitHelpCap;
}

struct SortBuffers {
    uint32_t *lo[2], *hi[2], *id[2]; // ping-pong: depth word, tile word, gaussian index; [capacity]
    uint32_t* table;                 // [16][G_max]  per-group digit counts (sumTable); 8-bit digits: [G8_max][256]
    uint32_t* seg_sum;               // [16][kSegments]  per-segment digit counts (reduce buffer); 8-bit digits:
                                     // [256][kSegments] counts, then [256][kSegments] scanned
    uint32_t* coarse;                // [kMaxSortPasses][16][kCoarse]  per-pass digit counts of the coarse segments
                                     // (8-bit digits: the first 256 words of a pass's slab = its digit totals)
    uint32_t* fed[3];                // 4-bit digits: [G_max][16] digit counts per group, three rotating sets of the fed
                                     // sort (k_scatter<.., FED>); null for 8-bit digits
    SortParams* params;              // [2]: the list's dispatch record; the same for the launches of a pass k_emit has done
                                     // already (SortRun::done_params): no elements unless the frame overflows
    uint32_t digit_bits;             // what alloc_sort sized table / seg_sum for (4 or 8): the digit width of every run over these buffers
};

// One run of radix passes: key bits [first_bit, num_sort_bits) of tile << 32 | depth over the list in ping-pong half
// `start` of a SortBuffers (in a frame the tile word is the compact tile id of FrameParams: a context that owns a subset of
// the tile rows sorts over fewer significant bits).  The digit width is SortBuffers::digit_bits.
struct SortRun {
    uint32_t capacity = 0;             // elements the list can hold: sizes the grids
    uint32_t first_bit = 0;
    uint32_t num_sort_bits = 0;
    int start = 0;
    uint32_t coarse_pass = 0;          // first slab of SortBuffers::coarse (one per pass; two runs of a frame must not share slabs)
    const SortParams* params = nullptr;   // dispatch record of this list (null: SortBuffers::params)
    uint32_t passes_done = 0;          // the list in half `start` is already in the order of this many leading passes (k_emit
                                       // stores a frame's list where pass 0 would: 1); the run goes on with pass passes_done,
                                       // whose word layout, coarse slab and key bit are those of that pass of the whole run
    const SortParams* done_params = nullptr;   // with passes_done: the leading passes are launched all the same, over this
                                       // dispatch record, from the half they would have started in.  It holds no elements
                                       // (the launches return at once) unless the producer had to leave the plain list there
    bool drop_depth_payload = false;   // frame path: a pass carries only the depth bytes that later passes still read
    bool hi16 = false;                 // frame path: the hi arrays hold 16-bit tile ids (at most 65535 owned tiles)
    bool packed = false;               // frame path, 4-bit digits, hi16, first_bit == 0, at least 32 sort bits, at most 2^24
                                       // splats: through the depth passes the payload travels as pk32 + pk8 (gs_sort_words.h)
    float share = 1.0f;                // the context's share of the tiles: below one half the grids shrink with it
    bool fed = false;                  // 4-bit digits only -- one Count launch for the whole run, every Scatter feeds the next
                                       // pass's counts (k_scatter<.., FED>); same output, meant for at most kFedMaxGroups groups
    hipEvent_t* scatter_events = nullptr;   // optional 2 * passes events recorded right before / after every Scatter launch
};

// Pass k of a run, as the launchers dispatch it and as the timing code reports the bytes it moves.
struct SortPass {
    uint32_t shift;          // of the 64-bit key
    uint32_t bits, mask;     // of this pass's digit (the last 8-bit pass may be narrower)
    bool tile_word;          // the digit lies in the tile word (shift >= 32), else in the depth word
    bool word16;             // that word is stored as 16 bits: the tile ids of a band (hi16) and, in a frame, the upper
                             // half of the depth word once the lower half is consumed (gs_sort_words.h)
    uint32_t word_shift;     // of the digit within the word as stored (= word_shift_of, gs_sort_words.h)
    int lo_in, lo_out;       // bytes of the depth word read / written per element (LO_IN / LO_OUT of gs_sort_words.h)
    int pk_in, pk_out;       // form of the payload read / written (kPk*; PK_IN / PK_OUT of gs_sort_words.h)
    bool last;
};
// The payload of an element: kPkNone = tile word + 32-bit splat index; else pk32 = tile16 << 16 | (id & 0xFFFF) in the id
// plane and pk8 = id >> 16 either in a byte plane (kPkPlane) or in the lowest byte of the stored depth word, once a
// pass has consumed that byte (kPkWord).
constexpr int kPkNone = 0, kPkPlane = 1, kPkWord = 2;
#ifndef GS_SORT_PACKED_PAYLOAD
#define GS_SORT_PACKED_PAYLOAD 1    /* tuning: 0 = a frame never packs the payload of its depth passes (the layouts before) */
#endif
constexpr uint32_t kPackedMaxSplats = 1u << 24;   // pk32 + pk8 hold a 24-bit splat index
// SortRun::packed of a frame of the contractual sorter (enqueue_frame): 16-bit tile ids, splat indices below 2^24.  A
// frame with per-pass timers (record_timings >= 2: nothing captured, an event pair around every Scatter launch) sorts in
// the unpacked layouts: its scatter_bytes_per_elem and scatter_ms_avg are the figures of the word layouts alone, which
// the recorded per-pass profiles and tests/test_parity_gpu.py (17.5 bytes for this sorter) are stated in.
inline bool frame_packs_payload(bool hi16, uint32_t num_gaussians, uint32_t record_timings) {
    return GS_SORT_PACKED_PAYLOAD != 0 && hi16 && num_gaussians <= kPackedMaxSplats && record_timings < 2u;
}
inline uint32_t sort_pass_count(const SortRun& r, uint32_t digit_bits) {
    return r.num_sort_bits > r.first_bit ? (r.num_sort_bits - r.first_bit + digit_bits - 1u) / digit_bits : 0u;
}
inline SortPass sort_pass(const SortRun& r, uint32_t digit_bits, uint32_t k) {
    SortPass p{};
    p.shift = r.first_bit + k * digit_bits;                                                // RadixSort.cpp:309
    p.bits = r.num_sort_bits - p.shift < digit_bits ? r.num_sort_bits - p.shift : digit_bits;
    p.mask = (1u << p.bits) - 1u;
    p.tile_word = p.shift >= 32u;
    p.last = p.shift + digit_bits >= r.num_sort_bits;
    p.lo_in = 4; p.lo_out = 4;
    if (r.drop_depth_payload) {
        if (p.tile_word) { p.lo_in = 0; p.lo_out = 0; }
        else if (r.first_bit == 0u) {   // what the passes still to come read: nothing below bit shift + digit_bits
            p.lo_in = p.shift >= 16u ? 2 : 4;
            p.lo_out = p.shift + digit_bits >= 32u ? 0 : (p.shift + digit_bits >= 16u ? 2 : 4);
        }
    }
    p.pk_in = kPkNone; p.pk_out = kPkNone;
    if (r.packed && r.drop_depth_payload && r.hi16 && r.first_bit == 0u && r.num_sort_bits >= 32u && digit_bits == 4u &&
        !p.tile_word) {
        // pk8 rides in byte 0 of the depth word as stored once the passes before have consumed that byte: key bits
        // 0-7 of a 32-bit word, 16-23 of the upper half; the last depth pass unpacks.  A fed run (short lists, bound by
        // latency) keeps the unpacked element where the byte plane would lie beside a 16-bit depth word, out of passes 3
        // and 4: those two launches measured 1.1 - 1.8 us slower with it at config A (profiles/packed_words_cost.txt)
        const bool fed = r.fed;
        auto form = [fed](uint32_t first_live_bit) {
            if (first_live_bit >= 32u) return kPkNone;
            if ((first_live_bit & 15u) >= 8u) return kPkWord;
            return fed && first_live_bit >= 16u ? kPkNone : kPkPlane;
        };
        p.pk_in = form(p.shift);
        p.pk_out = form(p.shift + digit_bits);
    }
    const bool lo16 = !p.tile_word && p.lo_in == 2;
    p.word16 = (p.tile_word && r.hi16) || lo16;
    p.word_shift = lo16 ? p.shift - 16u : p.shift & 31u;
    return p;
}
// Bytes of an element on one side of a Scatter launch: `lo` depth bytes + the payload in form `pk`; of pass p: read + written
inline uint32_t sort_elem_bytes(int lo, int pk, bool hi16) {
    return (uint32_t)lo + (pk == kPkNone ? (hi16 ? 2u : 4u) + 4u : (pk == kPkPlane ? 1u + 4u : 4u));
}
inline uint32_t sort_pass_bytes(const SortPass& p, bool hi16) {
    return sort_elem_bytes(p.lo_in, p.pk_in, hi16) + sort_elem_bytes(p.lo_out, p.pk_out, hi16);
}

// ---- launchers (each enqueues on `stream`, no host sync) ------------------------------------
void launch_project(const FrameParams& fp, const SceneBuffers& scene, const SplatScratch& sc,
                    hipStream_t stream);
// sums == nullptr: block_sums -> block_offsets, the frame's clears, the IndirectSetup record in `params`.
// gs_debug_read of a full-grid context, on demand from the last frame's camera.  out_records: float[n][8], what k_project
// computed and did not store for the splats that passed the culls and touched no tile (k_debug_records); out_rgba: float[n][4],
// their colours, from those records' flags
void launch_debug_records(const FrameParams& fp, const SceneBuffers& scene, const SplatScratch& sc, float* out_records, hipStream_t stream);
void launch_debug_colour(const FrameParams& fp, const SceneBuffers& scene, const float* records, float* out_rgba, hipStream_t stream);
void launch_scan_blocks(const FrameParams& fp, const SplatScratch& sc, SortParams* params,
                        uint32_t* ranges, uint32_t* coarse, hipStream_t stream);
// pass0: the list goes to half 1, in the order pass 0 of the depth sort would leave it (GS_EMIT_PASS0; an overflowing
// frame writes the plain list into half 0 all the same, and sb.params[1] says so to the sort)
void launch_emit(const FrameParams& fp, const SplatScratch& sc, const SortBuffers& sb, bool pass0,
                 hipStream_t stream);
// GS_SORT_RADIX4_SPLAT_FIRST (gs_project.hip): the (depth word | tile count | splat) list of the emitting splats into
// sort buffers [1] (lo, hi, id), with its dispatch record in sc.aux_params[0]; then, once that list is sorted by depth
// (buffers [sorted]), the sums of its tile counts + their scan; then the emit in depth order into buffers [0].
void launch_splat_list(const FrameParams& fp, const SplatScratch& sc, const SortBuffers& sb, hipStream_t stream);
void launch_gather_sorted(const FrameParams& fp, const SplatScratch& sc, const SortBuffers& sb, int sorted, hipStream_t stream);
void launch_emit_sorted(const FrameParams& fp, const SplatScratch& sc, const SortBuffers& sb, int sorted, hipStream_t stream);
// Sorts the list of `run` -> the ping-pong half (0 or 1) that holds the result; -1 without launching anything when the
// buffers cannot serve the run (another digit width, fed counts without their rows).  sb.coarse must be zero on entry.
int launch_radix_sort(const SortBuffers& sb, const SortRun& run, hipStream_t stream);
// the same with 8-bit digits (gs_sort8.hip); launch_radix_sort forwards here when sb.digit_bits == 8
int launch_radix_sort8(const SortBuffers& sb, const SortRun& run, hipStream_t stream);
// GS_SORT_TILE_BUCKET: per-tile depth sort of the owned tiles (gs_tilesort.hip)
int init_tile_sort();
void launch_tile_sort(const FrameParams& fp, const uint32_t* ranges, uint32_t* lo, uint32_t* id,
                      uint32_t* lo_alt, uint32_t* id_alt, hipStream_t stream, hipStream_t helper = nullptr,
                      hipEvent_t fork = nullptr, hipEvent_t join = nullptr);
void launch_find_ranges(const FrameParams& fp, const uint32_t* sorted_tile, const SortParams* params,
                        uint32_t* ranges, hipStream_t stream);
// order[k] = the k-th tile RenderGaussians dispatches, as an index among the context's own tiles, longest list first
void launch_tile_order(const FrameParams& fp, const uint32_t* ranges, uint32_t* order, hipStream_t stream);
size_t tile_order_words(uint32_t grid_w, uint32_t grid_h);   // words `order` must hold: the table and the kernels' scratch
// The optional per-pixel outputs of a frame (gs_set_outputs), addressed like the RGBA8 image: rgba32f = premultiplied
// colour before the clamp + 1 - T_end, depth = the colour's blend of view_z.  All null: the RGBA8 frame alone.
struct RenderOutputs {
    float4* rgba32f;         // [H][W] or null
    float* depth;            // [H][W] or null
    const float* view_z;     // SplatScratch::view_z (needed with depth)
};
// order == nullptr: raster order
void launch_render(const FrameParams& fp, const SplatRaster* raster, const uint32_t* sorted_id,
                   const uint32_t* ranges, const uint32_t* order, uint8_t* rgba, uint32_t render_mode,
                   uint32_t render_kernel, hipStream_t stream, const RenderOutputs& outs = RenderOutputs{});
// The buffers of one per-splat scan (gs_splat_scan.h) of K sums over n splats, in blocks of 256 splats
struct SplatScan {
    uint32_t* offsets;        // [n]  row 0 summed over the splats before g, saturated at 2^32 - 1
    uint32_t* block_sums;     // [K][ceil(n / 256)]
    uint32_t* block_offsets;  // [K][ceil(n / 256)]  exclusive scan of block_sums, row 0 saturated
    uint32_t* totals;         // [K]  the grand totals of the rows whose total the caller asks for
};
// gs_backward* (gs_backward.hip): scratch of a backward pass, allocated on the first call
constexpr int kRowFloats = 10;    // a row of BackwardBuffers::rows: dL/d{sx, sy, ix, iy, iz, r, g, b, a, z} of one list element, in
                                  // that order (screen position, inverse 2-D covariance, colour, opacity, view depth)
constexpr int kAbsRowFloats = 2;  // a row of BackwardBuffers::abs_rows: the sums over the tile's pixels of |dL_p/dsx| and |dL_p/dsy|
struct BackwardBuffers {
    float* rows;              // [capacity][kRowFloats]  per element, in its slot
    float* abs_rows;          // [capacity][kAbsRowFloats]  gs_set_abs_gradients: null until the first backward with the switch on;
                              // in a BackwardFrame: null unless THIS backward runs with the switch on (k_bwd_blend<true>)
    // row 0: tiles_touched, so offsets[g] = the first slot of splat g; row 1 (gs_backward_visible* only): the flag
    // tiles_touched != 0, whose scan is the position of g in V = the splats with tiles_touched != 0, ascending
    SplatScan scan;           // K = 2
    uint32_t* vis_ids;        // [N]  the first |V| entries: V
};
// |V| on the device after launch_backward_visible_scan: what its kernels and the host read
inline const uint32_t* visible_count_of(const BackwardBuffers& bb) { return bb.scan.totals + 1; }
inline size_t backward_row_bytes(uint32_t capacity) { return (size_t)capacity * kRowFloats * sizeof(float); }
inline uint32_t backward_blocks(uint32_t n) { return (n + 255u) / 256u; }   // 256 splats per block of the per-splat kernels
// The tile count of splat g in the last frame, as every kernel behind the frame reads it.  In a contiguous band of tile rows
// k_band_cull rejects whole project blocks: such a block gets a zero block sum and nothing else, so the tiles_touched (and
// extents, and raster records) of its 256 splats are whatever an earlier frame on the context left.  A block that runs
// writes the count of every one of its splats (0 for a skipped wave).  Hence the count of this frame is block_sums[g /
// kProjThreads] != 0 ? tiles_touched[g] : 0.  Every other frame (the whole grid, interleaved rows) runs every block:
// block_sums is null there and the count is the stored word, at no cost.
struct SplatCounts {
    const uint32_t* touched;          // SplatScratch::tiles_touched
    const uint32_t* block_sums;       // SplatScratch::block_sums, per kProjThreads splats, or null: no block was culled
    __device__ __forceinline__ uint32_t of(uint32_t g) const {
        return block_sums && block_sums[g / (uint32_t)kProjThreads] == 0u ? 0u : touched[g];
    }
};
inline SplatCounts splat_counts_of(const SplatScratch& sc, const FrameParams& fp) {
    const bool culled = !(fp.row_begin == 0u && fp.row_end == fp.grid_h) && fp.row_stride == 1u;   // launch_project ran k_band_cull
    return SplatCounts{sc.tiles_touched, culled ? sc.block_sums : nullptr};
}
// The frame a backward pass differentiates: its FrameParams (GS_RENDER_EXACT; the whole grid, or the tile rows of a band
// context), the scene, what its forward left (scratch, sorted list, ranges) and the backward's own scratch
struct BackwardFrame {
    FrameParams fp;
    SceneBuffers scene;
    SplatScratch sc;
    const uint32_t* sorted_id;
    const uint32_t* ranges;
    BackwardBuffers bb;
};
// dL/d(record) [N][84] of the frame, from dL/dRGBA32F [H][W][4] and dL/dDEPTH [H][W] (may be null).
void launch_backward(const BackwardFrame& f, const float* grad_rgba, const float* grad_depth, float* grad_records,
                     hipStream_t stream);
// The visible form, in two steps on one stream.  _scan: the slot offsets of launch_backward plus V (bb.vis_ids, |V| at
// visible_count_of(bb)); ids_out (device, may be null) gets the first max_rows of V, count_out (device, may be null)
// |V|.  _rows: the blend backward, then record gradient i of splat vis_ids[i] into grad_rows[i][84], i < min(|V|, max_rows).
void launch_backward_visible_scan(const BackwardFrame& f, uint32_t* ids_out, uint32_t max_rows, uint32_t* count_out,
                                  hipStream_t stream);
void launch_backward_visible_rows(const BackwardFrame& f, const float* grad_rgba, const float* grad_depth,
                                  uint32_t max_rows, float* grad_rows, hipStream_t stream);
// The slot offsets alone (row 0 of the scan, what launch_backward runs first): scan.offsets[g] = the first slot of splat g.
// Over the buffers of a backward's scan it rewrites the values that are there and leaves V and |V| alone.
void launch_slot_offsets(const SplatCounts& counts, uint32_t n, const SplatScan& scan, hipStream_t stream);
// gs_debug_read(GS_BUF_BACKWARD_ROWS): out[N][kRowFloats] (device) = per splat the sum of its rows in bb.rows exactly as
// k_bwd_rowsum_chain adds them (the input of bwd_chain), zeros for a splat outside the list.  Needs bb.scan.offsets and
// bb.rows of a launch_backward* on this frame.
void launch_backward_row_sums(const BackwardFrame& f, float* out, hipStream_t stream);
// gs_contrib_device (gs_contrib.hip): a row {sum, max, count} of the blend weights of one list element, in its slot
constexpr int kContribRowWords = 3;
inline size_t contrib_row_bytes(uint32_t capacity) { return (size_t)capacity * kContribRowWords * sizeof(uint32_t); }
// wmax / wsum / pixels [N] (device; wsum and pixels may be null) accumulate the frame's blend weights per splat; offsets:
// the slot offsets of the frame, rows: contrib_row_bytes(capacity) of scratch.  f.bb is not used.
void launch_contrib(const BackwardFrame& f, const uint32_t* offsets, uint32_t* rows, float* wmax, float* wsum,
                    uint32_t* pixels, hipStream_t stream);
// gs_backward_camera* (gs_camera.hip): from the rows a launch_backward* left in bb.rows, grad_camera[35] = dL/dview[16],
// dL/dproj[16], dL/dcam_pos[3] (device); partials: backward_camera_partial_bytes(N) of scratch, [35][backward_blocks(N)]
size_t backward_camera_partial_bytes(uint32_t n);
void launch_backward_camera(const BackwardFrame& f, float* partials, float* grad_camera, hipStream_t stream);
// gs_photometric_loss* (gs_loss.hip): scratch of the loss, allocated on the first call and freed with the resolution
struct LossBuffers {
    float* maps;              // [3][H][W][3]  A, B, E of gs_loss.hip: derivatives of ssim, scaled by -lambda / (3 H W)
    float* tile_sums;         // [tiles][2]    per 16 x 16 tile: sum of 1 - ssim, sum of |I - G|
};
size_t loss_map_bytes(uint32_t width, uint32_t height);
size_t loss_tile_bytes(uint32_t width, uint32_t height);
// loss_out[3] = {loss, L1, DSSIM} and, unless grad is null, grad[H][W][4] = dloss/dRGBA32F of rgba[H][W][4] against
// target[H][W][3]; bg: three HOST floats or null (black).  All other pointers are device pointers.
void launch_photometric_loss(const LossBuffers& lb, const float* rgba, const float* target, float lambda, const float* bg,
                             uint32_t width, uint32_t height, float* loss_out, float* grad, hipStream_t stream);
void launch_aos_to_soa(const float* chunk, uint32_t first, uint32_t count, uint32_t n,
                       const SceneBuffers& s, hipStream_t stream);
void launch_block_bounds(uint32_t n, const SceneBuffers& s, hipStream_t stream);
// gs_upload_rows_device: the planes of splats ids[i], i < min(*count, max_rows), rewritten from records[ids[i]] (records: the
// whole [n][84] array); an id >= n is skipped.  The caller rebuilds the block bounds.  max_rows > 0.
void launch_upload_rows(const float* records, uint32_t n, const uint32_t* ids, const uint32_t* count, uint32_t max_rows,
                        const SceneBuffers& s, hipStream_t stream);
// gs_adam_rows_device (gs_adam.hip): what the kernel needs of gs_adam_params, the bias correction folded into step[] on the host
struct AdamStep {
    float beta1, beta2, c1, c2, eps;
    float step[6], lo[6], hi[6];      // per GS_ADAM_* group
};
void launch_adam_rows(float* records, float* m, float* v, uint32_t n, const uint32_t* ids, const float* grad_rows,
                      const uint32_t* count, uint32_t max_rows, const AdamStep& a, hipStream_t stream);
// The raw parameter space (gs_raw.hip).  launch_adam_rows_raw: launch_adam_rows on raw / m / v with the chain from the record
// gradient in front and records[fields] = act(raw') behind.  launch_convert_space: dst = act(src) on the fields of n rows, or
// with to_raw its inverse.  launch_reset_opacity_raw: float 15 of every row (m, v: both null or neither); logit = the raw
// value a reset opacity gets.
void launch_adam_rows_raw(float* raw, float* records, float* m, float* v, uint32_t n, const uint32_t* ids,
                          const float* grad_rows, const uint32_t* count, uint32_t max_rows, const AdamStep& a,
                          hipStream_t stream);
void launch_convert_space(const float* src, float* dst, uint32_t n, bool to_raw, hipStream_t stream);
void launch_reset_opacity_raw(float* raw, float* records, float* m, float* v, uint32_t n, float max_opacity, float logit,
                              hipStream_t stream);
// gs_densify_stats_device (gs_densify.hip): the listed ids of the frame, what its backward left, and the caller's arrays
struct DensifyStatsArgs {
    const uint32_t* ids;
    const uint32_t* count;
    uint32_t max_rows, n;
    SplatCounts counts;               // splat_counts_of(the frame's scratch)
    const uint32_t* offsets;          // BackwardBuffers::scan.offsets
    const float* rows;                // BackwardBuffers::rows
    const SplatRaster* raster;
    uint32_t capacity, width, height;
    float* grad_accum;
    uint32_t* seen;
    float* max_radius;
};
void launch_densify_stats(const DensifyStatsArgs& a, hipStream_t stream);
// gs_abs_screen_gradient_device / gs_densify_stats_abs_device (gs_densify.hip): the listed ids of the frame and the absolute
// pairs its backward left (BackwardBuffers::abs_rows).  out: the pairs [max_rows][2] by list position, or the accumulator [n]
struct AbsGradArgs {
    const uint32_t* ids;
    const uint32_t* count;
    uint32_t max_rows, n;
    SplatCounts counts;               // splat_counts_of(the frame's scratch)
    const uint32_t* offsets;          // BackwardBuffers::scan.offsets
    const float* abs_rows;
    uint32_t capacity, width, height;
    float* out;
};
void launch_abs_screen_gradient(const AbsGradArgs& a, hipStream_t stream);
void launch_densify_stats_abs(const AbsGradArgs& a, hipStream_t stream);
inline size_t backward_abs_row_bytes(uint32_t capacity) { return (size_t)capacity * kAbsRowFloats * sizeof(float); }
// gs_densify_device: the thresholds of gs_densify_params, the caller's arrays and the context's scratch
struct DensifyRule {
    float grad_threshold, split_scale, prune_opacity, prune_scale, prune_radius;
};
struct DensifyArgs {
    const float *records, *m, *v;     // m, v, m_out, v_out: all null or none
    uint32_t n;
    const float* grad_accum;
    const uint32_t* seen;
    const float* max_radius;
    DensifyRule rule;
    float split_shrink;
    uint64_t seed;
    float *records_out, *m_out, *v_out;
    uint32_t max_out;
    SplatScan scan;                   // K = 4: outputs, cloned, split, pruned; offsets[g] = o(g), the index of g's first output
};
void launch_densify(const DensifyArgs& a, uint32_t* counts_out, hipStream_t stream);
// gs_prune_below_device: the rows g with score[g] >= threshold, ascending, into rows [0, kept) of every output below max_out
struct PruneArgs {
    const float* score;
    float threshold;
    uint32_t n;
    const float *records, *raw, *m, *v;            // raw, m, v: each null together with its output
    float *records_out, *raw_out, *m_out, *v_out;
    uint32_t max_out;
    SplatScan scan;                   // K = 2: kept, dropped; offsets[g] = the output row of a kept g
};
void launch_prune_below(const PruneArgs& a, uint32_t* counts_out, hipStream_t stream);
// gs_relocate_device / gs_grow_device / gs_position_noise_device (gs_mcmc.hip).  The sampler's scratch for n splats, in blocks
// of 256 splats: w(g) is never stored, P(g) = block_prefix[g / 256] + within[g]
constexpr uint32_t kMcmcMaxRatio = 51;          // r = min(cnt + 1, kMcmcMaxRatio)
constexpr uint32_t kMcmcTableFloats = kMcmcMaxRatio * kMcmcMaxRatio + kMcmcMaxRatio;    // B[51][51], then Q[51]
constexpr uint32_t kMcmcAlive = 0xFFFFFFFFu, kMcmcDeadNoDraw = 0xFFFFFFFEu;             // McmcScratch::src_of of a row that is no copy
struct McmcScratch {
    uint32_t* within;         // [n]  the exclusive sum of w inside the splat's block (at most 255 * 2^24)
    uint64_t* block_sums;     // [ceil(n / 256)]
    uint64_t* block_prefix;   // [ceil(n / 256) + 1]  exclusive scan of block_sums; the last entry is `total`
    uint32_t* cnt;            // [n]  draws that chose g
    uint32_t* src_of;         // [n]  gs_relocate_device: src(d) of a dead d that drew, kMcmcDeadNoDraw of a dead d with
                              //      total == 0, kMcmcAlive of an alive g
    float* tables;            // [kMcmcTableFloats]  B and Q of the header, made on the host (mcmc_fill_tables)
};
void mcmc_fill_tables(float* host_tables);      // kMcmcTableFloats floats
struct McmcArgs {
    float *records, *raw, *m, *v;     // raw: null or given; m, v: both null or neither
    uint32_t n;
    float min_opacity;
    uint64_t seed;
    McmcScratch s;
    SplatScan scan;                   // relocate K = 3: changed, dead, sources; grow K = 2: outputs, sources
};
// ids_out: the changed rows below max_rows, ascending; counts_out[3] = {changed, dead, sources}
void launch_relocate(const McmcArgs& a, uint32_t* ids_out, uint32_t max_rows, uint32_t* counts_out, hipStream_t stream);
// a.records / raw / m / v are only read; counts_out[2] = {outputs, sources}
void launch_grow(const McmcArgs& a, uint32_t n_add, float* records_out, float* raw_out, float* m_out, float* v_out,
                 uint32_t max_out, uint32_t* counts_out, hipStream_t stream);
// ids == null: every g < n (count and max_rows unused)
void launch_position_noise(float* records, float* raw, uint32_t n, const uint32_t* ids, const uint32_t* count, uint32_t max_rows,
                           float scale, float gate_k, float gate_x0, uint64_t seed, hipStream_t stream);
// gs_rows_accumulate_device / gs_rows_collect_device (gs_batch.hip).  _accumulate: acc[ids[i]] (+)= weight * grad_rows[i] on the
// fields, then mark[ids[i]] += 1, i < min(*count, max_rows); max_rows == 0 launches nothing.  _collect: the splats with a
// non-zero mark, ascending, into ids_out / rows_out (both may be null with max_rows == 0) below max_rows, their number into
// count_out, mark cleared; scan: K >= 2 rows for at least n splats.
void launch_rows_accumulate(float* acc, uint32_t* mark, uint32_t n, const uint32_t* ids, const float* grad_rows,
                            const uint32_t* count, uint32_t max_rows, float weight, hipStream_t stream);
void launch_rows_collect(const float* acc, uint32_t* mark, uint32_t n, const SplatScan& scan, uint32_t* ids_out,
                         float* rows_out, uint32_t max_rows, uint32_t* count_out, hipStream_t stream);
// gs_knn_mean_dist2_device / gs_records_from_points_device (gs_init.hip): the context's scratch for n points, beside a
// SortBuffers of capacity n (code, 0, input index)
constexpr uint32_t kInitBoundBlocks = 256;      // partial boxes of the bounds reduction: a fixed shape
struct InitScratch {
    float* partial;           // [kInitBoundBlocks][6]  min xyz, max xyz
    float* bounds;            // [6]  of the flipped positions, from the loader's start values
    float4* sorted;           // [n]  flipped positions in sorted order, w = 0
    float4* boxes;            // [ceil(n / 64)][2]  min, max of every 64 consecutive sorted positions
    float* dist2;             // [n]  mean squared distance in sorted order (the row writer's input)
    uint32_t* probe;          // null, or (a GS_INIT_PROBE build) [ceil(n / 64)][2] surviving boxes per wave: coarse, per lane
};
// Both enqueue bounds, codes, the sort of `run` over sb and the gather, then the search (and the rows); they return the
// ping-pong half of sb that holds the sorted ids, or -1 with nothing of the search enqueued when sb cannot serve the run.
int launch_knn_mean_dist2(const float* points, uint32_t n, const InitScratch& s, const SortBuffers& sb, const SortRun& run,
                          float* dist2_out, hipStream_t stream);
int launch_records_from_points(const float* points, const float* colors, uint32_t n, const InitScratch& s, const SortBuffers& sb,
                               const SortRun& run, float opacity, float min_dist2, float max_scale, float* records_out,
                               uint32_t* order_out, hipStream_t stream);
#ifdef GS_INIT_PROBE
hipError_t init_probe_ms(float ms[6]);      // a tuning build: milliseconds of the six launches of the last, completed call
#endif
void launch_stream_probe(int kind, const void* src, void* dst, size_t bytes, uint32_t blocks, hipStream_t stream);
// helpers for the stand-alone sorter entry points
void launch_set_sort_params(SortParams* params, uint32_t* coarse, uint32_t n, hipStream_t stream);
void launch_fill_random_keys(uint32_t* lo, uint32_t* hi, uint32_t* id, uint32_t n,
                             uint32_t num_tiles, uint64_t seed, hipStream_t stream);
void launch_check_sorted(const uint32_t* lo, const uint32_t* hi, uint32_t n, uint32_t* bad_count,
                         hipStream_t stream);

} // namespace gs
