// gs_init.hip -- a cloud from points (gs_knn_mean_dist2_device, gs_records_from_points_device; no reference counterpart): the
// loader's Morton order restated on the device (gs_ply.cpp, sweep 1), an exact 3-nearest-neighbour search over the points
// in that order, and the records gs_load_ply would make of the .ply an INRIA trainer writes at iteration 0.
//
// The search is exact and a function of the multiset of squared distances alone: every pruning bound is computed in the
// shape of the distance itself -- per axis a gap that float subtraction, being monotone, cannot make larger than the
// |difference| of any member of the box, then (ex * ex + ey * ey) + ez * ez, monotone again -- so a box is dropped only when
// no member can enter the three best.  No atomics, no waiting: a wave owns its 64 query points from start to end.
#include "gs_internal.h"
#include "gs_device_utils.h"

#include <cfloat>

namespace gs {

namespace {

constexpr float kPosInf = __builtin_huge_valf();

// ResourceManager.cpp:231-236: the record's position of a .ply point
__device__ __forceinline__ float3 flipped(const float* __restrict__ points, size_t i) {
    return make_float3(points[i * 3] * -1.0f, points[i * 3 + 1] * -1.0f, points[i * 3 + 2]);
}

// SMath.h:10-18 (morton_part_by2 of gs_ply.cpp)
__device__ __forceinline__ uint32_t part_by2(uint32_t x) {
    x &= 0x000003ffu;
    x = (x ^ (x << 16)) & 0xff0000ffu;
    x = (x ^ (x << 8)) & 0x0300f00fu;
    x = (x ^ (x << 4)) & 0x030c30c3u;
    x = (x ^ (x << 2)) & 0x09249249u;
    return x;
}

// min of v[0..2], max of v[3..5] over the workgroup's 256 threads -> thread 0
__device__ __forceinline__ void block_min_max(float (&v)[6]) {
    __shared__ float part[4][6];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = fminf(v[k], __shfl_xor(v[k], off, 64));
#pragma unroll
        for (int k = 3; k < 6; ++k) v[k] = fmaxf(v[k], __shfl_xor(v[k], off, 64));
    }
    if (lane_id() == 0)
        for (int k = 0; k < 6; ++k) part[wave_id()][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; ++w) {
            for (int k = 0; k < 3; ++k) v[k] = fminf(v[k], part[w][k]);
            for (int k = 3; k < 6; ++k) v[k] = fmaxf(v[k], part[w][k]);
        }
}

// Bounds, launch 1: kInitBoundBlocks partial boxes.  Every thread starts where the loader starts (gs_ply.cpp:246: FLT_MAX and
// the smallest positive float, as written there); both are idempotent under min / max, so the result is the loader's.
__global__ __launch_bounds__(256) void k_init_bounds(const float* __restrict__ points, uint32_t n, float* __restrict__ partial) {
    float v[6] = {FLT_MAX, FLT_MAX, FLT_MAX, FLT_MIN, FLT_MIN, FLT_MIN};
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += kInitBoundBlocks * 256u) {
        const float3 p = flipped(points, i);
        v[0] = fminf(v[0], p.x); v[1] = fminf(v[1], p.y); v[2] = fminf(v[2], p.z);
        v[3] = fmaxf(v[3], p.x); v[4] = fmaxf(v[4], p.y); v[5] = fmaxf(v[5], p.z);
    }
    block_min_max(v);
    if (threadIdx.x == 0)
        for (int k = 0; k < 6; ++k) partial[blockIdx.x * 6u + k] = v[k];
}

// Bounds, launch 2: one workgroup, a partial box per thread
__global__ __launch_bounds__(256) void k_init_bounds_final(const float* __restrict__ partial, float* __restrict__ bounds) {
    static_assert(kInitBoundBlocks == 256u, "one partial box per thread");
    float v[6];
    for (int k = 0; k < 6; ++k) v[k] = partial[threadIdx.x * 6u + k];
    block_min_max(v);
    if (threadIdx.x == 0)
        for (int k = 0; k < 6; ++k) bounds[k] = v[k];
}

// Codes (gs_ply.cpp:252-258) and the identity list: the sort's lo word = code, hi word = 0, id = the input index
__global__ __launch_bounds__(256) void k_init_codes(const float* __restrict__ points, uint32_t n, const float* __restrict__ bounds,
                                                     uint32_t* __restrict__ lo, uint32_t* __restrict__ hi, uint32_t* __restrict__ id) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float3 p = flipped(points, i);
    const float pos[3] = {p.x, p.y, p.z};
    uint32_t q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float delta = bounds[3 + a] - bounds[a];
        q[a] = f2u_sat((pos[a] - bounds[a]) / delta * 1023.0f);     // a flat axis: 0 / 0 = NaN -> 0
    }
    lo[i] = (part_by2(q[2]) << 2) + (part_by2(q[1]) << 1) + part_by2(q[0]);
    hi[i] = 0u;
    id[i] = i;
}

// Gather: the flipped positions in sorted order (one 16-byte record each, so the search reads contiguously), and the box
// of every 64 consecutive ones: boxes[2 b] = min xyz, boxes[2 b + 1] = max xyz over the points the box really holds
__global__ __launch_bounds__(256) void k_init_gather(const float* __restrict__ points, const uint32_t* __restrict__ sorted_id,
                                                      uint32_t n, float4* __restrict__ sorted, float4* __restrict__ boxes) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const bool ok = k < n;
    float3 p = make_float3(0.0f, 0.0f, 0.0f);
    if (ok) {
        p = flipped(points, sorted_id[k]);
        sorted[k] = make_float4(p.x, p.y, p.z, 0.0f);
    }
    float v[6] = {ok ? p.x : kPosInf, ok ? p.y : kPosInf, ok ? p.z : kPosInf, ok ? p.x : -kPosInf, ok ? p.y : -kPosInf, ok ? p.z : -kPosInf};
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) v[a] = fminf(v[a], __shfl_xor(v[a], off, 64));
#pragma unroll
        for (int a = 3; a < 6; ++a) v[a] = fmaxf(v[a], __shfl_xor(v[a], off, 64));
    }
    if (lane_id() == 0 && (k & ~63u) < n) {
        boxes[(size_t)(k >> 6) * 2] = make_float4(v[0], v[1], v[2], 0.0f);
        boxes[(size_t)(k >> 6) * 2 + 1] = make_float4(v[3], v[4], v[5], 0.0f);
    }
}

// the squared distance, in the one shape every caller and every bound uses (the build never contracts)
__device__ __forceinline__ float dist2_of(const float4& p, const float4& q) {
    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    return (dx * dx + dy * dy) + dz * dz;
}
__device__ __forceinline__ float gap2_of(float ex, float ey, float ez) { return (ex * ex + ey * ey) + ez * ez; }

// d into the three smallest a <= b <= c
__device__ __forceinline__ void keep_three(float& a, float& b, float& c, float d) {
    const float nc = fminf(c, fmaxf(b, d)), nb = fminf(b, fmaxf(a, d));
    a = fminf(a, d); b = nb; c = nc;
}

// the largest x of the wave, every x >= +0 (or +inf): such floats order like their bits.  All 64 lanes active.
__device__ __forceinline__ float wave_max_nonneg(float x) {
    return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_max(__float_as_uint(x)), 63));
}

// Search: a wave per 64 consecutive sorted points (its query box), four independent waves per workgroup; lane = point, its
// three best in registers.  Seeded from the wave's own 64 points; then all boxes, 64 per round: lane l tests box b0 + l
// against the query box with the wave's largest third-best, and for every survivor each lane tests ITS point against the
// box with ITS third-best -- a wave across a Morton seam has a huge query box, and only this test prunes for it.  A box some
// lane still wants is staged in the wave's LDS and read back by broadcast.  Every loop is bounded by the box count or 64.
// out[BY_INPUT ? sorted_id[k] : k] = ((a + b) + c) / 3 of sorted point k.
// PROBE (tools/init_cost.py, a tuning build): probe[2 q], probe[2 q + 1] = the boxes that survived the coarse and the
// per-lane test of wave q.
template <bool BY_INPUT, bool PROBE>
__global__ __launch_bounds__(256) void k_init_search(const float4* __restrict__ sorted, const float4* __restrict__ boxes,
                                                      const uint32_t* __restrict__ sorted_id, uint32_t n, float* __restrict__ out,
                                                      uint32_t* __restrict__ probe) {
    __shared__ float4 stage[4][64];
    const uint32_t num_boxes = (n + 63u) / 64u;
    const uint32_t lane = lane_id(), qb = blockIdx.x * 4u + wave_id();
    if (qb >= num_boxes) return;                                  // the whole wave; there is no workgroup barrier below
    float4* const mine = stage[wave_id()];
    const uint32_t k = qb * 64u + lane;
    const bool valid = k < n;
    const float4 p = valid ? sorted[k] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float a = kPosInf, b = kPosInf, c = kPosInf;

    // the wave's own points: every other index counts, a duplicate position included
    const uint32_t own = n - qb * 64u < 64u ? n - qb * 64u : 64u;
    mine[lane] = p;
    __builtin_amdgcn_wave_barrier();
    for (uint32_t j = 0; j < own; ++j) {
        const float d = dist2_of(p, mine[j]);
        if (j != lane) keep_three(a, b, c, d);
    }
    const float4 qlo = boxes[(size_t)qb * 2], qhi = boxes[(size_t)qb * 2 + 1];

    uint32_t coarse_kept = 0, lane_kept = 0;
    for (uint32_t b0 = 0; b0 < num_boxes; b0 += 64u) {
        const float worst = wave_max_nonneg(valid ? c : 0.0f);
        const uint32_t bl = b0 + lane;
        bool keep = false;
        if (bl < num_boxes && bl != qb) {
            const float4 lo = boxes[(size_t)bl * 2], hi = boxes[(size_t)bl * 2 + 1];
            const float ex = fmaxf(fmaxf(lo.x - qhi.x, qlo.x - hi.x), 0.0f);
            const float ey = fmaxf(fmaxf(lo.y - qhi.y, qlo.y - hi.y), 0.0f);
            const float ez = fmaxf(fmaxf(lo.z - qhi.z, qlo.z - hi.z), 0.0f);
            keep = !(gap2_of(ex, ey, ez) > worst);
        }
        uint64_t todo = __ballot(keep);
        if (PROBE) coarse_kept += (uint32_t)__popcll(todo);
        while (todo) {
            const uint32_t bj = b0 + (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1ull;
            const float4 lo = boxes[(size_t)bj * 2], hi = boxes[(size_t)bj * 2 + 1];      // one address for the wave
            const float ex = fmaxf(fmaxf(lo.x - p.x, p.x - hi.x), 0.0f);
            const float ey = fmaxf(fmaxf(lo.y - p.y, p.y - hi.y), 0.0f);
            const float ez = fmaxf(fmaxf(lo.z - p.z, p.z - hi.z), 0.0f);
            const bool wants = valid && !(gap2_of(ex, ey, ez) > c);
            if (__ballot(wants) == 0ull) continue;
            if (PROBE) ++lane_kept;
            const uint32_t first = bj * 64u, members = n - first < 64u ? n - first : 64u;
            __builtin_amdgcn_wave_barrier();                      // the reads of the box before are done
            if (lane < members) mine[lane] = sorted[first + lane];
            __builtin_amdgcn_wave_barrier();
            for (uint32_t j = 0; j < members; ++j) {
                const float d = dist2_of(p, mine[j]);
                if (wants) keep_three(a, b, c, d);
            }
        }
    }
    if (valid) out[BY_INPUT ? sorted_id[k] : k] = ((a + b) + c) / 3.0f;
    if (PROBE && lane == 0) { probe[(size_t)qb * 2] = coarse_kept; probe[(size_t)qb * 2 + 1] = lane_kept; }
}

// Rows: a thread per float of the output.  Row k is input point sorted_id[k]; its position is sorted[k].  The rotation is
// what convert_row (gs_ply.cpp) makes of rot_0..3 = (1, 0, 0, 0): inv = 1, (-r2, -r3, r0, -r1) = (-0, -0, 1, -0).
__global__ __launch_bounds__(256) void k_init_rows(const float4* __restrict__ sorted, const uint32_t* __restrict__ sorted_id,
                                                    const float* __restrict__ dist2, const float* __restrict__ colors, uint32_t n,
                                                    float opacity, float min_dist2, float max_scale, float* __restrict__ records,
                                                    uint32_t* __restrict__ order) {
    const size_t at = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (at >= (size_t)n * kRecordFloats) return;
    const uint32_t k = (uint32_t)(at / kRecordFloats), col = (uint32_t)(at % kRecordFloats);
    float v = 0.0f;
    if (col < 3u) {
        const float4 p = sorted[k];
        v = col == 0u ? p.x : (col == 1u ? p.y : p.z);
        if (col == 0u && order) order[k] = sorted_id[k];
    } else if (col >= kRecScale && col < kRecScale + 3u) {
        const float d2 = dist2[k], d = d2 < min_dist2 ? min_dist2 : d2;
        const float s = sqrtf(d);
        v = s > max_scale ? max_scale : s;
    } else if (col >= kRecRot && col < kRecRot + 4u) {
        v = col == kRecRot + 2u ? 1.0f : -0.0f;
    } else if (col >= 12u && col < 15u) {
        if (colors) v = (colors[(size_t)sorted_id[k] * 3 + (col - 12u)] - 0.5f) / 0.28209479177387814f;
    } else if (col == kRecOpacity) {
        v = opacity;
    }
    records[at] = v;
}

// A GS_INIT_PROBE build (tools/init_cost.py) brackets the six launches of a call with events: bounds, codes, sort, gather +
// boxes, search, rows.  The product build records nothing.
#ifdef GS_INIT_PROBE
hipEvent_t g_marks[7];
bool g_marks_made = false;
void mark(int k, hipStream_t stream) {
    if (!g_marks_made) {
        for (hipEvent_t& e : g_marks) (void)hipEventCreate(&e);
        g_marks_made = true;
    }
    (void)hipEventRecord(g_marks[k], stream);
}
#else
inline void mark(int, hipStream_t) {}
#endif

// what both calls share: bounds, codes, sort, gather + boxes -> the ping-pong half that holds the sorted list (< 0: the
// sorter refused)
int enqueue_order(const float* points, uint32_t n, const InitScratch& s, const SortBuffers& sb, const SortRun& run, hipStream_t stream) {
    const uint32_t blocks = (n + 255u) / 256u;
    mark(0, stream);
    hipLaunchKernelGGL(k_init_bounds, dim3(kInitBoundBlocks), dim3(256), 0, stream, points, n, s.partial);
    hipLaunchKernelGGL(k_init_bounds_final, dim3(1), dim3(256), 0, stream, s.partial, s.bounds);
    mark(1, stream);
    hipLaunchKernelGGL(k_init_codes, dim3(blocks), dim3(256), 0, stream, points, n, s.bounds, sb.lo[0], sb.hi[0], sb.id[0]);
    mark(2, stream);
    launch_set_sort_params(sb.params, sb.coarse, n, stream);
    const int si = launch_radix_sort(sb, run, stream);
    if (si < 0) return si;
    mark(3, stream);
    hipLaunchKernelGGL(k_init_gather, dim3(blocks), dim3(256), 0, stream, points, sb.id[si], n, s.sorted, s.boxes);
    mark(4, stream);
    return si;
}

template <bool BY_INPUT>
void enqueue_search(const InitScratch& s, const uint32_t* sorted_id, uint32_t n, float* out, hipStream_t stream) {
    const uint32_t waves = (n + 63u) / 64u;
#ifdef GS_INIT_PROBE
    hipLaunchKernelGGL((k_init_search<BY_INPUT, true>), dim3((waves + 3u) / 4u), dim3(256), 0, stream, s.sorted, s.boxes, sorted_id, n, out, s.probe);
#else
    hipLaunchKernelGGL((k_init_search<BY_INPUT, false>), dim3((waves + 3u) / 4u), dim3(256), 0, stream, s.sorted, s.boxes, sorted_id, n, out, s.probe);
#endif
}

} // namespace

int launch_knn_mean_dist2(const float* points, uint32_t n, const InitScratch& s, const SortBuffers& sb, const SortRun& run,
                          float* dist2_out, hipStream_t stream) {
    const int si = enqueue_order(points, n, s, sb, run, stream);
    if (si < 0) return si;
    enqueue_search<true>(s, sb.id[si], n, dist2_out, stream);
    mark(5, stream);
    mark(6, stream);
    return si;
}

int launch_records_from_points(const float* points, const float* colors, uint32_t n, const InitScratch& s, const SortBuffers& sb,
                               const SortRun& run, float opacity, float min_dist2, float max_scale, float* records_out,
                               uint32_t* order_out, hipStream_t stream) {
    const int si = enqueue_order(points, n, s, sb, run, stream);
    if (si < 0) return si;
    enqueue_search<false>(s, sb.id[si], n, s.dist2, stream);
    mark(5, stream);
    const size_t floats = (size_t)n * kRecordFloats;
    hipLaunchKernelGGL(k_init_rows, dim3((uint32_t)((floats + 255u) / 256u)), dim3(256), 0, stream, s.sorted, sb.id[si], s.dist2,
                       colors, n, opacity, min_dist2, max_scale, records_out, order_out);
    mark(6, stream);
    return si;
}

#ifdef GS_INIT_PROBE
// milliseconds of the six launches of the last call (it must have completed)
hipError_t init_probe_ms(float ms[6]) {
    for (int k = 0; k < 6; ++k) {
        const hipError_t e = g_marks_made ? hipEventElapsedTime(&ms[k], g_marks[k], g_marks[k + 1]) : hipErrorNotReady;
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
#endif

} // namespace gs
