// gs_raw.hip -- the "raw" parameter space of include/gsplat.h (log-scale, logit-opacity, rotation before normalisation: what
// a .ply stores and the INRIA trainer optimises) next to the record space the frame reads: gs_adam_rows_raw_device,
// gs_records_from_raw_device, gs_raw_from_records_device, gs_reset_opacity_raw_device.  No reference counterpart.  All four
// are bandwidth-bound and touch nothing but the 59 fields of a row (gs_record.h); every kernel runs a lane per (row, group of
// four floats), like k_adam_rows, so the scale's three and the rotation's four components sit in one lane.
#include "../../include/gsplat.h"
#include "gs_adam_field.h"
#include "gs_splat_math.h"

namespace gs {

namespace {

struct Quad {
    float3 p;
    float w;      // only where has_w
};
__device__ __forceinline__ Quad load_quad(const float* __restrict__ a, size_t at, bool has_w) {
    Quad q;
    q.p = *reinterpret_cast<const float3*>(a + at);
    q.w = has_w ? a[at + 3] : 0.0f;
    return q;
}
__device__ __forceinline__ void store_quad(float* __restrict__ a, size_t at, bool has_w, const Quad& q) {
    *reinterpret_cast<float3*>(a + at) = q.p;
    if (has_w) a[at + 3] = q.w;
}

}  // namespace

// k_adam_rows (gs_adam.hip) with the chain in front and act() behind: per listed row the gradient row is read, the fields of
// raw, m and v are read and written, the record's scale, rotation and opacity are read (the values the frame rasterised)
// and the record's fields are written.
__global__ __launch_bounds__(256) void k_adam_rows_raw(float* __restrict__ raw, float* __restrict__ records,
                                                       float* __restrict__ m, float* __restrict__ v, uint32_t n,
                                                       const uint32_t* __restrict__ ids, const float* __restrict__ grad_rows,
                                                       const uint32_t* __restrict__ count, uint32_t max_rows, AdamStep a) {
    const uint32_t listed = *count, rows = listed < max_rows ? listed : max_rows;
    const uint64_t first = (uint64_t)blockIdx.x * 256u;
    if (first / kRecFieldQuads >= rows) return;                   // the whole block is past the count
    const uint64_t item = first + threadIdx.x;
    const uint32_t row = (uint32_t)(item / kRecFieldQuads), quad = (uint32_t)(item % kRecFieldQuads);
    if (row >= rows) return;
    const uint32_t id = ids[row];
    if (id >= n) return;
    const size_t at = (size_t)id * kRecordFloats + quad * 4u, gat = (size_t)row * kRecordFloats + quad * 4u;
    const uint32_t g3 = quad < 4u ? quad : (uint32_t)GS_ADAM_SH_REST;    // groups 0..3 are POSITION, SCALE, ROTATION, SH_DC
    const bool has_w = rec_is_field(quad * 4u + 3u);
    const uint32_t gw = quad == kQuadRot ? (uint32_t)GS_ADAM_ROTATION : (uint32_t)GS_ADAM_OPACITY;

    Quad g = load_quad(grad_rows, gat, has_w);
    Quad p = load_quad(raw, at, has_w), mm = load_quad(m, at, has_w), vv = load_quad(v, at, has_w);

    // dL/d(raw) from dL/d(record) and the record's current values
    if (quad == kQuadScale) {
        const float3 s = *reinterpret_cast<const float3*>(records + at);
        g.p.x = g.p.x * s.x; g.p.y = g.p.y * s.y; g.p.z = g.p.z * s.z;
    } else if (quad == kQuadRot) {
        const Quad q = load_quad(records, at, true);
        const float inv = inv_length4(p.p.x, p.p.y, p.p.z, p.w);        // of the OLD raw rotation
        const float d = (g.p.x * q.p.x + g.p.y * q.p.y) + (g.p.z * q.p.z + g.w * q.w);
        g.p.x = (g.p.x - q.p.x * d) * inv; g.p.y = (g.p.y - q.p.y * d) * inv;
        g.p.z = (g.p.z - q.p.z * d) * inv; g.w = (g.w - q.w * d) * inv;
    } else if (quad == kQuadDc) {
        const float o = records[at + 3];
        g.w = (g.w * o) * (1.0f - o);
    }

    const float step = pick(a.step, g3), lo = pick(a.lo, g3), hi = pick(a.hi, g3);
    adam_field(p.p.x, mm.p.x, vv.p.x, g.p.x, a, step, lo, hi);
    adam_field(p.p.y, mm.p.y, vv.p.y, g.p.y, a, step, lo, hi);
    adam_field(p.p.z, mm.p.z, vv.p.z, g.p.z, a, step, lo, hi);
    if (has_w) adam_field(p.w, mm.w, vv.w, g.w, a, pick(a.step, gw), pick(a.lo, gw), pick(a.hi, gw));
    store_quad(raw, at, has_w, p);
    store_quad(m, at, has_w, mm);
    store_quad(v, at, has_w, vv);
    act_quad(quad, p.p, p.w);
    store_quad(records, at, has_w, p);
}

// dst = act(src) (to_raw == false) or its inverse (to_raw == true) on the fields of all n rows
template <bool to_raw>
__global__ __launch_bounds__(256) void k_convert_space(const float* __restrict__ src, float* __restrict__ dst, uint32_t n) {
    const uint64_t item = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t row = item / kRecFieldQuads;
    const uint32_t quad = (uint32_t)(item % kRecFieldQuads);
    if (row >= n) return;
    const size_t at = (size_t)row * kRecordFloats + quad * 4u;
    const bool has_w = rec_is_field(quad * 4u + 3u);
    Quad q = load_quad(src, at, has_w);
    if (to_raw) {
        if (quad == kQuadScale) { q.p.x = log_scale(q.p.x); q.p.y = log_scale(q.p.y); q.p.z = log_scale(q.p.z); }
        else if (quad == kQuadDc) q.w = logit_opacity(q.w);
    } else {
        act_quad(quad, q.p, q.w);
    }
    store_quad(dst, at, has_w, q);
}

// a lane per row: float 15 of raw, records, m and v (m == nullptr: without the moments)
__global__ __launch_bounds__(256) void k_reset_opacity_raw(float* __restrict__ raw, float* __restrict__ records,
                                                           float* __restrict__ m, float* __restrict__ v, uint32_t n,
                                                           float max_opacity, float logit) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (g >= n) return;
    const size_t at = (size_t)g * kRecordFloats + kRecOpacity;
    if (m) { m[at] = 0.0f; v[at] = 0.0f; }
    if (records[at] > max_opacity) {
        raw[at] = logit;
        records[at] = sigmoid_pinned(logit);
    }
}

void launch_adam_rows_raw(float* raw, float* records, float* m, float* v, uint32_t n, const uint32_t* ids,
                          const float* grad_rows, const uint32_t* count, uint32_t max_rows, const AdamStep& a,
                          hipStream_t stream) {
    if (max_rows == 0) return;
    const uint64_t blocks = ((uint64_t)max_rows * kRecFieldQuads + 255u) / 256u;  // < 2^29 for every uint32 max_rows
    hipLaunchKernelGGL(k_adam_rows_raw, dim3((uint32_t)blocks), dim3(256), 0, stream, raw, records, m, v, n, ids, grad_rows,
                       count, max_rows, a);
}

void launch_convert_space(const float* src, float* dst, uint32_t n, bool to_raw, hipStream_t stream) {
    if (n == 0) return;
    const uint64_t blocks = ((uint64_t)n * kRecFieldQuads + 255u) / 256u;         // < 2^29
    if (to_raw) hipLaunchKernelGGL(k_convert_space<true>, dim3((uint32_t)blocks), dim3(256), 0, stream, src, dst, n);
    else hipLaunchKernelGGL(k_convert_space<false>, dim3((uint32_t)blocks), dim3(256), 0, stream, src, dst, n);
}

void launch_reset_opacity_raw(float* raw, float* records, float* m, float* v, uint32_t n, float max_opacity, float logit,
                              hipStream_t stream) {
    if (n == 0) return;
    const uint64_t blocks = ((uint64_t)n + 255u) / 256u;
    hipLaunchKernelGGL(k_reset_opacity_raw, dim3((uint32_t)blocks), dim3(256), 0, stream, raw, records, m, v, n, max_opacity,
                       logit);
}

}  // namespace gs
