// gs_adam.hip -- gs_adam_rows_device (include/gsplat.h): torch.optim.SparseAdam's rule on the rows gs_backward_visible*
// lists, on the caller's own records and moments.  No reference counterpart.  Bandwidth-bound: per listed row one
// gradient row is read and the row's 59 fields of records, m and v are read and written (7 x 236 bytes; the other 25
// floats of a row are never touched, so nothing wider than the fields is loaded or stored).
#include "../../include/gsplat.h"
#include "gs_adam_field.h"
#include "gs_device_utils.h"
#include "gs_internal.h"

namespace gs {

// A lane per (listed row, group of four floats): the lanes of a row read 304 consecutive bytes of the gradient row and of
// the three rows of splat ids[row], ascending.  x, y, z of a group are fields of one GS_ADAM_* group in every group; w is a
// field in groups 2 (rotation) and 3 (opacity) only.
__global__ __launch_bounds__(256) void k_adam_rows(float* __restrict__ records, float* __restrict__ m, float* __restrict__ v,
                                                   uint32_t n, const uint32_t* __restrict__ ids,
                                                   const float* __restrict__ grad_rows, const uint32_t* __restrict__ count,
                                                   uint32_t max_rows, AdamStep a) {
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
    const uint32_t gw = quad == kRecRot / 4u ? (uint32_t)GS_ADAM_ROTATION : (uint32_t)GS_ADAM_OPACITY;

    const float3 g = *reinterpret_cast<const float3*>(grad_rows + gat);
    float3 p = *reinterpret_cast<const float3*>(records + at);
    float3 mm = *reinterpret_cast<const float3*>(m + at);
    float3 vv = *reinterpret_cast<const float3*>(v + at);
    float gw_ = 0.0f, pw = 0.0f, mw = 0.0f, vw = 0.0f;
    if (has_w) { gw_ = grad_rows[gat + 3]; pw = records[at + 3]; mw = m[at + 3]; vw = v[at + 3]; }

    const float step = pick(a.step, g3), lo = pick(a.lo, g3), hi = pick(a.hi, g3);
    adam_field(p.x, mm.x, vv.x, g.x, a, step, lo, hi);
    adam_field(p.y, mm.y, vv.y, g.y, a, step, lo, hi);
    adam_field(p.z, mm.z, vv.z, g.z, a, step, lo, hi);
    *reinterpret_cast<float3*>(records + at) = p;
    *reinterpret_cast<float3*>(m + at) = mm;
    *reinterpret_cast<float3*>(v + at) = vv;
    if (has_w) {
        adam_field(pw, mw, vw, gw_, a, pick(a.step, gw), pick(a.lo, gw), pick(a.hi, gw));
        records[at + 3] = pw; m[at + 3] = mw; v[at + 3] = vw;
    }
}

void launch_adam_rows(float* records, float* m, float* v, uint32_t n, const uint32_t* ids, const float* grad_rows,
                      const uint32_t* count, uint32_t max_rows, const AdamStep& a, hipStream_t stream) {
    if (max_rows == 0) return;
    const uint64_t blocks = ((uint64_t)max_rows * kRecFieldQuads + 255u) / 256u;  // < 2^29 for every uint32 max_rows
    hipLaunchKernelGGL(k_adam_rows, dim3((uint32_t)blocks), dim3(256), 0, stream, records, m, v, n, ids, grad_rows, count,
                       max_rows, a);
}

}  // namespace gs
