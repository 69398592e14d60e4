// gs_batch.hip -- several views per optimiser step (include/gsplat.h, no reference counterpart):
//   gs_rows_accumulate_device : the listed gradient rows of one frame, times a weight, summed into the caller's accumulator
//                   acc[n][84], with a touch count per splat in mark[n].  Two launches: k_rows_accumulate (the sums) and
//                   k_rows_mark (the counts);
//   gs_rows_collect_device    : the touched rows of the accumulator as one ascending (ids, rows, count) list, and mark cleared
//                   for the next batch.  The per-splat scan of gs_splat_scan.h over CollectSource (three launches) gives the
//                   position of every touched splat and their number; k_rows_gather writes the rows.
// Both are bandwidth-bound: the accumulate reads a gradient row's 59 fields and reads and writes those of acc (3 x 236 bytes
// per listed row, 2 x 236 on a first touch) plus 8 bytes of id and mark; the collect reads mark twice and clears it (12 bytes
// per splat) and moves 236 + 336 bytes per output row.  No atomics: ids are distinct within a list and the lists of a batch
// follow each other on one stream, so the sums are bitwise reproducible.  Built with contraction off (the Makefile's
// -ffp-contract=off): weight * row is rounded before it is added.
#include "gs_splat_scan.h"

namespace gs {

// ---- accumulate ---------------------------------------------------------------------------------------------------

// A lane per (listed row, group of four floats), the mapping of k_adam_rows: the lanes of a row read 304 consecutive bytes of
// the gradient row and of acc[ids[row]].  x, y, z of a group are fields in every group, w in groups 2 (rotation) and 3
// (opacity) only, so nothing wider than the fields is loaded or stored.
// Race-free by construction: the 19 lanes of a row may lie in two waves or two blocks, and all of them must see the mark as
// it was before this list.  This kernel only READS mark, nothing in this launch writes it; the increment is k_rows_mark, a
// launch of its own behind this one on the same stream.  acc[g] is written by the lanes of the one row that lists g (ids are
// distinct), each lane its own floats.
// (Four items per lane, their loads issued level by level, were measured beside this form and were no faster: DESIGN.md
// section 8.)
__global__ __launch_bounds__(256) void k_rows_accumulate(float* __restrict__ acc, const uint32_t* __restrict__ mark, uint32_t n,
                                                         const uint32_t* __restrict__ ids,
                                                         const float* __restrict__ grad_rows,
                                                         const uint32_t* __restrict__ count, uint32_t max_rows, float weight) {
    const uint32_t listed = *count, rows = listed < max_rows ? listed : max_rows;
    const uint64_t first = (uint64_t)blockIdx.x * 256u;
    if (first / kRecFieldQuads >= rows) return;                   // the whole block is past the count
    const uint64_t item = first + threadIdx.x;
    const uint32_t row = (uint32_t)(item / kRecFieldQuads), quad = (uint32_t)(item % kRecFieldQuads);
    if (row >= rows) return;
    const uint32_t id = ids[row];
    if (id >= n) return;
    const size_t at = (size_t)id * kRecordFloats + quad * 4u, gat = (size_t)row * kRecordFloats + quad * 4u;
    const bool has_w = rec_is_field(quad * 4u + 3u);
    const bool first_touch = mark[id] == 0u;

    const float3 g = *reinterpret_cast<const float3*>(grad_rows + gat);
    float3 s = make_float3(weight * g.x, weight * g.y, weight * g.z);
    float sw = has_w ? weight * grad_rows[gat + 3] : 0.0f;
    if (!first_touch) {                                           // a first touch is a store: acc needs no initialisation
        const float3 a = *reinterpret_cast<const float3*>(acc + at);
        s = make_float3(a.x + s.x, a.y + s.y, a.z + s.z);
        if (has_w) sw = acc[at + 3] + sw;
    }
    *reinterpret_cast<float3*>(acc + at) = s;
    if (has_w) acc[at + 3] = sw;
}

// mark[ids[i]] += 1 for the rows k_rows_accumulate has just summed: a lane per listed row
__global__ __launch_bounds__(256) void k_rows_mark(uint32_t* __restrict__ mark, uint32_t n, const uint32_t* __restrict__ ids,
                                                   const uint32_t* __restrict__ count, uint32_t max_rows) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t listed = *count, rows = listed < max_rows ? listed : max_rows;
    if (i >= rows) return;
    const uint32_t g = ids[i];
    if (g >= n) return;
    mark[g] += 1u;
}

void launch_rows_accumulate(float* acc, uint32_t* mark, uint32_t n, const uint32_t* ids, const float* grad_rows,
                            const uint32_t* count, uint32_t max_rows, float weight, hipStream_t stream) {
    if (max_rows == 0) return;
    const uint64_t blocks = ((uint64_t)max_rows * kRecFieldQuads + 255u) / 256u;  // < 2^29 for every uint32 max_rows
    hipLaunchKernelGGL(k_rows_accumulate, dim3((uint32_t)blocks), dim3(256), 0, stream, acc, mark, n, ids, grad_rows, count,
                       max_rows, weight);
    hipLaunchKernelGGL(k_rows_mark, dim3(backward_blocks(max_rows)), dim3(256), 0, stream, mark, n, ids, count, max_rows);
}

// ---- collect ------------------------------------------------------------------------------------------------------

namespace {

// The rows of the scan: the flag mark[g] != 0, twice -- row 0 is the scan's count row, row 1 the placed row whose exclusive sum is
// the position of g in U = { g : mark[g] != 0 } (ascending g by construction) and whose total is |U|.  place() is the last
// reader of mark[g] (k_splat_block_sums, the other one, is an earlier launch) and its only writer, so it may clear it.
struct CollectSource {
    static constexpr uint32_t K = 2u, kPlaced = 2u, kTotalsFrom = 1u;
    uint32_t* mark;
    uint32_t* ids_out;
    uint32_t max_rows;
    __device__ void counts(uint32_t g, uint32_t (&c)[K]) const { c[0] = c[1] = mark[g] != 0u ? 1u : 0u; }
    __device__ void place(uint32_t g, const uint32_t (&c)[K], const uint32_t (&pos)[K]) const {
        if (c[1] != 0u) {                         // pos[1] < |U| <= n
            if (pos[1] < max_rows) ids_out[pos[1]] = g;
            mark[g] = 0u;
        }
    }
};

}  // namespace

// A lane per (output row i < min(|U|, max_rows), quad of the 21): the fields of acc[ids_out[i]] bit for bit, +0 in the other 25
// floats -- the row shape of gs_backward_visible*.  Of acc only the fields are loaded.
__global__ __launch_bounds__(256) void k_rows_gather(const float* __restrict__ acc, const uint32_t* __restrict__ ids_out,
                                                     const uint32_t* __restrict__ total, uint32_t max_rows,
                                                     float* __restrict__ rows_out) {
    const uint32_t listed = *total, rows = listed < max_rows ? listed : max_rows;
    const uint64_t first = (uint64_t)blockIdx.x * 256u;
    if (first / kRecordQuads >= rows) return;                     // the whole block is past the count
    const uint64_t item = first + threadIdx.x;
    const uint32_t row = (uint32_t)(item / kRecordQuads), quad = (uint32_t)(item % kRecordQuads);
    if (row >= rows) return;
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (quad < kRecFieldQuads) {
        const size_t at = (size_t)ids_out[row] * kRecordFloats + quad * 4u;     // ids_out[row] < n: the scan wrote it
        const float3 a = *reinterpret_cast<const float3*>(acc + at);
        out.x = a.x; out.y = a.y; out.z = a.z;
        if (rec_is_field(quad * 4u + 3u)) out.w = acc[at + 3];
    }
    reinterpret_cast<float4*>(rows_out)[item] = out;
}

void launch_rows_collect(const float* acc, uint32_t* mark, uint32_t n, const SplatScan& scan, uint32_t* ids_out,
                         float* rows_out, uint32_t max_rows, uint32_t* count_out, hipStream_t stream) {
    launch_splat_scan(CollectSource{mark, ids_out, max_rows}, n, scan, count_out, stream);     // n < 2^31: nothing saturates
    if (max_rows == 0) return;
    const uint32_t most = n < max_rows ? n : max_rows;
    const uint64_t blocks = ((uint64_t)most * kRecordQuads + 255u) / 256u;       // < 2^28 for n < 2^31
    hipLaunchKernelGGL(k_rows_gather, dim3((uint32_t)blocks), dim3(256), 0, stream, acc, ids_out, scan.totals + 1, max_rows,
                       rows_out);
}

}  // namespace gs
