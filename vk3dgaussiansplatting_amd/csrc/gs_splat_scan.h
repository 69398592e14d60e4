// gs_splat_scan.h -- the exclusive scan over the splats that gs_backward.hip (dense and visible) and gs_densify.hip run, as
// three launches without atomics over the buffers of a SplatScan (gs_internal.h):
//   k_splat_block_sums  : the K sums of every block of 256 splats;
//   k_splat_scan_blocks : one workgroup of 1024 threads, each owning per = ceil(blocks / 1024) consecutive blocks: the
//                         exclusive scan of the block sums and, for the rows from S::kTotalsFrom on, the grand totals;
//   k_splat_offsets     : offsets[g] = row 0 summed over the splats before g, and S::place for what else the caller
//                         derives from the position of g.
// Row 0 is the count row: its running total is 64 bits wide and stored saturated at 2^32 - 1.  The other rows count splats
// (flags 0 / 1) and stay below 2^32.  The caller describes its rows with a source S, passed by value:
//   static constexpr uint32_t K;            rows summed
//   static constexpr uint32_t kPlaced;      leading rows whose exclusive sum per splat place() consumes (1: offsets[] only)
//   static constexpr uint32_t kTotalsFrom;  rows kTotalsFrom .. K - 1 have their totals stored
//   void counts(uint32_t g, uint32_t (&c)[K]) const;                                  g < n
//   void place(uint32_t g, const uint32_t (&c)[K], const uint32_t (&pos)[kPlaced]) const;   g < n; pos[0] is not set
// A row the caller does not ask for costs nothing: K = 1 is the plain scan of one count per splat.
#pragma once

#include "gs_device_utils.h"
#include "gs_internal.h"

namespace gs {

__device__ __forceinline__ uint32_t saturate32(uint64_t v) { return v < 0xFFFFFFFFull ? (uint32_t)v : 0xFFFFFFFFu; }

template <class S>
__global__ __launch_bounds__(256) void k_splat_block_sums(const S src, uint32_t n, uint32_t blocks,
                                                           uint32_t* __restrict__ block_sums) {
    __shared__ uint32_t s_w[S::K][4];
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    uint32_t c[S::K] = {};
    if (g < n) src.counts(g, c);
#pragma unroll
    for (uint32_t q = 0; q < S::K; ++q) {
        const uint32_t t = wave_sum_to_lane63(c[q]);                  // < 256 * the largest count: no overflow
        if (lane_id() == 63) s_w[q][wave_id()] = t;
    }
    __syncthreads();
    if (threadIdx.x < S::K) {
        const uint32_t q = threadIdx.x;
        block_sums[(size_t)q * blocks + blockIdx.x] = s_w[q][0] + s_w[q][1] + s_w[q][2] + s_w[q][3];
    }
}

// Every thread carries the running totals across its `per` blocks.  The last thread of the last wave ends with the grand
// totals: rows kTotalsFrom .. K - 1 of them go to totals[q] and to totals_copy[q - kTotalsFrom] (either may be null).
template <class S>
__global__ __launch_bounds__(1024) void k_splat_scan_blocks(const uint32_t* __restrict__ block_sums, uint32_t blocks,
                                                             uint32_t* __restrict__ block_offsets,
                                                             uint32_t* __restrict__ totals,
                                                             uint32_t* __restrict__ totals_copy) {
    constexpr uint32_t K = S::K;
    __shared__ uint64_t s_w[16];
    __shared__ uint32_t s_f[K][16];                                   // row 0 unused
    const uint32_t per = (blocks + 1023u) / 1024u;
    const uint32_t b0 = threadIdx.x * per;
    uint64_t mine = 0;
    uint32_t fmine[K] = {}, frun[K] = {};
    for (uint32_t k = 0; k < per; ++k) {
        if (b0 + k < blocks) {
            mine += block_sums[b0 + k];
#pragma unroll
            for (uint32_t q = 1; q < K; ++q) fmine[q] += block_sums[(size_t)q * blocks + b0 + k];
        }
    }
    const uint64_t inc = wave_inclusive_scan64(mine);
    if (lane_id() == 63) s_w[wave_id()] = inc;
#pragma unroll
    for (uint32_t q = 1; q < K; ++q) {
        const uint32_t finc = wave_inclusive_scan(fmine[q]);
        if (lane_id() == 63) s_f[q][wave_id()] = finc;
        frun[q] = finc - fmine[q];
    }
    __syncthreads();
    uint64_t run = inc - mine;
    for (int w = 0; w < wave_id(); ++w) {
        run += s_w[w];
#pragma unroll
        for (uint32_t q = 1; q < K; ++q) frun[q] += s_f[q][w];
    }
    for (uint32_t k = 0; k < per; ++k) {
        if (b0 + k < blocks) {
            block_offsets[b0 + k] = saturate32(run);
            run += block_sums[b0 + k];
#pragma unroll
            for (uint32_t q = 1; q < K; ++q) {
                block_offsets[(size_t)q * blocks + b0 + k] = frun[q];
                frun[q] += block_sums[(size_t)q * blocks + b0 + k];
            }
        }
    }
    if constexpr (S::kTotalsFrom < K) {
        if (threadIdx.x == 1023u) {
#pragma unroll
            for (uint32_t q = S::kTotalsFrom; q < K; ++q) {
                const uint32_t t = q == 0u ? saturate32(run) : frun[q];
                if (totals) totals[q] = t;
                if (totals_copy) totals_copy[q - S::kTotalsFrom] = t;
            }
        }
    }
}

template <class S>
__global__ __launch_bounds__(256) void k_splat_offsets(const S src, uint32_t n, uint32_t blocks,
                                                        const uint32_t* __restrict__ block_offsets,
                                                        uint32_t* __restrict__ offsets) {
    constexpr uint32_t P = S::kPlaced;
    __shared__ uint32_t s_w[P][4];
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    uint32_t c[S::K] = {}, before[P];
    if (g < n) src.counts(g, c);
#pragma unroll
    for (uint32_t q = 0; q < P; ++q) {
        const uint32_t inc = wave_inclusive_scan(c[q]);
        if (lane_id() == 63) s_w[q][wave_id()] = inc;
        before[q] = inc - c[q];
    }
    __syncthreads();
    for (int w = 0; w < wave_id(); ++w) {
#pragma unroll
        for (uint32_t q = 0; q < P; ++q) before[q] += s_w[q][w];
    }
    if (g >= n) return;
    offsets[g] = saturate32((uint64_t)block_offsets[blockIdx.x] + before[0]);
    if constexpr (P > 1) {
#pragma unroll
        for (uint32_t q = 1; q < P; ++q) before[q] += block_offsets[(size_t)q * blocks + blockIdx.x];
        src.place(g, c, before);
    }
}

// The three launches for the n splats of `src` over the buffers of `b` (allocated for at least n splats and S::K rows)
template <class S>
void launch_splat_scan(const S& src, uint32_t n, const SplatScan& b, uint32_t* totals_copy, hipStream_t stream) {
    const uint32_t blocks = backward_blocks(n);
    hipLaunchKernelGGL(k_splat_block_sums<S>, dim3(blocks), dim3(256), 0, stream, src, n, blocks, b.block_sums);
    hipLaunchKernelGGL(k_splat_scan_blocks<S>, dim3(1), dim3(1024), 0, stream, b.block_sums, blocks, b.block_offsets, b.totals,
                       totals_copy);
    hipLaunchKernelGGL(k_splat_offsets<S>, dim3(blocks), dim3(256), 0, stream, src, n, blocks, b.block_offsets, b.offsets);
}

} // namespace gs
