// gs_camera.hip -- gradients of the last frame w.r.t. its camera (gs_backward_camera*, include/gsplat.h): dL/dview[16],
// dL/dproj[16], dL/dcam_pos[3], 35 floats.  A second call behind gs_backward*: the rows the blend backward left in the
// context's scratch are summed per splat once more (splat_row_sum) and taken through the camera side of the per-splat chain,
// in two launches:
//   k_bwd_camera_blocks : thread g < N; a splat that emitted nothing, or whose summed row is zero, contributes 35 zeros
//                   without running the chain.  The 256 x 35 values of a block are summed in a fixed shape -- per component a
//                   DPP wave reduction in float32 (the float twin of wave_sum_to_lane63: the same order on every wave), then
//                   waves 0..3 added in that order through LDS -- and stored as partials[35][blocks] with plain stores;
//   k_bwd_camera_reduce : one workgroup of 1024 in the shape of k_loss_reduce: thread t adds blocks [t per, (t + 1) per) in
//                   ascending order in double, the 1024 totals meet in a fixed LDS tree, each component is rounded once.
// No atomics: the 35 words are a function of the rows and the scene alone.
// The chain is bwd_chain<true> of gs_bwd_chain.h: the function k_bwd_rowsum_chain instantiates with <false> for the record
// gradients, with the camera's statements switched on and the record's outputs off.
#include "gs_bwd_chain.h"

namespace gs {

namespace {

constexpr int kCamFloats = 35;            // GS_CAMERA_GRAD_FLOATS
constexpr int kCamReduceGroup = 7;        // components per round of k_bwd_camera_reduce (5 rounds, 56 KiB of LDS)

// The float twin of wave_sum_to_lane63: lane 63 ends with the wave's sum, added in the same order on every wave.  A lane
// the DPP step does not feed adds the bits of +0.0f.  Every lane of the wave must be active at the call.
__device__ __forceinline__ float wave_sum_f32_to_lane63(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, false));   // row_shr:1
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x112, 0xf, 0xf, false));   // row_shr:2
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x114, 0xf, 0xe, false));   // row_shr:4
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x118, 0xf, 0xc, false));   // row_shr:8
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x142, 0xa, 0xf, false));   // row_bcast:15
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x143, 0xc, 0xf, false));   // row_bcast:31
    return v;
}

}  // namespace

// Thread g of the grid backward_blocks(N) x 256.  No thread leaves early: every lane takes part in the wave sums.
__global__ __launch_bounds__(256) void k_bwd_camera_blocks(const FrameParams fp, const SceneBuffers scene,
                                                            const SplatCounts counts,
                                                            const uint32_t* __restrict__ offsets,
                                                            const float* __restrict__ rows, float* __restrict__ partials) {
    __shared__ float s_part[4][kCamFloats];
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    float cg[kCamFloats];
#pragma unroll
    for (int k = 0; k < kCamFloats; ++k) cg[k] = 0.0f;
    if (g < fp.num_gaussians && counts.of(g) != 0u) {
        float row[kRowFloats];
        splat_row_sum(counts, offsets, rows, g, fp.capacity, row);
        bwd_chain<true>(fp, scene, g, true, row, nullptr, cg);       // a zero row leaves the zeros
    }
    const int lane = lane_id(), wave = wave_id();
#pragma unroll
    for (int k = 0; k < kCamFloats; ++k) {
        const float t = wave_sum_f32_to_lane63(cg[k]);
        if (lane == 63) s_part[wave][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)kCamFloats) {
        const uint32_t k = threadIdx.x;
        partials[(size_t)k * gridDim.x + blockIdx.x] = ((s_part[0][k] + s_part[1][k]) + s_part[2][k]) + s_part[3][k];
    }
}

// One workgroup: thread t sums blocks [t * per, (t + 1) * per) in order, in double; the 1024 totals meet in a fixed tree in
// LDS, kCamReduceGroup components per round.
__global__ __launch_bounds__(1024) void k_bwd_camera_reduce(const float* __restrict__ partials, uint32_t blocks,
                                                             float* __restrict__ out) {
    __shared__ double s_s[kCamReduceGroup][1024];
    const uint32_t per = (blocks + 1023u) / 1024u;
    const uint32_t b0 = threadIdx.x * per;
    for (int k0 = 0; k0 < kCamFloats; k0 += kCamReduceGroup) {
#pragma unroll
        for (int j = 0; j < kCamReduceGroup; ++j) {
            const float* col = partials + (size_t)(k0 + j) * blocks;
            double sum = 0.0;
            for (uint32_t i = 0; i < per; ++i)
                if (b0 + i < blocks) sum += (double)col[b0 + i];
            s_s[j][threadIdx.x] = sum;
        }
        __syncthreads();
        for (uint32_t half = 512u; half > 0u; half >>= 1) {
            if (threadIdx.x < half) {
#pragma unroll
                for (int j = 0; j < kCamReduceGroup; ++j) s_s[j][threadIdx.x] += s_s[j][threadIdx.x + half];
            }
            __syncthreads();
        }
        if (threadIdx.x < (uint32_t)kCamReduceGroup) out[k0 + threadIdx.x] = (float)s_s[threadIdx.x][0];
        __syncthreads();
    }
}

size_t backward_camera_partial_bytes(uint32_t n) { return (size_t)kCamFloats * backward_blocks(n) * sizeof(float); }

void launch_backward_camera(const BackwardFrame& f, float* partials, float* grad_camera, hipStream_t stream) {
    const uint32_t blocks = backward_blocks(f.fp.num_gaussians);
    hipLaunchKernelGGL(k_bwd_camera_blocks, dim3(blocks), dim3(256), 0, stream, f.fp, f.scene, splat_counts_of(f.sc, f.fp),
                       f.bb.scan.offsets, f.bb.rows, partials);
    hipLaunchKernelGGL(k_bwd_camera_reduce, dim3(1), dim3(1024), 0, stream, partials, blocks, grad_camera);
}

} // namespace gs
