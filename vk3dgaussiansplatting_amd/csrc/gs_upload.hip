// gs_upload.hip -- one-off conversion of the reference's 336-byte AoS GaussianData records
// (Engine/Graphics/ShaderStructs.h:59-70) to the SoA planes the per-frame kernels read with fully
// coalesced loads.  Runs once per scene (Renderer::initForScene, Renderer.cpp:712-724), chunk by
// chunk through a staging buffer so a 50 M-splat scene never needs a second full-size AoS copy in HBM.
#include "gs_splat_math.h"

namespace gs {

// One record (rec: its 84 floats) into the planes of splat g; n = total splats (plane stride).  Called by the four waves of
// a workgroup with part = 0..3 and lane = record: they split the 59 fields, and part 3 adds the cull bound sig2.  The one
// place a record becomes planes: the full upload and the upload of listed rows write the same bits.
__device__ __forceinline__ void store_record_planes(const float* rec, uint32_t part, size_t g, uint32_t n, const SceneBuffers& s) {
    for (uint32_t fld = part; fld < kRecFields; fld += 4u) {
        if (fld < 3u) s.pos[(size_t)fld * n + g] = rec[kRecPos + fld];
        else if (fld < 6u) s.scale[(size_t)(fld - 3u) * n + g] = rec[kRecScale + (fld - 3u)];
        else if (fld < 10u) s.rot[(size_t)(fld - 6u) * n + g] = rec[kRecRot + (fld - 6u)];
        else if (fld < 58u) {
            const uint32_t k = fld - 10u, coeff = k / 3u, ch = k % 3u;
            s.sh[(size_t)k * n + g] = rec[rec_sh(coeff, ch)];
        } else s.opacity[g] = rec[kRecOpacity];
    }
    if (part == 3u) {
        // |R|_2^2 * max(scale)^2 >= largest eigenvalue of Sigma = (R S)(R S)^T, with R as Common.glsl:17-30
        // builds it from the (not necessarily unit) quaternion
        const Mat3 rm = get_rot_mat(rec[kRecRot], rec[kRecRot + 1], rec[kRecRot + 2], rec[kRecRot + 3]);
        const float (&e)[3][3] = rm.m;                   // e[i]: column i of R; R^T R has the norm of R R^T
        // |R|_2^2 <= min(trace, largest absolute row sum) of R R^T (Gershgorin): 1 for a unit quaternion, where the
        // Frobenius norm alone says 3
        // the maxima keep a NaN (fmaxf would drop it): a NaN scale, or a row of R R^T that is inf - inf (an infinite
        // quaternion component, or a finite one whose square overflows), must end in a NaN or infinite bound -- the
        // splat's own covariance is NaN then, and the reference puts such a splat into tile 0
        auto nan_max = [](float a, float b) { return (a > b || a != a) ? a : b; };
        float f2 = 0.0f, gersh = 0.0f;
#pragma unroll
        for (int k = 0; k < 9; ++k) f2 += e[k / 3][k % 3] * e[k / 3][k % 3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            float row = 0.0f;
#pragma unroll
            for (int j = 0; j < 3; ++j) row += fabsf(e[i][0] * e[j][0] + e[i][1] * e[j][1] + e[i][2] * e[j][2]);
            gersh = nan_max(row, gersh);
        }
        const float r2 = (gersh < f2 ? gersh : f2) * 1.0001f;      // a NaN takes f2, NaN or infinite: the splat is kept
        const float s0 = fabsf(rec[kRecScale]), s1 = fabsf(rec[kRecScale + 1]), s2 = fabsf(rec[kRecScale + 2]);
        const float sm = nan_max(s0, nan_max(s1, s2));
        s.sig2[g] = r2 * sm * sm;
    }
}

// chunk: [count][84] floats starting at splat `first`; n = total splats (plane stride)
__global__ __launch_bounds__(256) void k_aos_to_soa(const float* __restrict__ chunk, uint32_t first,
                                                     uint32_t count, uint32_t n, SceneBuffers s) {
    __shared__ float tile[64][kRecordFloats + 1];   // 64 records, padded row to dodge bank conflicts
    const uint32_t rec0 = blockIdx.x * 64u;
    const uint32_t nrec = (count - rec0) < 64u ? (count - rec0) : 64u;
    // coalesced read of nrec*84 consecutive floats
    for (uint32_t k = threadIdx.x; k < nrec * kRecordFloats; k += 256u)
        tile[k / kRecordFloats][k % kRecordFloats] = chunk[(size_t)rec0 * kRecordFloats + k];
    __syncthreads();
    // coalesced plane writes: lane = record
    const uint32_t r = threadIdx.x & 63u, part = threadIdx.x >> 6;   // 4 waves split the 59 fields
    if (r < nrec) store_record_planes(tile[r], part, (size_t)first + rec0 + r, n, s);
}

// gs_upload_rows_device: a workgroup per 64 listed rows; records = the whole [n][84] array, the fields of row ids[i] staged
// for i below min(*count, max_rows) and ids[i] < n.  The ids ascend (gs_backward_visible* writes them so), which keeps the plane writes
// of neighbouring lanes close.
__global__ __launch_bounds__(256) void k_upload_rows(const float* __restrict__ records, uint32_t n,
                                                      const uint32_t* __restrict__ ids, const uint32_t* __restrict__ count,
                                                      uint32_t max_rows, SceneBuffers s) {
    __shared__ float tile[64][kRecordFloats + 1];
    __shared__ uint32_t id_of[64];
    const uint32_t listed = *count, rows = listed < max_rows ? listed : max_rows;
    const uint32_t row0 = blockIdx.x * 64u;
    if (row0 >= rows) return;                                    // the whole block is past the count
    const uint32_t nrow = (rows - row0) < 64u ? (rows - row0) : 64u;
    if (threadIdx.x < nrow) id_of[threadIdx.x] = ids[row0 + threadIdx.x];
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < nrow * kRecordFloats; k += 256u) {
        const uint32_t g = id_of[k / kRecordFloats], col = k % kRecordFloats;
        // the 59 fields only: the other 25 floats of a record are never read
        if (g < n && rec_is_field(col)) tile[k / kRecordFloats][col] = records[(size_t)g * kRecordFloats + col];
    }
    __syncthreads();
    const uint32_t r = threadIdx.x & 63u, part = threadIdx.x >> 6;
    if (r < nrow && id_of[r] < n) store_record_planes(tile[r], part, (size_t)id_of[r], n, s);
}

// Per wave of the project kernel (64 consecutive splats -- neighbours in space, the arrays are in Morton order): the box
// around the positions and the largest sig2.  A context that renders a subset of the tile rows rejects whole waves
// with it (k_project).  min/max are exact selections, so the box contains every position whatever the order.
__global__ __launch_bounds__(256) void k_block_bounds(uint32_t n, SceneBuffers s) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    const bool ok = g < n;
    float v[7];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = ok ? s.pos[(size_t)a * n + g] : 0.0f;
        v[a] = ok ? p : 3.0e38f;        // min
        v[3 + a] = ok ? p : -3.0e38f;   // max
    }
    v[6] = ok ? s.sig2[g] : 0.0f;
    // a NaN position or bound must not be lost by fminf/fmaxf: it poisons the record instead (k_project then keeps
    // the wave, every comparison with a NaN being false)
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 7; ++k) bad = bad || (ok && !(v[k] == v[k]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = fminf(v[k], __shfl_xor(v[k], off, 64));
#pragma unroll
        for (int k = 3; k < 7; ++k) v[k] = fmaxf(v[k], __shfl_xor(v[k], off, 64));
    }
    const bool wave_bad = __ballot(bad) != 0ull;
    if ((threadIdx.x & 63) == 0 && blockIdx.x * 256u + (threadIdx.x & ~63u) < n) {
        const float nanv = __builtin_nanf("");
        float4* out = reinterpret_cast<float4*>(s.block_bounds) + (size_t)(g >> 6) * 2;
        out[0] = wave_bad ? make_float4(nanv, nanv, nanv, nanv) : make_float4(v[0], v[1], v[2], v[3]);
        out[1] = wave_bad ? make_float4(nanv, nanv, nanv, nanv) : make_float4(v[4], v[5], v[6], 0.0f);
    }
}

void launch_block_bounds(uint32_t n, const SceneBuffers& s, hipStream_t stream) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_block_bounds, dim3((n + 255u) / 256u), dim3(256), 0, stream, n, s);
}

void launch_upload_rows(const float* records, uint32_t n, const uint32_t* ids, const uint32_t* count, uint32_t max_rows,
                        const SceneBuffers& s, hipStream_t stream) {
    if (max_rows == 0) return;
    hipLaunchKernelGGL(k_upload_rows, dim3(max_rows / 64u + (max_rows % 64u ? 1u : 0u)), dim3(256), 0, stream, records, n, ids, count, max_rows, s);
}

void launch_aos_to_soa(const float* chunk, uint32_t first, uint32_t count, uint32_t n,
                       const SceneBuffers& s, hipStream_t stream) {
    if (count == 0) return;
    hipLaunchKernelGGL(k_aos_to_soa, dim3((count + 63u) / 64u), dim3(256), 0, stream, chunk, first,
                       count, n, s);
}

} // namespace gs

// ---------------------------------------------------------------------------------------------
// Stream bandwidth probes: the "measured HBM roofline" denominator of north_star (device-to-device
// copy on the same MI355X) and the small-buffer regime the per-pass sort kernels live in.
// ---------------------------------------------------------------------------------------------
namespace gs {

template <typename T>
__global__ __launch_bounds__(256) void k_stream_copy(const T* __restrict__ src, T* __restrict__ dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        dst[i] = src[i];
}

template <typename T>
__global__ __launch_bounds__(256) void k_stream_read(const T* __restrict__ src, uint32_t* __restrict__ sink, size_t n) {
    uint32_t acc = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const T v = src[i];
        const uint32_t* w = reinterpret_cast<const uint32_t*>(&v);
#pragma unroll
        for (int k = 0; k < (int)(sizeof(T) / 4); ++k) acc ^= w[k];
    }
    if (acc == 0x9E3779B9u) sink[0] = acc;   // keeps the loads alive, practically never taken
}

// Copy with four 16-byte loads in flight per lane before the first store (the plain grid-stride copy above keeps one):
// what MI355X_MICROARCH.md's 6.3 TB/s "float4 copy" needs -- more bytes in flight per CU.  NT = 1: non-temporal
// stores (the destination is not re-read); NT = 2: non-temporal loads too.
template <int NT>
__global__ __launch_bounds__(256) void k_stream_copy4(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n) {
    const size_t stride = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (NT == 2) {
                const unsigned __attribute__((ext_vector_type(4)))* p =
                    reinterpret_cast<const unsigned __attribute__((ext_vector_type(4)))*>(src + i + k * stride);
                const unsigned __attribute__((ext_vector_type(4))) t = __builtin_nontemporal_load(p);
                v[k] = make_uint4(t.x, t.y, t.z, t.w);
            } else {
                v[k] = src[i + k * stride];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (NT >= 1) {
                unsigned __attribute__((ext_vector_type(4))) t = {v[k].x, v[k].y, v[k].z, v[k].w};
                __builtin_nontemporal_store(t, reinterpret_cast<unsigned __attribute__((ext_vector_type(4)))*>(dst + i + k * stride));
            } else {
                dst[i + k * stride] = v[k];
            }
        }
    }
    for (; i < n; i += stride) dst[i] = src[i];
}

// Radix-scatter write pattern without the sorting: the buffer is treated as three arrays of n dwords;
// persistent workgroups read tiles of TILE consecutive dwords from each array and write every tile as
// 16 runs of TILE/16 dwords into 16 destination regions (what a 4-bit pass with uniform digits does).
template <int TILE, int SKEW = 0>
__global__ __launch_bounds__(256) void k_scatter_pattern(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, size_t n3) {
    const size_t n = n3 / 3;                       // dwords per array
    const size_t tiles = n / TILE;
    constexpr int RUN = TILE / 16;
    for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const uint32_t* s = src + a * n + t * TILE;
            uint32_t* d = dst + a * n;
#pragma unroll
            for (int r = 0; r < TILE / 256; ++r) {
                const int p = r * 256 + threadIdx.x;          // position inside the tile
                const int digit = p / RUN, off = p % RUN;
                d[(size_t)digit * (n / 16) + t * RUN + off + (size_t)digit * SKEW] = s[p];   // SKEW: misaligned regions
            }
        }
    }
}

void launch_stream_probe(int kind, const void* src, void* dst, size_t bytes, uint32_t blocks, hipStream_t stream) {
    switch (kind) {
        case 4: hipLaunchKernelGGL(k_scatter_pattern<3072>, dim3(blocks), dim3(256), 0, stream, (const uint32_t*)src, (uint32_t*)dst, bytes / 4); return;
        case 5: hipLaunchKernelGGL(k_scatter_pattern<6144>, dim3(blocks), dim3(256), 0, stream, (const uint32_t*)src, (uint32_t*)dst, bytes / 4); return;
        case 6: hipLaunchKernelGGL(k_scatter_pattern<12288>, dim3(blocks), dim3(256), 0, stream, (const uint32_t*)src, (uint32_t*)dst, bytes / 4); return;
        case 7: hipLaunchKernelGGL(k_scatter_pattern<49152>, dim3(blocks), dim3(256), 0, stream, (const uint32_t*)src, (uint32_t*)dst, bytes / 4); return;
        case 8: hipLaunchKernelGGL((k_scatter_pattern<3072, 37>), dim3(blocks), dim3(256), 0, stream, (const uint32_t*)src, (uint32_t*)dst, bytes / 4); return;
        case 9: hipLaunchKernelGGL((k_scatter_pattern<3072, 5>), dim3(blocks), dim3(256), 0, stream, (const uint32_t*)src, (uint32_t*)dst, bytes / 4); return;
        case 10: hipLaunchKernelGGL(k_stream_copy4<0>, dim3(blocks), dim3(256), 0, stream, (const uint4*)src, (uint4*)dst, bytes / 16); return;
        case 11: hipLaunchKernelGGL(k_stream_copy4<1>, dim3(blocks), dim3(256), 0, stream, (const uint4*)src, (uint4*)dst, bytes / 16); return;
        case 12: hipLaunchKernelGGL(k_stream_copy4<2>, dim3(blocks), dim3(256), 0, stream, (const uint4*)src, (uint4*)dst, bytes / 16); return;
        default: break;
    }
    switch (kind) {
        case 0: hipLaunchKernelGGL(k_stream_read<uint4>, dim3(blocks), dim3(256), 0, stream, (const uint4*)src, (uint32_t*)dst, bytes / 16); break;
        case 1: hipLaunchKernelGGL(k_stream_copy<uint4>, dim3(blocks), dim3(256), 0, stream, (const uint4*)src, (uint4*)dst, bytes / 16); break;
        case 2: hipLaunchKernelGGL(k_stream_read<uint32_t>, dim3(blocks), dim3(256), 0, stream, (const uint32_t*)src, (uint32_t*)dst, bytes / 4); break;
        default: hipLaunchKernelGGL(k_stream_copy<uint32_t>, dim3(blocks), dim3(256), 0, stream, (const uint32_t*)src, (uint32_t*)dst, bytes / 4); break;
    }
}

} // namespace gs
