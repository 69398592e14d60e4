// gs_loss.hip -- the photometric loss of a 3DGS optimisation step (gs_photometric_loss*, include/gsplat.h):
//   loss = (1 - lambda) * L1 + lambda * (1 - mean SSIM) of the composited frame I = rgb + (1 - a) * bg against a target G,
// and its gradient with respect to the RGBA32F quantities of the frame, in the layout gs_backward* takes.  Three launches:
//   k_loss_forward  : per 16 x 16 tile, G and D = I - G with a 5-pixel halo in LDS (zero outside the image, the zero padding
//                     of conv2d(padding = 5)), five 11 x 11 gaussian windows per channel -- conv(G), conv(D), conv(G G),
//                     conv(D D), conv(G D) -- run separably (rows into LDS, then columns); per pixel and channel 1 - ssim and
//                     |D|, and the three partial derivatives of ssim the backward convolves, each already scaled by
//                     -lambda / (3 H W), stored as three float[H][W][3] maps; the tile's sums of 1 - ssim and of |D| reduced
//                     in a fixed tree (wave butterfly, then the four waves in order) and stored as one pair;
//   k_loss_reduce   : one workgroup sums the pairs in a fixed order (every thread owns consecutive tiles) and writes
//                     loss_out = {loss, L1, DSSIM};
//   k_loss_backward : same tiling over the three maps (zero outside: a window centred outside the image does not exist),
//                     dI = conv(A) + (2 (I - G) conv(B) + G conv(E)) + (1 - lambda) / (3 H W) * sign(I - G), written as
//                     float4 (dI, -sum_c bg_c dI_c).  Skipped for a loss-only call.
// The window is symmetric, so the adjoint of the convolution is the convolution.  No float atomics: loss and gradient are
// bitwise reproducible.
// Why D and not I: a training step spends its life near I == G, where ssim = 1 - (small) and its gradient is a difference
// of terms a thousand times its size.  With mu1 = mG + mD, s2 = conv(G G) - mG^2, vD = conv(D D) - mD^2 and
// cGD = conv(G D) - mG mD (so sigma1^2 = s2 + 2 cGD + vD, sigma12 = s2 + cGD) every such difference is a quantity of its own:
//   1 - ssim = mD^2 / B1 + lum * vD / B2                       (lum = A1 / B1, cs = A2 / B2, ssim = lum * cs)
//   B = d ssim / d sigma1^2 = -ssim / B2
//   E = d ssim / d sigma12 + 2 B = 2 lum vD / B2^2
//   A = d ssim / d mu1 with the variances' -2 mu1 and -mu2 terms folded in
//     = -2 cs mD (mu2 (mu1 + mu2) + C1) / B1^2 - 2 B mD - E mu2
// and 2 I conv(B) + G conv(C) = 2 (I - G) conv(B) + G conv(E).  Nothing cancels: DSSIM keeps its relative accuracy down to
// zero, and I == G gives DSSIM = 0 and a zero gradient exactly.  The same five windows as the textbook form, the same cost.
// The window sums use fused multiply-adds (asked for by name: the file is compiled with -ffp-contract=off like the rest).
#include "gs_device_utils.h"
#include "gs_internal.h"

namespace gs {

constexpr int kLossR = 5;                         // window radius: 11 taps
constexpr int kLossHalo = kTile + 2 * kLossR;     // 26
constexpr int kLossTexels = kLossHalo * kLossHalo;   // 676 staged texels of a tile
constexpr int kLossRowOut = kLossHalo * kTile;       // 416 outputs of the row pass: 26 rows x 16 columns

// exp(-k^2 / (2 * 1.5^2)), k = -5 .. 5, normalised to sum 1 in double and rounded once
__device__ __forceinline__ float loss_weight(int k) {
    constexpr float w[11] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c40p-3f, 0x1.106560p-2f,
                             0x1.b43c40p-3f,  0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};
    return w[k];
}

// sum_k w[k] * p[k * stride], taps in ascending k
__device__ __forceinline__ float loss_window(const float* p, int stride) {
    float acc = loss_weight(0) * p[0];
#pragma unroll
    for (int k = 1; k < 11; ++k) acc = __builtin_fmaf(loss_weight(k), p[k * stride], acc);
    return acc;
}

struct LossArgs {
    const float4* rgba;     // [H][W]
    const float* target;    // [H][W][3]
    float* maps;            // [3][H][W][3]: A, B, E
    float2* tile_sums;      // [tiles]: sum of 1 - ssim, sum of |I - G|
    float4* grad;           // [H][W] or null
    float* loss_out;        // [3]
    uint32_t width, height, grid_w, tiles;
    float bg[3];
    uint32_t has_bg;
    float lambda;
    float ssim_scale;       // -lambda / (3 H W)
    float l1_scale;         // (1 - lambda) / (3 H W)
    double inv_count;       // 1 / (3 H W)
};

__device__ __forceinline__ void loss_composite(const LossArgs& a, const float4 v, float out[3]) {
    out[0] = v.x; out[1] = v.y; out[2] = v.z;
    if (a.has_bg) {
        const float t = 1.0f - v.w;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = out[c] + t * a.bg[c];
    }
}

// One 256-thread workgroup per tile, one pixel per thread.
__global__ __launch_bounds__(256) void k_loss_forward(const LossArgs a) {
    __shared__ float s_g[3][kLossTexels];
    __shared__ float s_d[3][kLossTexels];         // D = I - G
    __shared__ float s_row[15][kLossRowOut];      // per channel: conv_x of G, D, G G, D D, G D
    __shared__ float s_part[4][2];

    const int tid = threadIdx.x;
    const uint32_t tile = blockIdx.x;
    const int x0 = (int)((tile % a.grid_w) * kTile) - kLossR, y0 = (int)((tile / a.grid_w) * kTile) - kLossR;

    for (int t = tid; t < kLossTexels; t += 256) {
        const int x = x0 + t % kLossHalo, y = y0 + t / kLossHalo;
        float dv[3] = {0.0f, 0.0f, 0.0f}, gv[3] = {0.0f, 0.0f, 0.0f};
        if (x >= 0 && y >= 0 && x < (int)a.width && y < (int)a.height) {
            const size_t p = (size_t)y * a.width + (size_t)x;
            float iv[3];
            loss_composite(a, a.rgba[p], iv);
#pragma unroll
            for (int c = 0; c < 3; ++c) { gv[c] = a.target[p * 3 + c]; dv[c] = iv[c] - gv[c]; }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { s_d[c][t] = dv[c]; s_g[c][t] = gv[c]; }
    }
    __syncthreads();

    // rows: output (r, x) of the 26 x 16 block reads texels (r, x .. x + 10)
    for (int o = tid; o < kLossRowOut; o += 256) {
        const int r = o / kTile, x = o % kTile;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float vg[11], vd[11], t[11];
#pragma unroll
            for (int k = 0; k < 11; ++k) { vg[k] = s_g[c][r * kLossHalo + x + k]; vd[k] = s_d[c][r * kLossHalo + x + k]; }
            s_row[c * 5 + 0][o] = loss_window(vg, 1);
            s_row[c * 5 + 1][o] = loss_window(vd, 1);
#pragma unroll
            for (int k = 0; k < 11; ++k) t[k] = vg[k] * vg[k];
            s_row[c * 5 + 2][o] = loss_window(t, 1);
#pragma unroll
            for (int k = 0; k < 11; ++k) t[k] = vd[k] * vd[k];
            s_row[c * 5 + 3][o] = loss_window(t, 1);
#pragma unroll
            for (int k = 0; k < 11; ++k) t[k] = vg[k] * vd[k];
            s_row[c * 5 + 4][o] = loss_window(t, 1);
        }
    }
    __syncthreads();

    // columns, then the pixel
    const int lx = tid & 15, ly = tid >> 4;
    const uint32_t px = (uint32_t)(x0 + kLossR + lx), py = (uint32_t)(y0 + kLossR + ly);
    const bool inside = px < a.width && py < a.height;
    float sum_dssim = 0.0f, sum_l1 = 0.0f;
    if (inside) {
        const size_t p = (size_t)py * a.width + px, plane = (size_t)a.width * a.height * 3;
        const int centre = (ly + kLossR) * kLossHalo + lx + kLossR;
        constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* col = &s_row[c * 5][ly * kTile + lx];
            const float mG = loss_window(col, kTile), mD = loss_window(col + kLossRowOut, kTile);
            const float s2 = loss_window(col + 2 * kLossRowOut, kTile) - mG * mG;
            const float vD = loss_window(col + 3 * kLossRowOut, kTile) - mD * mD;
            const float cGD = loss_window(col + 4 * kLossRowOut, kTile) - mG * mD;
            const float m2 = mG, m1 = mG + mD;
            const float s1 = s2 + (2.0f * cGD + vD), s12 = s2 + cGD;
            const float A1 = 2.0f * (m1 * m2) + C1, A2 = 2.0f * s12 + C2;
            const float B1 = (m1 * m1 + m2 * m2) + C1, B2 = (s1 + s2) + C2;
            const float lum = A1 / B1, cs = A2 / B2;
            const float ssim = lum * cs;
            const float d_s1 = -ssim / B2;
            const float d_e = 2.0f * lum * vD / (B2 * B2);
            const float d_m1 = -2.0f * cs * mD * (m2 * (m1 + m2) + C1) / (B1 * B1);      // with sigma1^2, sigma12 held
            const float d_mu = (d_m1 - 2.0f * d_s1 * mD) - d_e * m2;
            a.maps[p * 3 + c] = d_mu * a.ssim_scale;
            a.maps[plane + p * 3 + c] = d_s1 * a.ssim_scale;
            a.maps[2 * plane + p * 3 + c] = d_e * a.ssim_scale;
            sum_dssim += (mD * mD) / B1 + lum * (vD / B2);
            sum_l1 += fabsf(s_d[c][centre]);
        }
    }
    // the tile's sums: a fixed butterfly (every lane ends with the same bits), then the four waves in order
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        sum_dssim += __shfl_xor(sum_dssim, off, 64);
        sum_l1 += __shfl_xor(sum_l1, off, 64);
    }
    if (lane_id() == 0) { s_part[wave_id()][0] = sum_dssim; s_part[wave_id()][1] = sum_l1; }
    __syncthreads();
    if (tid == 0)
        a.tile_sums[tile] = make_float2(((s_part[0][0] + s_part[1][0]) + s_part[2][0]) + s_part[3][0],
                                        ((s_part[0][1] + s_part[1][1]) + s_part[2][1]) + s_part[3][1]);
}

// One workgroup: thread t sums tiles [t * per, (t + 1) * per) in order, in double (a tile's float sums are exact there and a
// 4K frame has 25 M terms); the 1024 totals meet in a fixed tree in LDS.
__global__ __launch_bounds__(1024) void k_loss_reduce(const LossArgs a) {
    __shared__ double s_s[1024], s_l[1024];
    const uint32_t per = (a.tiles + 1023u) / 1024u;
    const uint32_t t0 = threadIdx.x * per;
    double ss = 0.0, sl = 0.0;
    for (uint32_t k = 0; k < per; ++k) {
        if (t0 + k < a.tiles) {
            const float2 v = a.tile_sums[t0 + k];
            ss += (double)v.x;
            sl += (double)v.y;
        }
    }
    s_s[threadIdx.x] = ss;
    s_l[threadIdx.x] = sl;
    __syncthreads();
    for (uint32_t half = 512u; half > 0u; half >>= 1) {
        if (threadIdx.x < half) {
            s_s[threadIdx.x] += s_s[threadIdx.x + half];
            s_l[threadIdx.x] += s_l[threadIdx.x + half];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double l1 = s_l[0] * a.inv_count, dssim = s_s[0] * a.inv_count;
        const double lam = (double)a.lambda;
        a.loss_out[0] = (float)((1.0 - lam) * l1 + lam * dssim);
        a.loss_out[1] = (float)l1;
        a.loss_out[2] = (float)dssim;
    }
}

__global__ __launch_bounds__(256) void k_loss_backward(const LossArgs a) {
    __shared__ float s_m[9][kLossTexels];         // map * 3 + channel
    __shared__ float s_row[9][kLossRowOut];

    const int tid = threadIdx.x;
    const uint32_t tile = blockIdx.x;
    const int x0 = (int)((tile % a.grid_w) * kTile) - kLossR, y0 = (int)((tile / a.grid_w) * kTile) - kLossR;
    const size_t plane = (size_t)a.width * a.height * 3;

    for (int t = tid; t < kLossTexels; t += 256) {
        const int x = x0 + t % kLossHalo, y = y0 + t / kLossHalo;
        const bool in = x >= 0 && y >= 0 && x < (int)a.width && y < (int)a.height;
        const size_t p = in ? ((size_t)y * a.width + (size_t)x) * 3 : 0;
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
            for (int c = 0; c < 3; ++c) s_m[m * 3 + c][t] = in ? a.maps[m * plane + p + c] : 0.0f;
    }
    __syncthreads();
    for (int o = tid; o < kLossRowOut; o += 256) {
        const int r = o / kTile, x = o % kTile;
#pragma unroll
        for (int q = 0; q < 9; ++q) s_row[q][o] = loss_window(&s_m[q][r * kLossHalo + x], 1);
    }
    __syncthreads();

    const int lx = tid & 15, ly = tid >> 4;
    const uint32_t px = (uint32_t)(x0 + kLossR + lx), py = (uint32_t)(y0 + kLossR + ly);
    if (px >= a.width || py >= a.height) return;
    const size_t p = (size_t)py * a.width + px;
    float iv[3];
    loss_composite(a, a.rgba[p], iv);
    float d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float g = a.target[p * 3 + c];
        const float* col = &s_row[c][ly * kTile + lx];
        const float ca = loss_window(col, kTile), cb = loss_window(col + 3 * kLossRowOut, kTile);
        const float ce = loss_window(col + 6 * kLossRowOut, kTile);
        const float diff = iv[c] - g;
        const float sign = diff > 0.0f ? 1.0f : (diff < 0.0f ? -1.0f : 0.0f);
        d[c] = (ca + ((2.0f * diff) * cb + g * ce)) + a.l1_scale * sign;
    }
    float da = 0.0f;
    if (a.has_bg) da = -((a.bg[0] * d[0] + a.bg[1] * d[1]) + a.bg[2] * d[2]);
    a.grad[p] = make_float4(d[0], d[1], d[2], da);
}

void launch_photometric_loss(const LossBuffers& lb, const float* rgba, const float* target, float lambda, const float* bg,
                             uint32_t width, uint32_t height, float* loss_out, float* grad, hipStream_t stream) {
    LossArgs a{};
    a.rgba = reinterpret_cast<const float4*>(rgba);
    a.target = target;
    a.maps = lb.maps;
    a.tile_sums = reinterpret_cast<float2*>(lb.tile_sums);
    a.grad = reinterpret_cast<float4*>(grad);
    a.loss_out = loss_out;
    a.width = width; a.height = height;
    a.grid_w = (width + kTile - 1) / kTile;
    a.tiles = a.grid_w * ((height + kTile - 1) / kTile);
    a.has_bg = bg ? 1u : 0u;
    for (int c = 0; c < 3; ++c) a.bg[c] = bg ? bg[c] : 0.0f;
    const double count = 3.0 * (double)width * (double)height;
    a.lambda = lambda;
    a.ssim_scale = (float)(-(double)lambda / count);
    a.l1_scale = (float)((1.0 - (double)lambda) / count);
    a.inv_count = 1.0 / count;
    hipLaunchKernelGGL(k_loss_forward, dim3(a.tiles), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(k_loss_reduce, dim3(1), dim3(1024), 0, stream, a);
    if (grad) hipLaunchKernelGGL(k_loss_backward, dim3(a.tiles), dim3(256), 0, stream, a);
}

size_t loss_map_bytes(uint32_t width, uint32_t height) { return (size_t)width * height * 9 * sizeof(float); }
size_t loss_tile_bytes(uint32_t width, uint32_t height) {
    return (size_t)((width + kTile - 1) / kTile) * ((height + kTile - 1) / kTile) * 2 * sizeof(float);
}

} // namespace gs
