// gs_mcmc.hip -- the MCMC strategy on the device (include/gsplat.h, no reference counterpart):
//   the sampler             : w(g) from the record's opacity, its 64-bit exclusive prefix sums as (per block of 256 splats)
//                   a 64-bit block prefix + a 32-bit sum inside the block -- k_mcmc_block_sums, then k_mcmc_scan_blocks, one
//                   workgroup in the pattern of k_splat_scan_blocks -- and a draw per thread: a counter-based 64-bit word,
//                   its 128-bit product with the total, a binary search over the block prefixes and one inside the block;
//                   cnt[src] += 1 with integer atomics.  Integer sums throughout: the same bits for every launch shape;
//   gs_relocate_device      : a draw per dead splat; the per-splat scan of gs_splat_scan.h over (changed, dead, source) gives
//                   ids_out and the counts; k_reloc_values rewrites the sources (a lane per splat), k_reloc_copy moves their
//                   rows onto the dead ones (a lane per (splat, quad)) -- two launches, since a dead row is never a source;
//   gs_grow_device          : n_add draws; the scan over 1 + cnt gives o(g); k_grow_values writes the two changed quads of
//                   a source into its first output, k_grow_write copies everything else and repeats those quads.  The 21
//                   lanes of a source write its 1 + cnt rows one after another: with few alive splats and a large n_add
//                   (one alive splat, 10^6 copies) the growth is serial on one wave -- correct, slow, and no shape of training;
//   gs_position_noise_device: k_position_noise, a lane per listed row.
// No float atomics, nothing read back by the host: all three calls are bitwise reproducible.
#include "gs_splat_math.h"
#include "gs_splat_scan.h"

#include <cmath>

namespace gs {

void mcmc_fill_tables(float* t) {
    uint64_t binom[kMcmcMaxRatio][kMcmcMaxRatio];      // C(50, 25) = 1.3e14: exact in 64 bits
    for (uint32_t a = 0; a < kMcmcMaxRatio; ++a)
        for (uint32_t b = 0; b < kMcmcMaxRatio; ++b) {
            binom[a][b] = b > a ? 0u : (b == 0u || b == a ? 1u : binom[a - 1][b - 1] + binom[a - 1][b]);
            t[a * kMcmcMaxRatio + b] = (float)binom[a][b];
        }
    for (uint32_t k = 0; k < kMcmcMaxRatio; ++k) t[kMcmcMaxRatio * kMcmcMaxRatio + k] = (float)(1.0 / std::sqrt((double)(k + 1u)));
}

namespace {

// ---- the sampler ----------------------------------------------------------------------------------------------------

// alive(g) and w(g) of the header, every comparison as it writes them: a NaN opacity is dead
__device__ __forceinline__ uint32_t mcmc_weight(const float* __restrict__ records, uint32_t g, float min_opacity) {
    const float o = records[(size_t)g * kRecordFloats + kRecOpacity];
    if (!(o > min_opacity)) return 0u;
    return (uint32_t)((o < 1.0f ? o : 1.0f) * 16777216.0f);       // min_opacity >= 2^-24: at least 1
}

// within[g], the block's sum, and cnt[g] = 0
__global__ __launch_bounds__(256) void k_mcmc_block_sums(const float* __restrict__ records, uint32_t n, float min_opacity,
                                                          McmcScratch s) {
    __shared__ uint32_t s_w[4];
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    const uint32_t w = g < n ? mcmc_weight(records, g, min_opacity) : 0u;
    const uint32_t inc = wave_inclusive_scan(w);                  // <= 64 * 2^24
    if (lane_id() == 63) s_w[wave_id()] = inc;
    __syncthreads();
    uint32_t before = inc - w;
    for (int k = 0; k < wave_id(); ++k) before += s_w[k];         // <= 255 * 2^24
    if (g < n) {
        s.within[g] = before;
        s.cnt[g] = 0u;
    }
    if (threadIdx.x == 0u) s.block_sums[blockIdx.x] = ((uint64_t)s_w[0] + s_w[1]) + ((uint64_t)s_w[2] + s_w[3]);
}

// One workgroup, every thread owning per = ceil(blocks / 1024) consecutive blocks: block_prefix[b] for b < blocks, and the
// total in block_prefix[blocks]
__global__ __launch_bounds__(1024) void k_mcmc_scan_blocks(const uint64_t* __restrict__ block_sums, uint32_t blocks,
                                                            uint64_t* __restrict__ block_prefix) {
    __shared__ uint64_t s_w[16];
    const uint32_t per = (blocks + 1023u) / 1024u;
    const uint32_t b0 = threadIdx.x * per;
    uint64_t mine = 0;
    for (uint32_t k = 0; k < per; ++k)
        if (b0 + k < blocks) mine += block_sums[b0 + k];
    const uint64_t inc = wave_inclusive_scan64(mine);
    if (lane_id() == 63) s_w[wave_id()] = inc;
    __syncthreads();
    uint64_t run = inc - mine;
    for (int w = 0; w < wave_id(); ++w) run += s_w[w];
    for (uint32_t k = 0; k < per; ++k) {
        if (b0 + k < blocks) {
            block_prefix[b0 + k] = run;
            run += block_sums[b0 + k];
        }
    }
    if (threadIdx.x == 1023u) block_prefix[blocks] = run;
}

// The source of draw i: the one g with P(g) <= t < P(g) + w(g).  total > 0.
__device__ __forceinline__ uint32_t mcmc_draw(uint32_t i, uint64_t seed, uint64_t total, const McmcScratch& s, uint32_t n,
                                              uint32_t blocks) {
    const uint32_t h = mix32(mix32(i ^ (uint32_t)seed) + (uint32_t)(seed >> 32));
    const uint64_t r64 = ((uint64_t)mix32(h + 0x9E3779B9u) << 32) | mix32(h + 2u * 0x9E3779B9u);
    const uint64_t t = __umul64hi(r64, total);                    // [0, total)
    uint32_t lo = 0u, hi = blocks;                                // block_prefix[lo] <= t; the block lies in [lo, hi)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (s.block_prefix[mid] <= t) lo = mid; else hi = mid;
    }
    const uint32_t rem = (uint32_t)(t - s.block_prefix[lo]);      // below the block's sum, at most 2^32 - 1
    uint32_t a = lo * 256u, b = n - a < 256u ? n : a + 256u;      // within[a] == 0 <= rem; the splat lies in [a, b)
    while (b - a > 1u) {
        const uint32_t mid = a + (b - a) / 2u;
        if (s.within[mid] <= rem) a = mid; else b = mid;
    }
    return a;
}

// gs_relocate_device: every dead d makes draw d
__global__ __launch_bounds__(256) void k_mcmc_draw_dead(const McmcArgs a, uint32_t blocks) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.n) return;
    if (mcmc_weight(a.records, g, a.min_opacity) != 0u) { a.s.src_of[g] = kMcmcAlive; return; }
    const uint64_t total = a.s.block_prefix[blocks];
    if (total == 0u) { a.s.src_of[g] = kMcmcDeadNoDraw; return; }
    const uint32_t src = mcmc_draw(g, a.seed, total, a.s, a.n, blocks);
    atomicAdd(a.s.cnt + src, 1u);
    a.s.src_of[g] = src;
}

// gs_grow_device: draws 0 .. n_add - 1
__global__ __launch_bounds__(256) void k_mcmc_draw_add(const McmcArgs a, uint32_t n_add, uint32_t blocks) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_add) return;
    const uint64_t total = a.s.block_prefix[blocks];
    if (total == 0u) return;
    atomicAdd(a.s.cnt + mcmc_draw(i, a.seed, total, a.s, a.n, blocks), 1u);
}

// ---- the relocation values ------------------------------------------------------------------------------------------

struct RelocValues {
    float o, s[3];            // what the record stores
    float raw_o, raw_s[3];    // RAW: what raw stores
};

// The header's expressions in the header's order, for a source drawn cnt > 0 times
template <bool RAW>
__device__ __forceinline__ RelocValues reloc_values(float o, float s0, float s1, float s2, uint32_t cnt, float min_opacity,
                                                    const float* __restrict__ tables) {
    const float* B = tables;
    const float* Q = tables + kMcmcMaxRatio * kMcmcMaxRatio;
    const uint32_t r = cnt + 1u < kMcmcMaxRatio ? cnt + 1u : kMcmcMaxRatio;
    const float top = 0x1.fffffep-1f;
    const float o1 = -expm1f(log1pf(-(o < top ? o : top)) / (float)r);
    const float oc = o1 < min_opacity ? min_opacity : (o1 > top ? top : o1);
    RelocValues out;
    out.raw_o = 0.0f;
    out.o = oc;
    if (RAW) {
        out.raw_o = logit_opacity(oc);
        out.o = sigmoid_pinned(out.raw_o);
    }
    const float op = out.o;
    float D = 0.0f;
    for (uint32_t i = 1u; i <= r; ++i) {
        float p = op, sg = 1.0f;
        for (uint32_t k = 0u; k < i; ++k) {
            D = D + B[(i - 1u) * kMcmcMaxRatio + k] * ((sg * Q[k]) * p);
            p = p * op;
            sg = -sg;
        }
    }
    const float c = o / D;
    const float s[3] = {s0, s1, s2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out.s[k] = c * s[k];
        out.raw_s[k] = 0.0f;
        if (RAW) {
            out.raw_s[k] = log_scale(out.s[k]);
            out.s[k] = exp_pinned(out.raw_s[k]);
        }
    }
    return out;
}

__device__ __forceinline__ RelocValues reloc_values_of(const float* __restrict__ rec, bool raw, uint32_t cnt, float min_opacity,
                                                       const float* __restrict__ tables) {
    const float o = rec[kRecOpacity], s0 = rec[kRecScale], s1 = rec[kRecScale + 1], s2 = rec[kRecScale + 2];
    return raw ? reloc_values<true>(o, s0, s1, s2, cnt, min_opacity, tables)
               : reloc_values<false>(o, s0, s1, s2, cnt, min_opacity, tables);
}

// ---- gs_relocate_device ---------------------------------------------------------------------------------------------

// The rows of the scan: changed (its exclusive sum is the row's place in ids_out), dead, source
struct RelocSource {
    static constexpr uint32_t K = 3u, kPlaced = 1u, kTotalsFrom = 0u;
    const uint32_t* cnt;
    const uint32_t* src_of;
    __device__ void counts(uint32_t g, uint32_t (&c)[K]) const {
        const uint32_t so = src_of[g];
        c[2] = cnt[g] != 0u ? 1u : 0u;
        c[1] = so != kMcmcAlive ? 1u : 0u;
        c[0] = so < kMcmcDeadNoDraw ? 1u : c[2];
    }
};

__global__ __launch_bounds__(256) void k_reloc_ids(const McmcArgs a, uint32_t* __restrict__ ids_out, uint32_t max_rows) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.n) return;
    if (a.s.src_of[g] >= kMcmcDeadNoDraw && a.s.cnt[g] == 0u) return;
    const uint32_t at = a.scan.offsets[g];
    if (at < max_rows) ids_out[at] = g;
}

// A lane per splat: a source gets its new opacity and scales, in records and in raw
__global__ __launch_bounds__(256) void k_reloc_values(const McmcArgs a) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.n) return;
    const uint32_t cnt = a.s.cnt[g];
    if (cnt == 0u) return;
    float* rec = a.records + (size_t)g * kRecordFloats;
    const RelocValues v = reloc_values_of(rec, a.raw != nullptr, cnt, a.min_opacity, a.s.tables);
    rec[kRecScale] = v.s[0]; rec[kRecScale + 1] = v.s[1]; rec[kRecScale + 2] = v.s[2];
    rec[kRecOpacity] = v.o;
    if (a.raw) {
        float* raw = a.raw + (size_t)g * kRecordFloats;
        raw[kRecScale] = v.raw_s[0]; raw[kRecScale + 1] = v.raw_s[1]; raw[kRecScale + 2] = v.raw_s[2];
        raw[kRecOpacity] = v.raw_o;
    }
}

// A lane per (splat g, group q of four floats): a dead g that drew receives the row of its source as k_reloc_values left it;
// the moment rows of both become zero.  A dead row is never a source, so no lane reads what another writes.
template <bool MOMENTS>
__global__ __launch_bounds__(256) void k_reloc_copy(const McmcArgs a) {
    const uint64_t item = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t g = (uint32_t)(item / kRecordQuads), q = (uint32_t)(item % kRecordQuads);
    if (g >= a.n) return;
    const uint32_t so = a.s.src_of[g];
    const bool copy = so < kMcmcDeadNoDraw;
    if (!copy && a.s.cnt[g] == 0u) return;
    if (copy) {
        const size_t from = (size_t)so * kRecordQuads + q;
        reinterpret_cast<float4*>(a.records)[item] = reinterpret_cast<const float4*>(a.records)[from];
        if (a.raw) reinterpret_cast<float4*>(a.raw)[item] = reinterpret_cast<const float4*>(a.raw)[from];
    }
    if (MOMENTS) {
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        reinterpret_cast<float4*>(a.m)[item] = zero4;
        reinterpret_cast<float4*>(a.v)[item] = zero4;
    }
}

// ---- gs_grow_device -------------------------------------------------------------------------------------------------

struct GrowOut {
    float *records, *raw, *m, *v;
    uint32_t max_out;
};

// The rows of the scan: the outputs 1 + cnt(g), whose exclusive sum is o(g), and the flag source.  The draws number
// n_add, so the outputs number n + n_add < 2^31: nothing saturates.
struct GrowSource {
    static constexpr uint32_t K = 2u, kPlaced = 1u, kTotalsFrom = 0u;
    const uint32_t* cnt;
    __device__ void counts(uint32_t g, uint32_t (&c)[K]) const {
        const uint32_t k = cnt[g];
        c[0] = 1u + k;
        c[1] = k != 0u ? 1u : 0u;
    }
};

// A lane per splat: the scale quad and the SH-DC quad of a source, with the relocation values, into its first output
__global__ __launch_bounds__(256) void k_grow_values(const McmcArgs a, const GrowOut out) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.n) return;
    const uint32_t cnt = a.s.cnt[g];
    if (cnt == 0u) return;
    const uint32_t o = a.scan.offsets[g];
    if (o >= out.max_out) return;
    const float* rec = a.records + (size_t)g * kRecordFloats;
    const RelocValues v = reloc_values_of(rec, a.raw != nullptr, cnt, a.min_opacity, a.s.tables);
    float4* to = reinterpret_cast<float4*>(out.records) + (size_t)o * kRecordQuads;
    to[kQuadScale] = make_float4(v.s[0], v.s[1], v.s[2], rec[kRecScale + 3]);
    to[kQuadDc] = make_float4(rec[kRecSh], rec[kRecSh + 1], rec[kRecSh + 2], v.o);
    if (a.raw) {
        const float* raw = a.raw + (size_t)g * kRecordFloats;
        float4* rto = reinterpret_cast<float4*>(out.raw) + (size_t)o * kRecordQuads;
        rto[kQuadScale] = make_float4(v.raw_s[0], v.raw_s[1], v.raw_s[2], raw[kRecScale + 3]);
        rto[kQuadDc] = make_float4(raw[kRecSh], raw[kRecSh + 1], raw[kRecSh + 2], v.raw_o);
    }
}

// A lane per (input splat g, group q of four floats), like k_dens_write: the lanes of g write group q of its 1 + cnt(g)
// outputs, rows o(g) .. o(g) + cnt(g), while they are below max_out.  The two quads k_grow_values wrote into row o(g) of a
// source are read there and repeated in its other rows.
template <bool MOMENTS>
__global__ __launch_bounds__(256) void k_grow_write(const McmcArgs a, const GrowOut out) {
    const uint64_t item = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t g = (uint32_t)(item / kRecordQuads), q = (uint32_t)(item % kRecordQuads);
    if (g >= a.n) return;
    const uint32_t cnt = a.s.cnt[g], o = a.scan.offsets[g];
    if (o >= out.max_out) return;
    const size_t first = (size_t)o * kRecordQuads + q;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool valued = cnt != 0u && (q == kQuadScale || q == kQuadDc);
    float4 rec, raw = zero4, mm = zero4, vv = zero4;
    if (valued) {
        rec = reinterpret_cast<const float4*>(out.records)[first];
        if (a.raw) raw = reinterpret_cast<const float4*>(out.raw)[first];
    } else {
        rec = reinterpret_cast<const float4*>(a.records)[item];
        if (a.raw) raw = reinterpret_cast<const float4*>(a.raw)[item];
    }
    if (MOMENTS && cnt == 0u) {        // a row nobody drew: the moments travel with the record
        mm = reinterpret_cast<const float4*>(a.m)[item];
        vv = reinterpret_cast<const float4*>(a.v)[item];
    }
    for (uint32_t j = 0u; j <= cnt; ++j) {             // o + cnt < 2^31
        if (o + j >= out.max_out) break;
        const size_t at = first + (size_t)j * kRecordQuads;
        if (!valued || j != 0u) {
            reinterpret_cast<float4*>(out.records)[at] = rec;
            if (a.raw) reinterpret_cast<float4*>(out.raw)[at] = raw;
        }
        if (MOMENTS) {
            reinterpret_cast<float4*>(out.m)[at] = mm;
            reinterpret_cast<float4*>(out.v)[at] = vv;
        }
    }
}

// ---- gs_position_noise_device ---------------------------------------------------------------------------------------

// Thread i < min(*count, max_rows) handles g = ids[i] (an id >= n is skipped); LISTED == false: g = i < n
template <bool LISTED>
__global__ __launch_bounds__(256) void k_position_noise(float* __restrict__ records, float* __restrict__ raw, uint32_t n,
                                                         const uint32_t* __restrict__ ids, const uint32_t* __restrict__ count,
                                                         uint32_t max_rows, float scale, float gate_k, float gate_x0,
                                                         uint64_t seed) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t g = i;
    if (LISTED) {
        const uint32_t listed = *count, rows = listed < max_rows ? listed : max_rows;
        if (i >= rows) return;
        g = ids[i];
    }
    if (g >= n) return;
    float* p = records + (size_t)g * kRecordFloats;
    const float s[3] = {p[kRecScale], p[kRecScale + 1], p[kRecScale + 2]};
    const Mat3 rm = get_rot_mat(p[kRecRot], p[kRecRot + 1], p[kRecRot + 2], p[kRecRot + 3]);   // R[row][col] = rm.m[col][row]
    const uint32_t h = mix32(mix32(g ^ (uint32_t)seed) + (uint32_t)(seed >> 32));
    const float z[3] = {densify_normal(h, 0u, 0u), densify_normal(h, 0u, 1u), densify_normal(h, 0u, 2u)};
    const float gate = sigmoid_pinned(gate_k * ((1.0f - p[kRecOpacity]) - gate_x0));
    float ak[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) ak[k] = s[k] * ((rm.m[k][0] * z[0] + rm.m[k][1] * z[1]) + rm.m[k][2] * z[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float off = ((rm.m[0][r] * s[0]) * ak[0] + (rm.m[1][r] * s[1]) * ak[1]) + (rm.m[2][r] * s[2]) * ak[2];
        const float pos = p[kRecPos + r] + (off * gate) * scale;
        p[kRecPos + r] = pos;
        if (raw) raw[(size_t)g * kRecordFloats + kRecPos + r] = pos;
    }
}

// block sums, block scan: what both samplers run first (n < 2^31)
void launch_mcmc_prefix(const McmcArgs& a, hipStream_t stream) {
    const uint32_t blocks = backward_blocks(a.n);
    hipLaunchKernelGGL(k_mcmc_block_sums, dim3(blocks), dim3(256), 0, stream, a.records, a.n, a.min_opacity, a.s);
    hipLaunchKernelGGL(k_mcmc_scan_blocks, dim3(1), dim3(1024), 0, stream, a.s.block_sums, blocks, a.s.block_prefix);
}

}  // namespace

void launch_relocate(const McmcArgs& a, uint32_t* ids_out, uint32_t max_rows, uint32_t* counts_out, hipStream_t stream) {
    const uint32_t blocks = backward_blocks(a.n);
    launch_mcmc_prefix(a, stream);
    hipLaunchKernelGGL(k_mcmc_draw_dead, dim3(blocks), dim3(256), 0, stream, a, blocks);
    launch_splat_scan(RelocSource{a.s.cnt, a.s.src_of}, a.n, a.scan, counts_out, stream);
    if (max_rows) hipLaunchKernelGGL(k_reloc_ids, dim3(blocks), dim3(256), 0, stream, a, ids_out, max_rows);
    hipLaunchKernelGGL(k_reloc_values, dim3(blocks), dim3(256), 0, stream, a);
    const uint64_t wblocks = ((uint64_t)a.n * kRecordQuads + 255u) / 256u;       // < 2^28 for n < 2^31
    if (a.m) hipLaunchKernelGGL(k_reloc_copy<true>, dim3((uint32_t)wblocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k_reloc_copy<false>, dim3((uint32_t)wblocks), dim3(256), 0, stream, a);
}

void launch_grow(const McmcArgs& a, uint32_t n_add, float* records_out, float* raw_out, float* m_out, float* v_out,
                 uint32_t max_out, uint32_t* counts_out, hipStream_t stream) {
    const uint32_t blocks = backward_blocks(a.n);
    launch_mcmc_prefix(a, stream);
    if (n_add) hipLaunchKernelGGL(k_mcmc_draw_add, dim3(backward_blocks(n_add)), dim3(256), 0, stream, a, n_add, blocks);
    launch_splat_scan(GrowSource{a.s.cnt}, a.n, a.scan, counts_out, stream);
    if (max_out == 0) return;
    const GrowOut out{records_out, raw_out, m_out, v_out, max_out};
    if (n_add) hipLaunchKernelGGL(k_grow_values, dim3(blocks), dim3(256), 0, stream, a, out);
    const uint64_t wblocks = ((uint64_t)a.n * kRecordQuads + 255u) / 256u;       // < 2^28 for n < 2^31
    if (a.m) hipLaunchKernelGGL(k_grow_write<true>, dim3((uint32_t)wblocks), dim3(256), 0, stream, a, out);
    else hipLaunchKernelGGL(k_grow_write<false>, dim3((uint32_t)wblocks), dim3(256), 0, stream, a, out);
}

void launch_position_noise(float* records, float* raw, uint32_t n, const uint32_t* ids, const uint32_t* count, uint32_t max_rows,
                           float scale, float gate_k, float gate_x0, uint64_t seed, hipStream_t stream) {
    if (ids) {
        if (max_rows == 0) return;
        const uint64_t blocks = ((uint64_t)max_rows + 255u) / 256u;              // < 2^24 for every uint32 max_rows
        hipLaunchKernelGGL(k_position_noise<true>, dim3((uint32_t)blocks), dim3(256), 0, stream, records, raw, n, ids, count,
                           max_rows, scale, gate_k, gate_x0, seed);
    } else {
        hipLaunchKernelGGL(k_position_noise<false>, dim3(backward_blocks(n)), dim3(256), 0, stream, records, raw, n, ids, count,
                           max_rows, scale, gate_k, gate_x0, seed);
    }
}

}  // namespace gs
