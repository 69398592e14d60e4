// gs_sort_words.h -- what the 4-bit sorter (gs_sort.hip) and the 8-bit sorter (gs_sort8.hip) share: how the two or
// three words of a sort element are staged in LDS, unstaged and written, how Count reads the one word its digit lives
// in, which group a Scatter workgroup takes next, and the host-side choice of the kernel instantiation of a pass.
//
// An element is (depth word `lo`, tile word `hi`, gaussian index `id`), stored SoA.  The id is always 32 bits wide.
// LO_IN / LO_OUT = bytes of the depth word a pass reads / writes per element (4, 2 or 0).  The stand-alone sorter
// (gs_sort_host) and GS_SORT_TILE_BUCKET use <4, 4>: everything moves.  In a frame the depth word is needed only as a
// sort key -- FindRanges reads the tile words, RenderGaussians the ids, gs_debug_read rebuilds the sorted depth
// words from the ids -- so bits a pass has consumed are dead weight and are dropped (SortRun::drop_depth_payload):
//   4-bit digits: passes 0-2 run <4, 4>, pass 3 writes only the upper half <4, 2>, passes 4-6 sort on that half
//                 <2, 2>, pass 7 (last depth digit) does not write it <2, 0>, the tile-word passes run <0, 0>;
//   8-bit digits: pass 0 <4, 4>, pass 1 <4, 2>, pass 2 <2, 2>, pass 3 <2, 0>, the tile-word passes <0, 0>.
// sort_pass() (gs_internal.h) derives the pair of a pass; with_word_layout() below turns it into template arguments.
// HI16: the tile words are 16-bit compact tile ids (at most 65535 owned tiles): 2 bytes less read and 2 less written
// per element in every pass.
// PK_IN / PK_OUT (SortRun::packed; kPk* of gs_internal.h): the depth passes never look at the payload, so with 16-bit
// tile ids and at most 2^24 splats the 4-bit sorter of a frame carries it in 5 bytes instead of 6:
//   pk32 = tile16 << 16 | (id & 0xFFFF) in the id plane, pk8 = id >> 16 in a byte plane that uses the storage of the
//   tile words (kPkPlane) or, as soon as a pass has consumed that byte, in the lowest byte of the stored depth word
//   (kPkWord).  Count reads the same word at the same shift either way.  Bytes per element read -> written:
//     k_emit -> 9 | pass 0  9 -> 9 <4, 4, plane, plane> | pass 1  9 -> 8 <4, 4, plane, word> | pass 2  8 -> 8 <4, 4, word, word>
//     pass 3  8 -> 7 <4, 2, word, plane> | pass 4  7 -> 7 <2, 2, plane, plane> | pass 5  7 -> 6 <2, 2, plane, word>
//     pass 6  6 -> 6 <2, 2, word, word>  | pass 7  6 -> 6 <2, 0, word, none>: tile u16 + id u32, what every later stage reads
//   117 bytes per element over the eight depth passes where the unpacked layouts move 140.  A fed run (SortRun::fed:
//   short lists, every launch bound by latency) does not use the byte plane beside a 16-bit depth word: pass 3 unpacks
//   <4, 2, word, none>, pass 4 runs unpacked <2, 2, none, none>, pass 5 packs again <2, 2, none, word> (121 bytes).
//   Everything else -- more than 65535 owned tiles, more than 2^24 splats, a frame with per-pass timers (record_timings
//   >= 2, frame_packs_payload()), the stand-alone sorter, the other sorters -- stays unpacked (sort_pass() decides; a
//   GS_SORT_PACKED_PAYLOAD=0 build never packs).
// FULL: the group holds all its keys (every group but the last): no per-element bounds logic.
#pragma once

#include "gs_internal.h"

#include <type_traits>

namespace gs {

// The keys of a pass are read once: non-temporal loads keep them from displacing the partly written destination lines
// in L2, which neighbouring groups are about to complete (config C's RadixSort 0.590 -> 0.552 ms, config D's 1.59 ->
// 1.33 with the 4-bit passes; DESIGN.md section 4.1.  Non-temporal STORES, or such loads in Count, cost 10-80 %).
// The striped loads of lo / hi / id themselves stay in scatter_group and scatter8_group, and so does the loop around
// xcd_group below: as helpers here (the arrays by reference or word by word, the loop with its body as a lambda) they
// cost nothing in the source but make the compiler order the code of every Scatter kernel differently.
#define GS_KEY_LOAD(p) __builtin_nontemporal_load(p)

// ---- Count: a wave takes kCountChunk keys per step, 32 per lane, with 16-byte loads of the word the digit lives in.
// W16: that word is stored as 16 bits (SortPass::word16).
constexpr int kCountChunk = 2048;
constexpr int kCountKeysPerLane = kCountChunk / 64;

template <bool W16>
struct CountRegs { uint4 v[kCountKeysPerLane / (W16 ? 8 : 4)]; };

template <bool W16>
__device__ __forceinline__ void count_load(const uint32_t* __restrict__ word, uint32_t first_key, uint32_t e, int lane,
                                           CountRegs<W16>& k) {
    constexpr int V = kCountKeysPerLane / (W16 ? 8 : 4);
    constexpr uint32_t PER = W16 ? 8u : 4u;          // keys per 16-byte load
    if (first_key + kCountChunk <= e) {
        const uint4* w4 = W16 ? reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(word) + first_key)
                              : reinterpret_cast<const uint4*>(word + first_key);
#pragma unroll
        for (int r = 0; r < V; ++r) k.v[r] = w4[r * 64 + lane];
    } else {   // ragged end of the list: element-wise; keys past the end are skipped by the bounds test of the count
#pragma unroll
        for (int r = 0; r < V; ++r) {
            const uint32_t i0 = first_key + (uint32_t)(r * 64 + lane) * PER;
            uint32_t w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if constexpr (W16) {
                    const uint16_t* h = reinterpret_cast<const uint16_t*>(word);
                    const uint32_t i = i0 + 2u * (uint32_t)q;
                    w[q] = (i < e ? (uint32_t)h[i] : 0u) | ((i + 1u < e ? (uint32_t)h[i + 1u] : 0u) << 16);
                } else {
                    w[q] = i0 + (uint32_t)q < e ? word[i0 + q] : 0u;
                }
            }
            k.v[r] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
}

// ---- Scatter: the element's way through a workgroup.
// Bit offset of the digit at key bit `shift` inside the word as a pass with LO_IN depth bytes holds it (sort_pass()
// computes the same number for Count: SortPass::word_shift).
template <int LO_IN>
__device__ __forceinline__ uint32_t word_shift_of(uint32_t shift) {
    return shift >= 32u ? shift - 32u : (LO_IN == 2 ? shift - 16u : shift);
}

// LDS staging: one 8-byte slot {id, word} per element.  Nothing travels beside it when the element is id + one 32-bit
// word (tile-word passes; depth passes whose depth and tile words are both 16 bits wide), else the tile word does,
// in s_third.
// Packed payload (PK_IN != kPkNone, HI16 only; the header comment): the slot is {pk32, depth word as stored}; pk8 is
// part of that word (kPkWord), sits beside a 16-bit depth word in the slot (kPkPlane, LO_IN == 2) or travels in
// s_third, one byte wide (kPkPlane, LO_IN == 4).  In registers `hi` carries pk8 of a kPkPlane element.
template <bool HI16, int PK_IN = kPkNone>
using third_word = typename std::conditional<PK_IN != kPkNone, uint8_t,
                                             typename std::conditional<HI16, uint16_t, uint32_t>::type>::type;
constexpr bool has_third(int lo_in, bool hi16, int pk_in = kPkNone) {
    return pk_in != kPkNone ? (pk_in == kPkPlane && lo_in == 4) : (lo_in == 4 || (lo_in == 2 && !hi16));
}

template <int LO_IN, bool HI16, int PK_IN = kPkNone>
__device__ __forceinline__ void stage_elem(uint2* s_slot, third_word<HI16, PK_IN>* s_third, uint32_t p, uint32_t id,
                                           uint32_t lo, uint32_t hi) {
    if constexpr (PK_IN == kPkWord) s_slot[p] = make_uint2(id, lo);
    else if constexpr (LO_IN == 0) s_slot[p] = make_uint2(id, hi);
    else if constexpr (!has_third(LO_IN, HI16, PK_IN)) s_slot[p] = make_uint2(id, lo | (hi << 16));
    else { s_slot[p] = make_uint2(id, lo); s_third[p] = (third_word<HI16, PK_IN>)hi; }
}

// -> the id (packed: pk32); l, h = the depth and tile words as loaded (packed: h = pk8)
template <int LO_IN, bool HI16, int PK_IN = kPkNone>
__device__ __forceinline__ uint32_t unstage_elem(const uint2* s_slot, const third_word<HI16, PK_IN>* s_third, uint32_t p,
                                                 uint32_t& l, uint32_t& h) {
    const uint2 sl = s_slot[p];
    if constexpr (PK_IN == kPkWord) { l = sl.y; h = sl.y & 0xFFu; }
    else if constexpr (LO_IN == 0) { l = 0u; h = sl.y; }
    else if constexpr (!has_third(LO_IN, HI16, PK_IN)) { l = sl.y & 0xFFFFu; h = sl.y >> 16; }
    else { l = sl.y; h = s_third[p]; }
    return sl.x;
}

// Element to index o of the destination; <4, 2> keeps the upper half of the depth word.  Packed: pk8 goes to the byte
// plane (the storage of out_hi) or over the consumed low byte of the depth word written.  A pass may unpack (PK_OUT ==
// kPkNone: the 16-bit tile word and the 32-bit splat index, as the last depth pass writes them) or pack what it read
// unpacked (PK_IN == kPkNone; a fed run does both, sort_pass()).
template <int LO_IN, int LO_OUT, bool HI16, int PK_IN = kPkNone, int PK_OUT = kPkNone>
__device__ __forceinline__ void store_elem(uint32_t* out_lo, uint32_t* out_hi, uint32_t* out_id, uint32_t o,
                                           uint32_t id, uint32_t l, uint32_t h) {
    if constexpr (PK_IN != kPkNone || PK_OUT != kPkNone) {
        static_assert(HI16, "the packed payload holds a 16-bit tile id");
        const uint32_t w = LO_IN == 4 && LO_OUT == 2 ? l >> 16 : l;          // the depth word in its width of the output
        const uint32_t pk32 = PK_IN != kPkNone ? id : (h << 16) | (id & 0xFFFFu);
        const uint32_t pk8 = PK_IN != kPkNone ? h : (id >> 16) & 0xFFu;
        if constexpr (PK_OUT == kPkWord) {
            static_assert(LO_OUT == LO_IN && LO_OUT != 0, "pk8 replaces the low byte of a word that keeps its width");
            if constexpr (LO_OUT == 4) out_lo[o] = (w & 0xFFFFFF00u) | pk8;
            else reinterpret_cast<uint16_t*>(out_lo)[o] = (uint16_t)((w & 0xFF00u) | pk8);
            out_id[o] = pk32;
        } else if constexpr (PK_OUT == kPkPlane) {
            if constexpr (LO_OUT == 4) out_lo[o] = w;
            else reinterpret_cast<uint16_t*>(out_lo)[o] = (uint16_t)w;
            reinterpret_cast<uint8_t*>(out_hi)[o] = (uint8_t)pk8;
            out_id[o] = pk32;
        } else {
            if constexpr (LO_OUT == 4) out_lo[o] = w;
            else if constexpr (LO_OUT == 2) reinterpret_cast<uint16_t*>(out_lo)[o] = (uint16_t)w;
            reinterpret_cast<uint16_t*>(out_hi)[o] = (uint16_t)(pk32 >> 16);
            out_id[o] = (pk8 << 16) | (pk32 & 0xFFFFu);
        }
    } else {
        if constexpr (LO_OUT == 4) out_lo[o] = l;
        else if constexpr (LO_OUT == 2) reinterpret_cast<uint16_t*>(out_lo)[o] = (uint16_t)(LO_IN == 4 ? l >> 16 : l);
        if constexpr (HI16) reinterpret_cast<uint16_t*>(out_hi)[o] = (uint16_t)h;
        else out_hi[o] = h;
        out_id[o] = id;
    }
}

// The walk of a Scatter workgroup over the groups: virtual blocks vb = blockIdx.x, + gridDim.x, ... below 8 per_xcd,
// per_xcd = ceil(G / 8); xcd_group(vb, per_xcd) is the group of vb (from G on: none).  One group per workgroup as a
// rule: the grid (scatter_grid) comes from an upper estimate of the element count, and a workgroup walks on only if a
// frame exceeds it; surplus workgroups leave at once.
// Workgroups b, b + 8, ... share an XCD (observed placement, speed only): each of the eight takes a contiguous run of
// the groups, so that the digit runs of neighbouring groups -- neighbours in the destination too -- meet in one L2
// and leave it as whole lines.
__device__ __forceinline__ uint32_t xcd_group(uint32_t vb, uint32_t per_xcd) { return (vb & 7u) * per_xcd + (vb >> 3); }

// ---- host side
// Workgroups of a Scatter launch over groups of `tile` keys.  A context that owns a share of the tiles (tile-row band
// of a multi-GPU frame) launches over twice that share of the capacity's groups; the workgroups walk on (xcd_group)
// if a frame should hold more.
inline uint32_t scatter_grid(const SortRun& run, uint32_t tile) {
    uint32_t max_groups = (run.capacity + tile - 1) / tile;
    if (run.share < 0.5f) {
        const uint32_t g = (uint32_t)((float)max_groups * 2.0f * run.share) + 64u;
        max_groups = g < max_groups ? g : max_groups;
    }
    return max_groups;
}

// f(std::true_type{}) or f(std::false_type{}): a runtime choice as a template argument
template <class F>
inline void with_bool(bool b, F&& f) {
    if (b) f(std::true_type{}); else f(std::false_type{});
}

// f(LO_IN, LO_OUT, HI16, PK_IN, PK_OUT) as std::integral_constants, for the word layout of pass p
template <class F>
inline void with_word_layout(const SortPass& p, bool hi16, F&& f) {
    using I0 = std::integral_constant<int, 0>; using I2 = std::integral_constant<int, 2>;
    using I4 = std::integral_constant<int, 4>;
    using None = std::integral_constant<int, kPkNone>; using Plane = std::integral_constant<int, kPkPlane>;
    using Word = std::integral_constant<int, kPkWord>;
    if (p.pk_in != kPkNone || p.pk_out != kPkNone) {   // sort_pass() packs under hi16 alone, in these ten combinations
        const std::true_type h16{};
        const int in = p.pk_in, out = p.pk_out;
        if (p.lo_in == 4 && p.lo_out == 4) {
            if (in == kPkPlane && out == kPkPlane) f(I4{}, I4{}, h16, Plane{}, Plane{});
            else if (in == kPkPlane) f(I4{}, I4{}, h16, Plane{}, Word{});
            else f(I4{}, I4{}, h16, Word{}, Word{});
        } else if (p.lo_in == 4) {
            if (out == kPkPlane) f(I4{}, I2{}, h16, Word{}, Plane{});
            else f(I4{}, I2{}, h16, Word{}, None{});              // a fed run unpacks here ...
        } else if (p.lo_out == 2) {
            if (in == kPkPlane && out == kPkPlane) f(I2{}, I2{}, h16, Plane{}, Plane{});
            else if (in == kPkPlane) f(I2{}, I2{}, h16, Plane{}, Word{});
            else if (in == kPkNone) f(I2{}, I2{}, h16, None{}, Word{});   // ... and packs again here
            else f(I2{}, I2{}, h16, Word{}, Word{});
        } else f(I2{}, I0{}, h16, Word{}, None{});
        return;
    }
    auto pair = [&](auto lo_in, auto lo_out) { with_bool(hi16, [&](auto h16) { f(lo_in, lo_out, h16, None{}, None{}); }); };
    if (p.lo_in == 4 && p.lo_out == 4) pair(I4{}, I4{});
    else if (p.lo_in == 4 && p.lo_out == 2) pair(I4{}, I2{});
    else if (p.lo_in == 2 && p.lo_out == 2) pair(I2{}, I2{});
    else if (p.lo_in == 2 && p.lo_out == 0) pair(I2{}, I0{});
    else pair(I0{}, I0{});
}

} // namespace gs
