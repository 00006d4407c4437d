// step_mt.h -- numpy's MT19937 stream, the 624-word key in a wave's registers:
// load/store, the wave-parallel twist, tempering, the masked bounded draw.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "snake_internal.h"
#include "step_lanes.h"

namespace snake {

__device__ __forceinline__ uint32_t gen_mask(uint32_t m)
{
    m |= m >> 1; m |= m >> 2; m |= m >> 4; m |= m >> 8; m |= m >> 16;
    return m;
}

// ---------------------------------------------------------------- MT19937
// numpy legacy RandomState stream (mt19937_seed / mt19937_gen / tempering).
// The 624-word key lives in registers: lane l holds words 64t + l, t = 0..9.
struct WaveMT {
    uint32_t w[10];
    int pos;
};

__device__ __forceinline__ uint32_t temper(uint32_t y)
{
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
}

// m.w[t] for a wave-uniform runtime t. Masked ORs, not selects: InstCombine turns
// a select of two loads into a load through a selected pointer, which would
// demote the whole register array to scratch.
__device__ __forceinline__ uint32_t word_at(const WaveMT &m, int t)
{
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) v |= m.w[i] & (0u - (uint32_t)(t == i));
    return v;
}

__device__ __forceinline__ void mt_load(WaveMT &m, const uint32_t *g, int pos, int lane)
{
#pragma unroll
    for (int t = 0; t < 10; t++) {
        const int e = 64 * t + lane;
        m.w[t] = (e < kMtN) ? g[e] : 0u;
    }
    m.pos = pos;
}

__device__ __forceinline__ void mt_store(const WaveMT &m, uint32_t *g, int lane)
{
#pragma unroll
    for (int t = 0; t < 10; t++) {
        const int e = 64 * t + lane;
        if (e < kMtN) g[e] = m.w[t];
    }
}

// mt19937_gen, wave-parallel. new[i] = X ^ (y >> 1) ^ mag(y), y = old[i]|old[i+1]
// (upper/lower bits), X = old[i+397] for i < 227 and new[i-227] after; the last
// word mixes new[0]. Every element's inputs sit at a fixed lane offset (13 for
// i+397, 29 for i-227) of an earlier register, so the twist is 10 register
// steps in four dependency levels (registers {0-2}, {3-5}, {6-8}, {9}); the
// cross-lane reads of a level are issued together.
__device__ __forceinline__ uint32_t mt_mix(uint32_t cur, uint32_t nxt, uint32_t x)
{
    const uint32_t y = (cur & 0x80000000u) | (nxt & 0x7fffffffu);
    return x ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

__device__ void mt_twist(WaveMT &m, int lane)
{
    const int l1 = (lane + 1) & 63, l13 = (lane + 13) & 63, l29 = (lane + 29) & 63;
    const bool wrap13 = lane + 13 >= 64, wrap29 = lane + 29 >= 64;
    uint32_t o1[10], xo[4], nw[10];
    // level 0: everything that reads old words only
#pragma unroll
    for (int t = 0; t < 10; t++) {
        const uint32_t same = __shfl(m.w[t], l1);
        const uint32_t nxt = __builtin_amdgcn_readlane(m.w[t < 9 ? t + 1 : 9], 0);
        o1[t] = (lane == 63) ? nxt : same;
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const uint32_t a = __shfl(m.w[t + 6], l13);
        const uint32_t b = __shfl(m.w[t + 7 <= 9 ? t + 7 : 9], l13);
        xo[t] = wrap13 ? b : a;
    }
#pragma unroll
    for (int t = 0; t < 3; t++) nw[t] = mt_mix(m.w[t], o1[t], xo[t]);
    // levels 1..3: X = new[i-227] = register t-4 (or t-3 past the lane wrap)
#pragma unroll
    for (int lv = 1; lv <= 3; lv++) {
        const int t0 = 3 * lv, t1 = (lv == 3) ? 10 : 3 * lv + 3;
        uint32_t xn[3];
#pragma unroll
        for (int t = t0; t < t1; t++) {
            const uint32_t a = __shfl(nw[t >= 4 ? t - 4 : 0], l29);
            const uint32_t b = __shfl(nw[t - 3], l29);
            xn[t - t0] = wrap29 ? b : a;
        }
        uint32_t n0 = 0, n396 = 0;
        if (lv == 3) {
            n0 = __builtin_amdgcn_readlane(nw[0], 0);
            n396 = __builtin_amdgcn_readlane(nw[6], 12);
        }
#pragma unroll
        for (int t = t0; t < t1; t++) {
            const int e = 64 * t + lane;
            uint32_t x = xn[t - t0], nx = o1[t];
            if (t == 3) x = (e < 227) ? xo[3] : x;
            if (t == 9 && e == kMtN - 1) { nx = n0; x = n396; }
            const uint32_t v = mt_mix(m.w[t], nx, x);
            nw[t] = (e < kMtN) ? v : 0u;
        }
    }
#pragma unroll
    for (int t = 0; t < 10; t++) m.w[t] = nw[t];
    m.pos -= kMtN;   // a pending twist: position 624 + j is word j of the new key
}

// One masked bounded draw: first raw r (in stream order) with (r & mask) <= rng.
// randint's masked rejection (grid_util.py:130); the caller handles rng == 0.
__device__ uint32_t mt_draw(WaveMT &m, uint32_t mask, uint32_t rng, int lane)
{
    for (;;) {
        if (m.pos >= kMtN) mt_twist(m, lane);
        const int t = m.pos >> 6, l0 = m.pos & 63;
        const uint32_t v = temper(word_at(m, t)) & mask;
        const int e = (t << 6) + lane;
        const unsigned long long b = __ballot(lane >= l0 && e < kMtN && v <= rng);
        if (b) {
            const int f = __ffsll((long long)b) - 1;
            m.pos = (t << 6) + f + 1;
            return (uint32_t)bcast((int)v, f);
        }
        m.pos = min((t + 1) << 6, kMtN);
    }
}

__device__ __forceinline__ void mt_load_sc1(WaveMT &m, const uint32_t *g, int pos, int lane)
{
#pragma unroll
    for (int t = 0; t < 10; t++) {
        const int e = 64 * t + lane;
        m.w[t] = (e < kMtN) ? ld_sc1(g + e) : 0u;
    }
    m.pos = pos;
}

}  // namespace snake
