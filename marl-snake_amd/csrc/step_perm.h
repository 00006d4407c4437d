// step_perm.h -- permutation(n)[:S] of a reset: the Fisher-Yates draws in
// ballot-refined rounds (mt_perm_draws) recording the draws, and the backward
// trace of arr[:S] (perm_trace, perm_trace_j).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <type_traits>

#include "snake_internal.h"
#include "step_args.h"
#include "step_lanes.h"
#include "step_mt.h"

namespace snake {

// permutation(n) = shuffle(arange(n)) draws j_i = random_interval(i) for
// i = n-1 .. 1 (snake_env.py:581). Only arr[0..S) is ever used, so instead of the
// draws themselves the pass records, for the backward trace (perm_trace):
//   jsmall[i] = j_i for i < S, and link[x] = min{ i >= S : j_i = x < i }.
// A round covers the unread raw words of one aligned register pair (2q, 2q+1):
// lane l holds the words at stream offsets p = l - l0 (first register) and
// 64 - l0 + l (second). A word is accepted iff (w & mask) <= i - A_p, A_p = the
// accepts before it. The accept set is found by bound refinement: with acc (sure
// accepts) and pos (possible accepts) every lane knows L = |acc before it| <= A_p
// <= U = |pos before it|, and re-deciding every lane against both bounds fixes at
// least the first undecided lane per pass (typically 1-2 passes). Words past the
// accept that takes i below the current power-of-two bracket were judged with
// the wrong mask: the round ends right after that accept.
template <typename NP>
__device__ __forceinline__ void perm_record(int ii, int w, int S, NP *link, lu16 *jsmall)
{
    if (ii < S) jsmall[ii] = (uint16_t)w;
    else if (w != ii) link_min(link + w, (uint32_t)ii);
}

// One draw round over the unread words of the register pair (tw0, tw1) at key
// offset base (see mt_perm_draws). Bound refinement from the possible set:
// c = {w <= i} is a superset of the accepts, a = {w + |c before| <= i} a
// subset; a == c settles the round (most rounds, in one pass: only a word
// within |c before p| - A_p of its threshold stays open), else the bounds
// alternate until they meet. The accept set's prefix counts b are the draw
// indices' offsets, and the draw record is written through a per-lane dummy
// slot instead of exec masking: under the step's load the worker waves are
// issue-bound, so instructions (SALU and branches included) are the cost.
// Returns true when the round ended at a bracket cut inside the pair with
// draws left: the next round reads the same register pair.
template <typename NP>
__device__ __forceinline__ bool draw_round(uint32_t tw0, uint32_t tw1, int base, WaveMT &m, int &i,
                                           uint32_t &mask, int &lo, int S, NP *link, NP *dummy,
                                           lu16 *jsmall, uint32_t ones, int lane)
{
    constexpr int kBig = 0x3fffffff;   // never accepted; w + b cannot overflow
    const int l0 = m.pos - base;
    const int p0 = lane - l0;   // stream offset of this lane's first word (second: + 64)
    const int w0 = p0 >= 0 ? (int)(tw0 & mask) : kBig;
    const int w1 = (p0 >= -64 && base + 64 + lane < kMtN) ? (int)(tw1 & mask) : kBig;
    unsigned long long c0 = __ballot(w0 <= i), c1 = __ballot(w1 <= i);
    int b0 = mbcnt64(c0), b1 = mbcnt64(c1, vpopc(c0, ones));
    unsigned long long a0 = __ballot(w0 + b0 <= i), a1 = __ballot(w1 + b1 <= i);
    // (the empty asm keeps each test on the OR of both halves: folded into two
    // 64-bit compares it costs two selects and an AND per test)
    unsigned long long und = (a0 ^ c0) | (a1 ^ c1);
    __asm__ volatile("" : "+s"(und));
    if (__builtin_expect(und != 0ull, 0)) {
        for (int pass = 0; pass < 128; pass++) {
            b0 = mbcnt64(a0);
            b1 = mbcnt64(a1, __popcll(a0));
            c0 = __ballot(w0 + b0 <= i);
            c1 = __ballot(w1 + b1 <= i);
            und = (a0 ^ c0) | (a1 ^ c1);
            __asm__ volatile("" : "+s"(und));
            if (und == 0ull) break;
            b0 = mbcnt64(c0);
            b1 = mbcnt64(c1, __popcll(c0));
            a0 = __ballot(w0 + b0 <= i);
            a1 = __ballot(w1 + b1 <= i);
            und = (a0 ^ c0) | (a1 ^ c1);
            __asm__ volatile("" : "+s"(und));
            if (und == 0ull) break;
        }
    }
    // a == c: b0, b1 = the accepts before each word
    const int A0 = __popcll(a0);
    int A = A0 + __popcll(a1);
    int end = min(128, kMtN - base);
    const int k = i - lo + 1;  // accepts left in this bracket
    bool cut = false;
    if (__builtin_expect(A >= k, 0)) {
        cut = true;
        if (A0 >= k) {
            const int b = __ffsll((long long)__ballot(inv_ballot(a0) && b0 == k - 1)) - 1;
            a0 &= (2ull << b) - 1ull;
            a1 = 0;
            end = b + 1;
        } else {
            const int b = __ffsll((long long)__ballot(inv_ballot(a1) && b1 == k - 1)) - 1;
            a1 &= (2ull << b) - 1ull;
            end = 64 + b + 1;
        }
        A = k;
    }
    const int ii0 = i - b0, ii1 = i - b1;
    if constexpr (std::is_same<NP, lu16>::value) {
        // LDS draw record: j_i at index i (one writer per index), the rest to
        // the lane's dummy slot
        *(inv_ballot(a0) ? link + ii0 : dummy) = (uint16_t)w0;
        *(inv_ballot(a1) ? link + ii1 : dummy) = (uint16_t)w1;
    } else if (__builtin_expect(i - A + 1 < S, 0)) {   // the last rounds: some indices < S
        if (inv_ballot(a0)) perm_record(ii0, w0, S, link, jsmall);
        if (inv_ballot(a1)) perm_record(ii1, w1, S, link, jsmall);
    } else {
        // every index of the round >= S: unconditional min, misses to the dummy
        link_min((inv_ballot(a0) && w0 != ii0) ? link + w0 : dummy, (uint32_t)ii0);
        link_min((inv_ballot(a1) && w1 != ii1) ? link + w1 : dummy, (uint32_t)ii1);
    }
    m.pos = base + end;
    i -= A;
    // the bracket of the new i, branch-free (i < 1 ends the draws anyway)
    mask = i > 0 ? (0xffffffffu >> __builtin_clz((uint32_t)i)) : 0u;
    lo = (int)(mask >> 1) + 1;
    return cut && i >= 1 && end < 128 && m.pos < kMtN;
}

template <typename NP>
__device__ void mt_perm_draws(WaveMT &m, int n, int S, NP *link, int link_n, lu16 *jsmall, int lane)
{
    int i = n - 1;
    if (i < 1) return;
    uint32_t mask = gen_mask((uint32_t)i);
    int lo = (int)(mask >> 1) + 1;
    // the tempered key stays in registers: the rounds never read LDS, so nothing
    // waits for the link-table atomics until the draws are done. The rounds of a
    // key block run pair by pair, unrolled: each pair's words are fixed registers.
    uint32_t tk[10];
#pragma unroll
    for (int t = 0; t < 10; t++) tk[t] = temper(m.w[t]);
    NP *dummy = link + link_n + lane;   // lanes with nothing to record hit their own dummy
    uint32_t ones;
    __asm__ volatile("v_mov_b32 %0, -1" : "=v"(ones));
    // every round advances the stream; the cap only guarantees that a broken
    // invariant ends the wave instead of hanging the GPU
    for (int guard = 0; i >= 1 && guard < (1 << 20); guard++) {
        if (m.pos >= kMtN) {
            mt_twist(m, lane);
#pragma unroll
            for (int t = 0; t < 10; t++) tk[t] = temper(m.w[t]);
        }
#pragma unroll
        for (int q = 0; q < 5; q++) {
            // a round normally consumes the rest of the pair; only a bracket cut
            // inside it repeats the pair
            if (i >= 1 && m.pos < kMtN && (m.pos >> 7) == q) {
                bool again;
                do {
                    again = draw_round(tk[2 * q], tk[2 * q + 1], q << 7, m, i, mask, lo, S, link, dummy, jsmall,
                                       ones, lane);
                } while (__builtin_expect(again, 0));
            }
        }
    }
}

// Final arr[k] of the Fisher-Yates pass for k < S from the LDS draw record
// (jarr[i] = j_i): replay the swaps i < S on lane k's position k, then scan
// i = S .. n-1 in order, 256 at a time: a tracked position x moves to i exactly
// when j_i == x (the swap brings arr[i] there; x < i always). Every tracked
// position is tested against a chunk with one ballot; a hit re-tests the rest
// of the chunk from the new position.
template <int MS>
__device__ void perm_trace_j(int S, int n, const lu16 *jarr, int (&q)[MS], int lane)
{
    int x = lane;
    for (int i = 1; i < S; i++) {
        const int j = jarr[i];
        x = (x == i) ? j : (x == j ? i : x);
    }
    // tracked positions, and as packed 16-bit pairs for the match test
    // (positions and record entries are < 65 535; untracked slots and the
    // padding past n are 0xffff: a padding match only sends the last chunk down
    // the exact per-position path)
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    int xk[MS];
    u16x2 xp[MS / 2];
#pragma unroll
    for (int k = 0; k < MS; k++) xk[k] = bcast(x, k);
    auto pack = [&]() {
#pragma unroll
        for (int p2 = 0; p2 < MS / 2; p2++) {
            xp[p2].x = (unsigned short)(2 * p2 < S ? xk[2 * p2] : 0xffff);
            xp[p2].y = (unsigned short)(2 * p2 + 1 < S ? xk[2 * p2 + 1] : 0xffff);
        }
    };
    pack();
    for (int base = S; base < n; base += 4 * kWave) {
        int jv[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = base + u * kWave + lane;
            jv[u] = (int)jarr[min(i, n - 1)];
            jv[u] = i < n ? jv[u] : 0xffff;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            // one ballot against every tracked position (a move is rare: ~ln n
            // per position over the whole scan); the per-position chase only
            // when some lane matched
            // (packed 16-bit differences to two tracked positions per vector
            // instruction, their minimum; zero = a match: one vector-to-scalar
            // hand-off per block)
            u16x2 jj;
            jj.x = (unsigned short)jv[u];
            jj.y = (unsigned short)jv[u];
            u16x2 dm = jj - xp[0];
#pragma unroll
            for (int p2 = 1; p2 < MS / 2; p2++) dm = __builtin_elementwise_min(dm, jj - xp[p2]);
            const bool hit = min(dm.x, dm.y) == 0;
            if (__builtin_expect(__ballot(hit) != 0ull, 0)) {
#pragma unroll
                for (int k = 0; k < MS; k++) {
                    if (k < S) {
                        unsigned long long m = __ballot(jv[u] == xk[k]);
                        while (m) {
                            const int l = __ffsll((long long)m) - 1;
                            xk[k] = base + u * kWave + l;
                            m = __ballot(jv[u] == xk[k]);
                        }
                    }
                }
                pack();
            }
        }
    }
#pragma unroll
    for (int k = 0; k < MS; k++) q[k] = xk[k];
}

// Final arr[k] of the Fisher-Yates pass for k < S, lane k: walk position k
// backwards through the swaps (i ascending). The swaps i < S only move positions
// < S (j_i <= i): replay them from jsmall. After that the tracked position q < S
// <= i is only moved by a swap with j_i = q, to position i; from position x the
// next move is the first later swap with j = x: link[x]. Chains are ~ln(n) long.
template <int MS, typename NP>
__device__ void perm_trace(int S, const NP *link, const lu16 *jsmall, int (&q)[MS], int lane)
{
    int x = lane;
    for (int i = 1; i < S; i++) {
        const int j = jsmall[i];
        x = (x == i) ? j : (x == j ? i : x);
    }
    if (lane < S) {
        for (;;) {
            const uint32_t y = link_get(link + x);
            if (y == kNoLink) break;
            x = (int)y;
        }
    }
#pragma unroll
    for (int k = 0; k < MS; k++) q[k] = bcast(x, k);
}

}  // namespace snake
