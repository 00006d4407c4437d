// pyrandom_kernels.hip -- Python's `random` module on the device: the one stream
// the reference trainer draws from (train_dqn.py:163-165 epsilon-greedy, :96-97
// random.sample); semantics in include/snake_env.h (snake_pyrandom_act,
// snake_pyrandom_sample), the draws' definitions in py_random.h.
//
// A stream is the 624 key words and the position of random.getstate()[1]; the
// caller owns n of them, key (n, 624) uint32 and pos (n,) int32.
//
// Act, one launch, 64 envs per wave. First a lane per snake: the greedy action
// (first maximal Q-value) of every snake, 0 for a skipped one -- coalesced, and
// no load of it waits for the stream. Then a lane per env walks its live snakes
// in slot order over the key words it consumes, read 16 at a time from its
// stream's key, and overwrites the actions that fall below epsilon; only the
// position is written back. A lane whose position reaches 624 with a word still
// to draw waits; the wave then twists those keys one after the other, all
// lanes on one key (step_mt.h), stores them, hands each lane the first words of
// its new key and the lanes go on at position 0. A key is moved once per 624
// words, not per step.
//
// Sample, one launch of one wave: the key sits in the wave's registers. Every
// pass tempers the 64 words of the key row the position stands in; a word the
// stream has passed, or that getrandbits(k) >= n rejects, drops out by a ballot.
//   pool branch (n <= setsize): one draw per pass, the first admissible word
//     of the row; the pool is uint16 in LDS (n <= 16 405) and one lane swaps.
//   set branch: every admissible word of the row is a draw of the set loop --
//     it is either new (the next output) or already selected (rejected), so the
//     whole row is settled at once: membership in an LDS hash of the selected
//     indices (open addressing, at most half full), repeats inside the row by
//     comparing with the earlier lanes -- only in a row where two candidates
//     meet in a 4 096-slot table of lane ids, which a repeat must -- and output
//     slots by a prefix count. The word that gives output B - 1 is the last
//     one consumed.
// Work and memory are O(B), whatever the capacity.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "snake_internal.h"
#include "snake_device.h"
#include "step_mt.h"
#include "py_random.h"

namespace snake {
namespace pyrandom {

struct ActArgs {
    const float *q;
    const uint8_t *skip;            // may be NULL
    uint32_t *key;
    int32_t *pos;
    int8_t *actions;
    int32_t *err;
    double epsilon;
    uint32_t N;
    int S, A;
};

struct SampleArgs {
    uint32_t *key;                  // the stream's 624 words
    int32_t *pos;
    const long long *count;
    long long *idx;
    int32_t *err;
    long long capacity;
    int B, setsize, hash_bits;
};

// a position outside [0, 624] cannot come from getstate(): flagged, and read as
// 624 so that no word outside the key is touched
__device__ __forceinline__ int checked_pos(int pos, int32_t *err)
{
    if ((uint32_t)pos > (uint32_t)kMtN) {
        *err = 1;
        pos = kMtN;
    }
    return pos;
}

__global__ void __launch_bounds__(256) k_pyrandom_act(const ActArgs g)
{
    __shared__ uint8_t skipped_all[4][kWave * kMaxSnakes];
    const int lane = threadIdx.x & 63;
    const uint32_t env0 = (blockIdx.x * 4u + (threadIdx.x >> 6)) * (uint32_t)kWave;
    if (env0 >= g.N) return;        // (the whole wave)
    uint8_t *skipped = skipped_all[threadIdx.x >> 6];
    const uint32_t env = env0 + lane;
    bool active = env < g.N;
    const int S = g.S, A = g.A;
    int pos = active ? checked_pos(g.pos[env], g.err) : 0;
    // What does not depend on the stream, a lane per snake: the greedy action of
    // every live snake and 0 for the others, the skip flags to the envs' lanes.
    const size_t rows = (size_t)g.N * S, wave_row0 = (size_t)env0 * S;
    for (int p = 0; p < S; p++) {
        const size_t row = wave_row0 + (size_t)(p * kWave + lane);
        if (row >= rows) break;
        const bool skip = g.skip != nullptr && g.skip[row] != 0;
        const float *q = g.q + row * A;
        int best = 0;
        float qb = q[0];
#pragma unroll 4
        for (int j = 1; j < A; j++) {
            const float v = q[j];
            best = v > qb ? j : best;
            qb = v > qb ? v : qb;
        }
        g.actions[row] = skip ? (int8_t)0 : (int8_t)best;
        skipped[p * kWave + lane] = skip;
    }
    wave_sync();
    uint32_t todo = 0;              // the snakes that still draw, in slot order
    if (active)
        for (int s = 0; s < S; s++) todo |= (uint32_t)(skipped[lane * S + s] == 0) << s;
    active = todo != 0;
    // The walk: the lane's next key words wait in win[0 .. navail), read kWin at
    // a time. stage 0: before a snake; 1: random()'s second word; 2: inside
    // _randbelow(A) of snake s.
    const uint32_t *key = g.key + (size_t)env * kMtN;
    const size_t row0 = (size_t)env * S;
    const int shift = randbelow_shift((uint32_t)A);
    uint32_t win[kWin], a = 0;
    int navail = 0, s = 0, stage = 0, tries = 0;
    bool twisted = false;
    for (;;) {
        while (active) {
            if (navail == 0) {
                if (pos >= kMtN) break;     // the next word is behind a twist
                if (twisted) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");   // the key this wave stored
                navail = min(kWin, kMtN - pos);
#pragma unroll
                for (int k = 0; k < kWin; k++) win[k] = key[min(pos + k, kMtN - 1)];
            }
            const uint32_t w = temper(win[0]);
#pragma unroll
            for (int k = 0; k + 1 < kWin; k++) win[k] = win[k + 1];
            navail--;
            pos++;
            if (stage == 0) {
                a = w;
                stage = 1;
            } else if (stage == 1) {
                s = __ffs((int)todo) - 1;
                if (random_double(a, w) < g.epsilon) {
                    stage = 2;
                    tries = 0;
                } else {
                    stage = 0;      // (the greedy action is stored)
                }
            } else {
                uint32_t r = w >> shift;
                if (r < (uint32_t)A || ++tries >= kMaxTries) {
                    if (r >= (uint32_t)A) {
                        *g.err = 1;
                        r = 0;
                    }
                    g.actions[row0 + s] = (int8_t)r;
                    stage = 0;
                }
            }
            if (stage == 0) {
                todo &= todo - 1;
                active = todo != 0;
            }
        }
        unsigned long long need = __ballot(active);
        if (!need) break;
        while (need) {              // all lanes on one key; its first words go to its lane
            const int f = __ffsll((long long)need) - 1;
            need &= need - 1;
            uint32_t *k = g.key + (size_t)(env0 + f) * kMtN;
            WaveMT m;
            mt_load(m, k, kMtN, lane);
            mt_twist(m, lane);
            mt_store(m, k, lane);
#pragma unroll
            for (int i = 0; i < kWin; i++) {
                const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)m.w[0], i);
                win[i] = lane == f ? v : win[i];
            }
        }
        if (active) {
            pos = 0;
            navail = kWin;
            twisted = true;
        }
    }
    if (env < g.N) g.pos[env] = pos;
}

// The tempered words of the key row the position stands in (after the twist that
// is due); *live: this lane's word is one the stream has not passed yet.
__device__ __forceinline__ uint32_t row_words(WaveMT &m, int lane, bool *twisted, bool *live)
{
    if (m.pos >= kMtN) {
        mt_twist(m, lane);
        *twisted = true;
    }
    const int t = m.pos >> 6;
    *live = lane >= (m.pos & 63) && (t << 6) + lane < kMtN;
    return temper(word_at(m, t));
}
__device__ __forceinline__ int row_base(const WaveMT &m) { return m.pos & ~63; }
__device__ __forceinline__ int next_row(const WaveMT &m) { return min(row_base(m) + 64, kMtN); }

__global__ void __launch_bounds__(64) k_pyrandom_sample(const SampleArgs g)
{
    // the selected indices' hash (u32 [1 << hash_bits]) or the pool (u16 [n])
    __shared__ uint32_t lds[kHashMax + 16];
    static_assert(sizeof(lds) >= 2 * (21 + 16384), "the pool of B = 4096");
    __shared__ uint8_t rowtab[1 << kRowBits];   // set branch: the last candidate lane per slot (never cleared)
    const int lane = threadIdx.x;
    const int B = g.B;
    // the three reads side by side (the key is only read, whatever n turns out to be)
    long long c = *g.count;
    const int pos0 = *g.pos;
    WaveMT m;
    mt_load(m, g.key, 0, lane);
    c = c < 0 ? 0 : (c > g.capacity ? g.capacity : c);
    const uint32_t n = (uint32_t)c;         // capacity < 2^31
    if (n < (uint32_t)B) {                  // where random.sample raises: nothing is drawn
        if (lane == 0) *g.err = 1;
        const uint32_t d = n ? n : 1u;
        for (int i = lane; i < B; i += kWave) g.idx[i] = (long long)((uint32_t)i % d);
        return;
    }
    m.pos = checked_pos(pos0, g.err);
    bool twisted = false, live, failed = false;
    int done = 0;                           // outputs written
    if (n <= (uint32_t)g.setsize) {
        uint16_t *pool = reinterpret_cast<uint16_t *>(lds);
        for (uint32_t i = lane; i < n; i += kWave) pool[i] = (uint16_t)i;
        wave_sync();
        for (; done < B && !failed; done++) {
            const uint32_t left = n - (uint32_t)done;
            const int shift = randbelow_shift(left);
            int tries = 0, j = -1;
            while (j < 0) {
                const uint32_t r = row_words(m, lane, &twisted, &live) >> shift;
                const unsigned long long ok = __ballot(live && r < left);
                if (ok) {
                    const int f = __ffsll((long long)ok) - 1;
                    j = bcast((int)r, f);
                    m.pos = row_base(m) + f + 1;
                } else {
                    tries += __popcll(__ballot(live));
                    m.pos = next_row(m);
                    if (tries >= kMaxTries) break;
                }
            }
            if (j < 0) {
                failed = true;
                break;
            }
            if (lane == 0) {
                g.idx[done] = pool[j];
                pool[j] = pool[left - 1];
            }
            wave_sync();
        }
    } else {
        const uint32_t hmask = (1u << g.hash_bits) - 1u;
        for (uint32_t i = lane; i <= hmask; i += kWave) lds[i] = kEmpty;
        wave_sync();
        const int shift = randbelow_shift(n);
        int run = 0;                        // words since the last new index
        while (done < B) {
            const uint32_t r = row_words(m, lane, &twisted, &live) >> shift;
            const bool valid = live && r < n;
            bool old = false;
            if (valid) {
                for (uint32_t h = hash_slot(r, g.hash_bits);; h = (h + 1) & hmask) {
                    const uint32_t v = lds[h];
                    if (v == r) old = true;
                    if (v == r || v == kEmpty) break;
                }
            }
            // A repeat inside the row shares its slot of the row table with its
            // twin: where every candidate reads its own lane id back, all differ.
            const bool cand = valid && !old;
            const uint32_t rs = hash_slot(r, kRowBits);
            if (cand) rowtab[rs] = (uint8_t)lane;
            wave_sync();
            if (__ballot(cand && rowtab[rs] != lane)) {
                for (unsigned long long vm = __ballot(cand); vm; vm &= vm - 1) {
                    const int f = __ffsll((long long)vm) - 1;
                    const uint32_t rf = (uint32_t)bcast((int)r, f);
                    if (f < lane && rf == r) old = true;
                }
            }
            const bool fresh = valid && !old;
            const unsigned long long fm = __ballot(fresh);
            const int rank = mbcnt64(fm), nf = __popcll(fm), room = B - done;
            wave_sync();                    // the lookups are over
            if (fresh && rank < room) {
                g.idx[done + rank] = (long long)r;
                for (uint32_t h = hash_slot(r, g.hash_bits);; h = (h + 1) & hmask)
                    if (atomicCAS(&lds[h], kEmpty, r) == kEmpty) break;
            }
            wave_sync();
            if (nf >= room) {
                const unsigned long long last = __ballot(fresh && rank == room - 1);
                m.pos = row_base(m) + __ffsll((long long)last);
                done = B;
            } else {
                run = nf ? 0 : run + __popcll(__ballot(live));
                done += nf;
                m.pos = next_row(m);
                if (run >= kMaxTries) {
                    failed = true;
                    break;
                }
            }
        }
    }
    if (failed) {       // no real stream gets here: flag it, and leave indices that can be gathered
        if (lane == 0) *g.err = 1;
        for (int i = done + lane; i < B; i += kWave) g.idx[i] = (long long)((uint32_t)i % n);
    }
    if (twisted) mt_store(m, g.key, lane);
    if (lane == 0) *g.pos = m.pos;
}

int check_plan(const char *who, int64_t A, int64_t B, int64_t capacity)
{
    if (A < 1 || A > kMaxActions) {
        set_error("%s: num_actions must be in [1, %d] (got %lld)", who, kMaxActions, (long long)A);
        return SNAKE_E_CONFIG;
    }
    if (B < 1 || B > kMaxBatch) {
        set_error("%s: batch must be in [1, %d] (got %lld)", who, kMaxBatch, (long long)B);
        return SNAKE_E_CONFIG;
    }
    if (capacity < 1 || capacity >= (1ll << 31)) {
        set_error("%s: capacity must be in [1, 2^31) (got %lld)", who, (long long)capacity);
        return SNAKE_E_CONFIG;
    }
    return SNAKE_OK;
}

}  // namespace pyrandom
}  // namespace snake

using namespace snake;

extern "C" int snake_pyrandom_plan(int32_t num_actions, int64_t batch, int64_t capacity)
{
    if (int rc = pyrandom::check_plan("snake_pyrandom_plan", num_actions, batch, capacity)) return rc;
    return pyrandom::sample_setsize((int)batch);
}

extern "C" int snake_pyrandom_act(const float *q, const uint8_t *skip, double epsilon, uint32_t *key, int32_t *pos,
                                  int8_t *actions, int32_t *err, int64_t num_envs, int32_t num_snakes,
                                  int32_t num_actions, void *stream)
{
    if (int rc = pyrandom::check_plan("snake_pyrandom_act", num_actions, 1, 1)) return rc;
    if (num_snakes < 1 || num_snakes > kMaxSnakes) {
        set_error("snake_pyrandom_act: num_snakes must be in [1, %d] (got %d)", kMaxSnakes, num_snakes);
        return SNAKE_E_CONFIG;
    }
    if (num_envs < 0 || num_envs > (1ll << 26)) {
        set_error("snake_pyrandom_act: num_envs must be in [0, 2^26] (got %lld)", (long long)num_envs);
        return SNAKE_E_ARG;
    }
    if (num_envs == 0) return SNAKE_OK;
    if (!q || !key || !pos || !actions || !err) {
        set_error("snake_pyrandom_act: NULL buffer");
        return SNAKE_E_ARG;
    }
    pyrandom::ActArgs g;
    g.q = q;
    g.skip = skip;
    g.key = key;
    g.pos = pos;
    g.actions = actions;
    g.err = err;
    g.epsilon = epsilon;
    g.N = (uint32_t)num_envs;
    g.S = num_snakes;
    g.A = num_actions;
    const hipStream_t s = (hipStream_t)stream;
    DeviceGuard dg(s);
    if (dg.dev < 0) return SNAKE_E_LAUNCH;
    const unsigned blocks = (unsigned)((num_envs + 255) / 256);
    hipLaunchKernelGGL(pyrandom::k_pyrandom_act, dim3(blocks), dim3(256), 0, s, g);
    return launch_status("k_pyrandom_act");
}

extern "C" int snake_pyrandom_sample(uint32_t *key, int32_t *pos, int64_t stream_index, const int64_t *count,
                                     int64_t capacity, int64_t batch, int64_t *idx, int32_t *err, void *stream)
{
    if (int rc = pyrandom::check_plan("snake_pyrandom_sample", 1, batch, capacity)) return rc;
    if (stream_index < 0 || stream_index >= (1ll << 26)) {
        set_error("snake_pyrandom_sample: stream_index must be in [0, 2^26) (got %lld)", (long long)stream_index);
        return SNAKE_E_ARG;
    }
    if (!key || !pos || !count || !idx || !err) {
        set_error("snake_pyrandom_sample: NULL buffer");
        return SNAKE_E_ARG;
    }
    pyrandom::SampleArgs g;
    g.key = key + stream_index * kMtN;
    g.pos = pos + stream_index;
    g.count = reinterpret_cast<const long long *>(count);
    g.idx = reinterpret_cast<long long *>(idx);
    g.err = err;
    g.capacity = capacity;
    g.B = (int)batch;
    g.setsize = pyrandom::sample_setsize((int)batch);
    g.hash_bits = pyrandom::sample_hash_bits((int)batch);
    const hipStream_t s = (hipStream_t)stream;
    DeviceGuard dg(s);
    if (dg.dev < 0) return SNAKE_E_LAUNCH;
    hipLaunchKernelGGL(pyrandom::k_pyrandom_sample, dim3(1), dim3(64), 0, s, g);
    return launch_status("k_pyrandom_sample");
}
