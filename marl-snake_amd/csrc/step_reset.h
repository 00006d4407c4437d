// step_reset.h -- resets and spawn-ahead: the fruit draws, one spawn attempt
// (permutation, poses, overlap test), the spawn-ahead records and their status
// word, do_reset, the spawn jobs, and the reset worker's job loop
// (autoreset_worker).
#pragma once
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdint.h>

#include "snake_internal.h"
#include "snake_diag.h"
#include "step_args.h"
#include "step_lanes.h"
#include "step_mt.h"
#include "step_perm.h"
#include "step_encode.h"

namespace snake {

// ------------------------------------------------------------ fruit respawn
// random_empty_coords + grid[xs, ys] = FRUIT (grid_util.py:126-133,
// snake_env.py:376-379): np.where order is row-major, draws are with
// replacement, all draws index the pre-respawn empty list.
__device__ void place_fruits(const KCfg &c, uint8_t *g, WaveMT &m, int k, uint16_t *fbuf, int lane)
{
    const int c0 = lane * c.cs, c1 = min(c.HW, c0 + c.cs);
    int cnt = 0;
    for (int x = c0; x < c1; x++) cnt += (g[x] == C_EMPTY);
    const int incl = wave_scan(cnt, lane), excl = incl - cnt;
    const int E = bcast(incl, 63);
    if (E == 0) return;  // no empty cell: no draw (random_empty_coords returns None)
    const uint32_t rng = (uint32_t)(E - 1), mask = gen_mask(rng);
    for (int d = 0; d < k; d++) {
        const uint32_t v = rng == 0 ? 0u : mt_draw(m, mask, rng, lane);
        if ((int)v >= excl && (int)v < incl) {
            int need = (int)v - excl;
            for (int x = c0; x < c1; x++) {
                if (g[x] == C_EMPTY) {
                    if (need == 0) { fbuf[d] = (uint16_t)x; break; }
                    need--;
                }
            }
        }
    }
    wave_sync();
    for (int d = lane; d < k; d += kWave) g[fbuf[d]] = C_FRUIT;
    wave_sync();
}


// The reset's fruits (SnakeEnv.reset :147-148 -> random_empty_coords,
// grid_util.py:126-133) on the freshly painted board: its empty cells are the
// interior minus the S*L disjoint snake cells, so no grid scan is needed.
// Draws: randint(0, E, size=k), one mt_draw each (all index the same empty
// list: placing a fruit does not change E).
// Cells: the v-th empty cell in np.where's row-major order has interior index
// y = the least fixed point of y = v + #{snake cells with interior index <= y}
// (iterated from v: a snake cell is never a least fixed point). `cell` = lane's
// snake cell (lanes < S*L).
__device__ void place_fruits_fresh(const KCfg &c, uint8_t *g, WaveMT &m, int k, int cell, int lane)
{
    const int Wi = c.W - 2, SL = c.S * c.L;
    const uint32_t E = (uint32_t)((c.H - 2) * Wi - SL), rng = E - 1, mask = gen_mask(rng);
    const int hr = (int)__umulhi((uint32_t)cell, c.mag_W);
    const int yi = lane < SL ? (hr - 1) * Wi + (cell - hr * c.W - 1) : INT_MAX;
    for (int d = 0; d < k; d++) {
        // randint(0, E) (rng == 0: no raw consumed), the same mt_draw as the step's respawn
        const int v = rng == 0 ? 0 : (int)mt_draw(m, mask, rng, lane);
        int y = v;
        for (int it = 0; it <= SL; it++) {
            const int y1 = v + __popcll(__ballot(yi <= y));
            if (y1 == y) break;
            y = y1;
        }
        const int r = y / Wi;
        if (lane == 0) g[(r + 1) * c.W + (y - r * Wi) + 1] = C_FRUIT;
    }
    wave_sync();
}

__device__ __forceinline__ int dir_of_diff(int diff, int W)
{
    return diff == -W ? 0 : (diff == 1 ? 1 : (diff == W ? 2 : 3));
}

// ------------------------------------------------------------------- reset
// One iteration of _generate_snakes' retry loop (:576-589): S spawn poses =
// permutation(n_cand)[:S] drawn from the wave's MT, lane (sk, si) = cell si of
// pose sk (-1 past S*L), q = the pose indices; true when the poses are disjoint
// (_clear_overlap :568-574).
template <int MS, int JL>
__device__ bool spawn_attempt(const KCfg &c, const snake_state &st, WaveMT &mt, uint8_t *lds, int slot,
                              int (&q)[MS], int &cell, int lane)
{
    const int S = c.S, L = c.L, SL = S * L;
    const int sk = lane / L, si = lane - sk * L;
    if constexpr (JL == 2) {
        {
            // small batches: the u32 link table in LDS (ds_min, no scan: the
            // trace is a short pointer chase)
            lu32 *link = (lu32 *)(lds + c.lds_link);
            lu16 *jsmall = (lu16 *)(lds + c.lds_fruit);   // the fruit buffer is free until place_fruits
            for (int x = 4 * lane; x < c.link_stride - kWave; x += 4 * kWave) *(lu4 *)(link + x) = (v4u32)kNoLink;
            wave_sync();
            mt_perm_draws(mt, c.n_cand, S, link, c.n_cand, jsmall, lane);
            wave_sync();
            perm_trace<MS>(S, link, jsmall, q, lane);
        }
    } else if constexpr (JL == 1) {
        {
            // the u16 draw record in LDS: every index 1..n-1 is written, nothing to clear
            lu16 *jarr = (lu16 *)(lds + c.lds_link);
            mt_perm_draws(mt, c.n_cand, S, jarr, c.n_cand, jarr, lane);
            wave_sync();
            perm_trace_j<MS>(S, c.n_cand, jarr, q, lane);
        }
    } else {
        // large boards: the link table in this worker's global scratch
        gu32 *link = (gu32 *)(st.jscratch + (int64_t)slot * c.link_stride);
        lu16 *jsmall = (lu16 *)(lds + c.lds_fruit);   // the fruit buffer is free until place_fruits
        for (int x = 4 * lane; x < c.link_stride - kWave; x += 4 * kWave)
            *(gu4 *)(link + x) = (v4u32)kNoLink;
        // (the table is this wave's alone: its own stores and atomics drained
        // and made visible, no workgroup barrier -- k_post_lean runs four
        // independent workers per workgroup)
        link_sync();
        mt_perm_draws(mt, c.n_cand, S, link, c.n_cand, jsmall, lane);
        link_sync();   // the link table, written by every lane
        perm_trace<MS>(S, link, jsmall, q, lane);
    }
    int pk = 0;
#pragma unroll
    for (int k = 0; k < MS; k++) pk = (sk == k) ? q[k] : pk;
    cell = (lane < SL) ? (int)st.cand[(int64_t)pk * L + si] : -1;
    bool dup = false;
    for (int x = 0; x < SL; x++) {
        const int cx = bcast(cell, x);
        dup |= (lane < SL && lane != x && cx == cell);
    }
    return __ballot(dup) == 0ull;
}

// Spawn-ahead status word (env word ENV_SPAWN): bits 0-1 the status, bit 2 the
// record buffer holding the record (background spawn-ahead keeps two per env,
// k_spawn), bits 3-31 the generation (bumped by every draw that voids it).
constexpr uint32_t kGenOne = 1u << kSpawnGenShift;
__device__ __forceinline__ uint32_t *spawn_rec(const KCfg &c, const snake_state &st, int64_t e, int b)
{
    return st.spawn + ((int64_t)b * c.N + e) * kSpawnStride;
}

// The MT19937 state a reset (or an in-step spawn-ahead attempt) of env e
// starts from: the spawn-ahead record when one exists (the key and position
// after its recorded attempts), else the env's own; cellw = this lane's word
// of the record's spawn cells (lanes 2m, 2m + 1: word m). Returns the status
// word (wave-uniform; the status is its bits 0-1). The state it expects (the
// record for a reset, the env's own for an attempt, which mostly starts afresh)
// is loaded with the status word, in the same round trip; the other one only
// when the status asks for it. (Records are in buffer 0 without background
// spawn-ahead.)
__device__ __forceinline__ int load_reset_mt(const KCfg &c, const snake_state &st, int64_t e, WaveMT &mt, int lane,
                                             bool expect_record, uint32_t &cellw)
{
    const uint32_t *rec = spawn_rec(c, st, e, 0);
    const uint32_t *key = st.mt + e * kMtN;
    const int spw = st.env[e * kEnvRec + ENV_SPAWN];
    if (expect_record) {
        mt_load(mt, rec, (int)rec[kSpawnPos], lane);
        cellw = rec[kSpawnCells + (lane >> 1)];
        if ((spw & 3) == SPAWN_NONE) mt_load(mt, key, st.env[e * kEnvRec + ENV_MTPOS], lane);
    } else {
        mt_load(mt, key, st.env[e * kEnvRec + ENV_MTPOS], lane);
        cellw = 0;
        if ((spw & 3) != SPAWN_NONE) mt_load(mt, rec, (int)rec[kSpawnPos], lane);
    }
    return spw;
}

// load_reset_mt for an explicit reset (k_reset) under background spawn-ahead
// (KCfg.bg): a k_spawn job publishes a record into its queue set's buffer and
// names that buffer in the status word, so the record is read from there, not
// from buffer 0. The launch is ordered after every background job
// (wait_background), so plain loads see what the jobs published and no job is
// drawing; a word still marked DRAWING counts as no record, as for a claim.
__device__ __forceinline__ int load_reset_mt_bg(const KCfg &c, const snake_state &st, int64_t e, WaveMT &mt, int lane,
                                                uint32_t &cellw)
{
    int spw = st.env[e * kEnvRec + ENV_SPAWN];
    if ((spw & 3) == SPAWN_DRAWING) spw &= ~3;
    cellw = 0;
    if ((spw & 3) != SPAWN_NONE) {
        const uint32_t *rec = spawn_rec(c, st, e, (spw >> kSpawnBufShift) & (kQSets - 1));
        mt_load(mt, rec, (int)rec[kSpawnPos], lane);
        cellw = rec[kSpawnCells + (lane >> 1)];
    } else {
        mt_load(mt, st.mt + e * kMtN, st.env[e * kEnvRec + ENV_MTPOS], lane);
    }
    return spw;
}

// Background spawn-ahead (KCfg.bg): an auto-reset takes env e's record with one
// atomic that bumps the generation (a k_spawn job still working on the env then
// fails its publish), and reads the record it found with sc1 loads.
// A reset that finds a background job drawing the env's record right now
// (status SPAWN_DRAWING, set by do_spawn_bg) waits for the job to publish
// instead of voiding it and drawing the same permutations again inline: the
// job was queued at least a step earlier and is usually close to done, while an
// inline 40x40 attempt took ~70-80 us of k_post_lean's span in a quarter of
// cfg5's steps (round 5 kernel trace). The wait is bounded (KCfg.draw_wait ticks
// of the 100 MHz clock, by default 2 ms, far beyond a job's ~100 us;
// snake_debug_set("draw_wait_ticks") changes it, e.g. 0 for the test of the
// fallback); after it the claim voids the job as before and the reset draws from
// the env's own state -- right for a job that started from a partial record too:
// the env's state is where that record's failed permutations began, so the reset
// replays them. The voided job may still be drawing; it writes only its own
// queue set's record buffer, which nothing reads until a later job of that set
// (same stream, after it) publishes there, and its final compare-and-swap fails
// against the claim's generation.
__device__ __forceinline__ int claim_reset_mt(const KCfg &c, const snake_state &st, int64_t e, WaveMT &mt,
                                              int lane, uint32_t &cellw)
{
    int v = 0;
    if (lane == 0) {
        uint32_t *wp = reinterpret_cast<uint32_t *>(st.env + e * kEnvRec + ENV_SPAWN);
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        const unsigned long long wait = (unsigned)c.draw_wait;
        if (c.diag && (ld_sc1(wp) & 3u) == SPAWN_DRAWING) DIAG_ADD(g_draw_wait);
        while ((ld_sc1(wp) & 3u) == SPAWN_DRAWING && __builtin_amdgcn_s_memrealtime() - t0 < wait)
            __builtin_amdgcn_s_sleep(8);
        v = (int)atomicAdd(wp, kGenOne);
        if (c.diag && (v & 3) == SPAWN_DRAWING) DIAG_ADD(g_draw_timeout);
    }
    int spw = __shfl(v, 0);
    if ((spw & 3) == SPAWN_DRAWING) spw &= ~3;   // (still drawing: from the env's own state, as for NONE)
    cellw = 0;
    if ((spw & 3) != SPAWN_NONE) {
        const uint32_t *rec = spawn_rec(c, st, e, (spw >> kSpawnBufShift) & (kQSets - 1));
        mt_load_sc1(mt, rec, (int)ld_sc1(rec + kSpawnPos), lane);
        cellw = ld_sc1(rec + kSpawnCells + (lane >> 1));
    } else {
        mt_load(mt, st.mt + e * kMtN, st.env[e * kEnvRec + ENV_MTPOS], lane);
    }
    return spw;
}

// ------------------------------------------------------------------- reset
// SnakeEnv.reset (snake_env.py:131-159): walled grid, S spawn poses =
// permutation(n_cand)[:S] retried until disjoint (:576-589), Snake(idx, coords)
// (core/snake.py:53-74), num_fruits fruit draws, first observation replicated
// over the frame stack. `mt` comes from load_reset_mt: with a ready spawn-ahead
// record the poses are the record's and the draws are already done; a partial
// record continues the retries where the record left them.
// The rest of the reset once the spawn cells are known (lane's cell, lanes <
// S*L): the grid, the snakes, the fruits, the records and the first observation.
__device__ __forceinline__ void reset_paint(const KCfg &c, const snake_state &st, const snake_out &o, int e, WaveMT &mt, uint8_t *lds,
                            int spw, int cell, bool failed, int lane)
{
    const int spst = spw & 3;
    uint8_t *frames = lds + c.lds_frames;
    int *org = reinterpret_cast<int *>(lds + c.lds_centers);
    uint16_t *fbuf = reinterpret_cast<uint16_t *>(lds + c.lds_fruit);
    uint8_t *work = frames + (c.fs - 1) * c.grid_stride;
    const int S = c.S, L = c.L, W = c.W, SL = S * L;
    const int sk = lane / L, si = lane - sk * L;
    // make_grid (grid_util.py:14-20), then paint (:138-144)
    for (int x = lane; x < c.HW; x += kWave) {
        const int r = (int)__umulhi((uint32_t)x, c.mag_W), cc = x - r * W;   // x / W
        work[x] = (r == 0 || cc == 0 || r == c.H - 1 || cc == W - 1) ? C_WALL : C_EMPTY;
    }
    wave_sync();
    const int nxt = __shfl(cell, (lane + 1) & 63);
    const int tailcell = __shfl(cell, min(lane + L - 1, 63));
    // the tail queue holds the whole deque (up to 14 directions): entry j =
    // directions[-1-j] = the direction of body cell L-2-j, on lane sk*L + L-2-j
    const int mydir = dir_of_diff(cell - nxt, W);
    const int nq0 = min(L - 1, 14);
    uint32_t tq0 = 0;
    for (int j = 0; j < nq0; j++) tq0 |= (uint32_t)__shfl(mydir, min(sk * L + L - 2 - j, 63)) << (2 * j);
    if (lane < SL) {
        const int v = (si == 0 ? C_HEAD : (si == L - 1 ? C_TAIL : C_BODY)) + 10 * sk;
        work[cell] = (uint8_t)v;
        uint8_t *ring = st.body + ((int64_t)e * S + sk) * c.ring_cap;
        if (si < L - 1) ring[si] = (uint8_t)dir_of_diff(cell - nxt, W);
        if (si == 0) {
            const int hr = (int)__umulhi((uint32_t)cell, c.mag_W), hc = cell - hr * W;
            const int tr = (int)__umulhi((uint32_t)tailcell, c.mag_W), tc = tailcell - tr * W;
            int4 rec;
            rec.x = hr | (hc << 8) | (tr << 16) | (tc << 24);
            rec.y = dir_of_diff(cell - nxt, W) | (1 << 8);
            rec.z = 0 | ((L - 1) << 16);
            // cached directions[-1] (the direction move() pops next)
            rec.w = (int)(tq0 | ((uint32_t)nq0 << 28));
            reinterpret_cast<int4 *>(st.snake)[(int64_t)e * S + sk] = rec;
            const int og = pack_origin(c, hr, hc);
            for (int f = 0; f < c.fs; f++) {
                org[f * kMaxSnakes + sk] = og;
                st.ctr[((int64_t)e * c.fs + f) * S + sk] = (uint16_t)((hr << 8) | hc);
            }
        }
    }
    wave_sync();
    if (!failed) place_fruits_fresh(c, work, mt, c.num_fruits, cell, lane);   // :147-148
    else place_fruits(c, work, mt, c.num_fruits, fbuf, lane);     // (overlapping snakes: count the grid)
    uint8_t *gbase = st.grid + (int64_t)e * c.fs * c.grid_stride;
    const int n16 = c.grid_stride >> 4;
    for (int q = lane; q < n16; q += kWave) {
        const uint4 v = reinterpret_cast<const uint4 *>(work)[q];
        for (int s = 0; s < c.fs; s++) reinterpret_cast<uint4 *>(gbase + s * c.grid_stride)[q] = v;
        for (int s = 0; s < c.fs - 1; s++) reinterpret_cast<uint4 *>(frames + s * c.grid_stride)[q] = v;
    }
    if (lane == 0) {
        int4 er;
        er.x = S; er.y = 0; er.z = c.fs - 1; er.w = mt.pos;
        *reinterpret_cast<int4 *>(st.env + (int64_t)e * kEnvRec) = er;
        // record used up (background: the claim's bumped generation, buffer 0)
        if (c.bg) st.env[(int64_t)e * kEnvRec + ENV_SPAWN] = (int)((((uint32_t)spw >> kSpawnGenShift) + 1u) << kSpawnGenShift);
        else if (spst != SPAWN_NONE) st.env[(int64_t)e * kEnvRec + ENV_SPAWN] = spw & ~3;
        st.env[(int64_t)e * kEnvRec + ENV_FAIL] = failed ? 1 : 0;
        if (failed && o.err) o.err[e] = 2;
    }
    if (lane < 2 * S) reinterpret_cast<uint64_t *>(st.stats)[(int64_t)e * 2 * S + lane] = 0ull;   // _reset_epi_stats
    mt_store(mt, st.mt + (int64_t)e * kMtN, lane);
    wave_sync();
    // (the direct encode: on the reset's critical path the staged row-wise
    // encode's two extra LDS passes cost more than they save)
    encode(c, frames, org, 0, o.obs + (int64_t)e * c.units * 8, lane);
}

template <int MS, int JL>
__device__ void do_reset(const KCfg &c, const snake_state &st, const snake_out &o, int e,
                         WaveMT &mt, uint8_t *lds, int slot, int spw, uint32_t cellw, int lane)
{
    const int spst = spw & 3;
    const int SL = c.S * c.L;
    int cell = -1;
    bool failed = false;
    if (spst == SPAWN_READY) {   // the record's cells (loaded with its key)
        if (lane < SL) cell = (int)((cellw >> (16 * (lane & 1))) & 0xffffu);
    } else {
        // The reference retries forever; a board too crowded for S disjoint spawn
        // poses would hang the wave, so give up after 2^16 permutations and flag
        // the env (env word ENV_FAIL; snake_plan rejects boards where that is
        // likelier than ~1e-6 per reset)
        int q[MS];
        bool ok = false;
        for (int attempt = 0; attempt < (1 << 16) && !ok; attempt++)
            ok = spawn_attempt<MS, JL>(c, st, mt, lds, slot, q, cell, lane);
        failed = !ok;
    }
    reset_paint(c, st, o, e, mt, lds, spw, cell, failed, lane);
}

// ------------------------------------------------------- spawn-ahead records
// Spawn-ahead job of env e (include/snake_env.h snake_step): one permutation
// attempt of its next reset, from its MT state or its partial record, into the
// record. k_logic queues only envs with no ready record whose reset is not this
// step, so nothing else touches the env's MT state or record meanwhile.
// The status word spw is the one the attempt started under (generation kept);
// a background job publishes with a compare-and-swap against it (k_spawn).
// The record goes to buffer nb. Background (k_spawn, BG): write-through stores,
// drained, then published with a compare-and-swap against spw.
// The spawn cells (lane < S*L: `cell`, from spawn_attempt) are stored as u16
// pairs, lanes 2m and 2m + 1 in word m, so a reset reads them with the key.
template <bool BG = false>
__device__ void store_spawn_record(const KCfg &c, const snake_state &st, int e, const WaveMT &mt, bool ok,
                                   int cell, int lane, uint32_t spw, int nb = 0)
{
    uint32_t *rec = spawn_rec(c, st, e, nb);
    // (the odd neighbour's cell: DPP quad_perm [1,0,3,2], the whole wave active)
    const int nxt = dpp_pin(__builtin_amdgcn_mov_dpp(cell, 0xb1, 0xf, 0xf, false));
    const uint32_t cw = ((uint32_t)cell & 0xffffu) | ((uint32_t)nxt << 16);
    const bool cst = ok && (lane & 1) == 0 && lane < c.S * c.L;
    uint32_t *wp = reinterpret_cast<uint32_t *>(st.env + (int64_t)e * kEnvRec + ENV_SPAWN);
    const uint32_t w1 = (spw & ~((1u << kSpawnGenShift) - 1u)) | ((uint32_t)nb << kSpawnBufShift) |
                        (ok ? SPAWN_READY : SPAWN_PARTIAL);
    if constexpr (BG) {
#pragma unroll
        for (int t = 0; t < 10; t++)
            if (64 * t + lane < kMtN) st_sc1(rec + 64 * t + lane, mt.w[t]);
        if (cst) st_sc1(rec + kSpawnCells + (lane >> 1), cw);
        if (lane == 0) st_sc1(rec + kSpawnPos, (uint32_t)mt.pos);
        __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) atomicCAS(wp, spw, w1);
    } else {
        mt_store(mt, rec, lane);
        if (cst) rec[kSpawnCells + (lane >> 1)] = cw;
        if (lane == 0) {
            rec[kSpawnPos] = (uint32_t)mt.pos;
            *wp = w1;
        }
    }
}

// The in-step spawn-ahead job of env e: one attempt from its MT state or its
// partial record, into record buffer 0.
template <int MS, int JL>
__device__ void do_spawn(const KCfg &c, const snake_state &st, int e, uint8_t *lds, int slot, int lane)
{
    WaveMT mt;
    uint32_t cellw;
    const int spw = load_reset_mt(c, st, e, mt, lane, false, cellw);
    if ((spw & 3) == SPAWN_READY) return;
    int q[MS], cell;
    bool ok = false;
    for (int a = 0; a < c.spawn_tries && !ok; a++) {   // (attempts until disjoint, at most spawn_tries)
        if (a > 0) wave_sync();
        ok = spawn_attempt<MS, JL>(c, st, mt, lds, slot, q, cell, lane);
    }
    store_spawn_record(c, st, e, mt, ok, cell, lane, (uint32_t)spw);
}

// Background spawn-ahead job (k_spawn) of env e, queued by step t's k_logic at
// generation qgen, running beside step t's resets and step t+1 (both its rules
// and its resets). Every writer of env e's MT state changes the generation with
// an atomic first or last -- k_logic's draws (atomic exchange after them), an
// auto-reset's claim (atomic add before it) -- so a job that sees another
// generation has nothing to do, and one whose inputs were being rewritten fails
// its final compare-and-swap (or is voided by the exchange landing after it).
// The record goes to buffer c.qpar, the job's queue set. Since round 5 the two
// sets' kernels run on two streams and may overlap: a job voided by k_logic's
// fruit draw (its word overwritten) may still be running when the next step's
// k_logic queues the env again into the other set, whose job then draws from
// the new state. Writing "the buffer the word does not point at" (as until
// round 5) let both jobs write the same buffer -- k_logic's exchange clears the
// buffer bit -- and a late write of the voided job could land in the published
// record. With one buffer per set the two write different buffers; jobs of one
// set run in order on one stream. A reset reads the buffer the word points at,
// and the job that published it has finished; a job continuing a partial
// record of its own set's buffer reads it whole (into registers) before it
// overwrites it.
template <int MS>
__device__ void do_spawn_bg(const KCfg &c, const snake_state &st, int e, uint32_t qgen, uint8_t *lds, int lane)
{
    uint32_t *wp = reinterpret_cast<uint32_t *>(st.env + (int64_t)e * kEnvRec + ENV_SPAWN);
    int v = 0;
    if (lane == 0) v = (int)atomicAdd(wp, 0u);   // (the memory-side value)
    uint32_t spw = (uint32_t)__shfl(v, 0);
    // (READY: nothing to do; DRAWING: another job -- an earlier step's -- has it)
    if (((spw >> kSpawnGenShift) & ((1u << kQGenBits) - 1u)) != qgen || (spw & 3u) >= SPAWN_READY) return;
    const uint32_t st0 = spw & 3u;
    {
        // mark the record as being drawn: claim_reset_mt waits for it, and a job
        // of the other queue set's kernel (they may overlap) leaves the env
        // alone. A word that moved meanwhile (a draw voided it, a reset claimed
        // it, the other job took it) ends this job.
        int won = 0;
        if (lane == 0) won = atomicCAS(wp, spw, (spw & ~3u) | SPAWN_DRAWING) == spw ? 1 : 0;
        if (!__shfl(won, 0)) return;
        spw = (spw & ~3u) | SPAWN_DRAWING;
    }
    // (fault injection for the tests, snake_debug_set "spawn_delay_ticks": the
    // job holds the record DRAWING that much longer, so resets meet it)
    if (c.spawn_delay) {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__builtin_amdgcn_s_memrealtime() - t0 < (unsigned)c.spawn_delay) __builtin_amdgcn_s_sleep(32);
    }
    const int buf = (spw >> kSpawnBufShift) & (kQSets - 1);
    WaveMT mt;
    if (st0 != SPAWN_NONE) {
        const uint32_t *rec = spawn_rec(c, st, e, buf);
        mt_load_sc1(mt, rec, (int)ld_sc1(rec + kSpawnPos), lane);
    } else {
        mt_load(mt, st.mt + (int64_t)e * kMtN, st.env[(int64_t)e * kEnvRec + ENV_MTPOS], lane);
    }
    int q[MS], cell;
    bool ok = false;
    for (int a = 0; a < c.bg_tries && !ok; a++) {   // (attempts until disjoint, at most bg_tries)
        if (a > 0) wave_sync();
        ok = spawn_attempt<MS, 1>(c, st, mt, lds, 0, q, cell, lane);
    }
    store_spawn_record<true>(c, st, e, mt, ok, cell, lane, spw, c.qpar);
}

// Spawn-ahead right after an explicit reset (k_reset): the next episode's spawn
// poses drawn from the MT state the reset leaves (still in registers), up to
// kResetAheadTries permutation attempts (READY, else a PARTIAL record the step's
// workers continue). Nothing else has drawn from that state, so the record is
// exactly what the next reset would draw (spawn-ahead semantics, snake_step).
constexpr int kResetAheadTries = 4;

template <int MS, int JL>
__device__ void spawn_after_reset(const KCfg &c, const snake_state &st, int e, WaveMT &mt, uint8_t *lds,
                                  int slot, int lane)
{
    wave_sync();   // the reset's encode has read the LDS frames the draw record may overlay
    int q[MS], cell;
    bool ok = false;
    for (int a = 0; a < kResetAheadTries && !ok; a++)
        ok = spawn_attempt<MS, JL>(c, st, mt, lds, slot, q, cell, lane);
    store_spawn_record(c, st, e, mt, ok, cell, lane, (uint32_t)st.env[(int64_t)e * kEnvRec + ENV_SPAWN], 0);
}

// RO: resets only (every-step mode, background spawn-ahead): no spawn-job path,
// fewer registers. JL: 1 the u16 draw record in LDS (KCfg.link_in_lds), 2 the
// u32 link table in LDS (KCfg.link32, batches of up to 32 768 envs), 0 the
// global link tables; one path per instantiation.
// wid = this worker (0 .. G-1): k_autoreset's block, or a block of k_post.
template <int MS, bool RO, int JL>
__device__ __forceinline__ void autoreset_worker(KPtr kp, const int wid, const int G, uint8_t *lds)
{
    const int lane = threadIdx.x & (kWave - 1);
    const KArgs &A = kargs(kp);
    const KCfg &c = A.c;
    const snake_state &st = A.st;
    // the shard counts of the three queues, prefix-summed: queue index j lives
    // in the shard whose [excl, incl) holds it
    const int64_t qset = kNumQ * kQShards * c.q_cap + kQCounters;
    int *qb = st.resetq + c.qpar * qset;
    int *qc = qb + kNumQ * kQShards * c.q_cap;
    const int cnt = qc[lane * kQSpread], ucnt = qc[(kQShards + lane) * kQSpread],
              ncnt = qc[(2 * kQShards + lane) * kQSpread];
    const int incl = wave_scan(cnt, lane), uincl = wave_scan(ucnt, lane), nincl = wave_scan(ncnt, lane);
    const int R = bcast(incl, kWave - 1), U = bcast(uincl, kWave - 1);
    // claim shards: min(G, kClaimShards), so that every shard has a worker
    const int nsh = min(G, kClaimShards);
    const int x = G >= kClaimShards ? (wid & (kClaimShards - 1)) : wid % nsh;
    const int P = (RO || c.bg) ? 0 : U + bcast(nincl, kWave - 1);   // (background: the spawn jobs are k_spawn's)
    const int T = R + P;
    if (wid == 0 && lane == 0 && R > 0) {
        atomicAdd(&g_resets_run, (unsigned long long)R);
        if (c.diag) atomicAdd(&g_resets_timed, (unsigned long long)R);
    }
    // env of job j of queue q
    // (only the inclusive prefix sums stay live across the jobs: the shard of
    // job j is the number of shards whose prefix ends at or before j)
    auto job_env = [&](int q, int j, int qincl) {
        const int sh = __popcll(__ballot(qincl <= j));
        const int base = sh ? bcast(qincl, sh - 1) : 0;
        return qb[(q * kQShards + sh) * c.q_cap + j - base];
    };
    // job idx < R: the step's resets (high priority, the critical path); then
    // the urgent spawn-ahead jobs, then the others. A worker's first job is its
    // block index, the next ones are claimed once it is free (a slow reset
    // never holds up a job another worker could take): worker w claims on
    // shard x = w % kClaimShards, whose n-th claim is job G + x + kClaimShards * n.
    int idx = wid, nx = 0;
    for (;;) {
        // (the arguments afresh for each job: nothing of them stays live across
        // jobs; so is the lane index, or every lane mask derived from it -- the
        // MT word bounds, the scan steps -- would be held, spilled, for the whole
        // kernel instead of recomputed by one compare)
        const KArgs &J = kargs(kp);
        int lane = threadIdx.x & (kWave - 1);
        __asm__ volatile("" : "+v"(lane));
        if (idx < R) {
            __builtin_amdgcn_s_setprio(3);
            const int e = job_env(0, idx, incl);
            FDBG_ENV_OR_STOP(1, e, J.c.N);
            ITEM_T0();
            WaveMT mt;
            uint32_t cellw;
            const int spst = J.c.bg ? claim_reset_mt(J.c, J.st, e, mt, lane, cellw)
                                    : load_reset_mt(J.c, J.st, e, mt, lane, true, cellw);
            if (J.c.diag && lane == 0 && (spst & 3) == SPAWN_READY) DIAG_ADD(g_spawn_hits);
            if (J.c.diag && lane == 0 && (spst & 3) == SPAWN_PARTIAL) DIAG_ADD(g_reset_part);
            do_reset<MS, JL>(J.c, J.st, J.o, e, mt, lds, wid, spst, cellw, lane);
            ITEM_LOG(wid, 2 - (spst & 3), e);
        } else if (!RO && idx < R + P) {
            if (J.c.spawn_prio == 0) __builtin_amdgcn_s_setprio(0);   // (s_setprio takes an immediate)
            else if (J.c.spawn_prio == 1) __builtin_amdgcn_s_setprio(1);
            else if (J.c.spawn_prio == 2) __builtin_amdgcn_s_setprio(2);
            else __builtin_amdgcn_s_setprio(3);
            const int j = idx - R;
            const int e = j < U ? job_env(1, j, uincl) : job_env(2, j - U, nincl);
            FDBG_ENV_OR_STOP(2, e, J.c.N);
            if (J.c.diag && lane == 0) DIAG_ADD(g_spawn_jobs);
            ITEM_T0();
            do_spawn<MS, JL>(J.c, J.st, e, lds, wid, lane);
            ITEM_LOG(wid, j < U ? 3 : 4, e);
        }
        int v = 0;
        if (lane == 0) v = atomicAdd(&qc[(kQClaim + x) * kQSpread], 1);
        nx = bcast(v, 0);
        idx = G + x + nsh * nx;
        if (idx >= T) break;
    }
    // Every worker ends with exactly one failing claim, so the shard's claims
    // number its jobs + its workers, and the worker whose failing claim is the
    // shard's last finishes the shard. The last shard to finish re-zeroes the
    // step's counters for the next step: every worker has read its counts and
    // made its last claim by then (no host-side step parity, one extra atomic
    // per shard).
    const int jobs_x = T > G + x ? (nsh == kClaimShards ? (T - G - x + kClaimShards - 1) / kClaimShards
                                                       : (T - G - x + nsh - 1) / nsh) : 0;
    const int workers_x = nsh == kClaimShards ? (G - x + kClaimShards - 1) / kClaimShards : (G - x + nsh - 1) / nsh;
    if (nx == jobs_x + workers_x - 1) {
        int d = 0;
        if (lane == 0) d = atomicAdd(&qc[kQDone * kQSpread], 1);
        if (bcast(d, 0) == nsh - 1)   // (background: the reset counters only)
            for (int q = lane; q < kQSpGen; q += kWave)
                if (!c.bg || q < kQShards || (q >= kQClaim && q <= kQDone)) qc[q * kQSpread] = 0;
    }
}

}  // namespace snake
