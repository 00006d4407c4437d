// snake_kernels.hip -- the batched multi-snake env step on CDNA4 (gfx950): the
// kernels. One translation unit; the device code they run is in the step_*.h
// headers beside this file, the host layer in snake_launch.inc:
//   step_args.h    KArgs / kargs (arguments through the kernarg segment), the
//                  cell codes, the address-space views;
//   step_lanes.h   link-table access, wave and DPP lane-group exchanges (gsel,
//                  gscan), small arithmetic, the sc1 loads and stores;
//   step_mt.h      MT19937 in a wave's registers: twist, tempering, mt_draw;
//   step_perm.h    the reset's permutation: Fisher-Yates draws in ballot-refined
//                  rounds recording the draws, trace of arr[:S];
//   step_encode.h  the NHWC one-hot observation from the grid ring: direct, lean
//                  and row-wise encodes, and the table encode (encode_tbl_block,
//                  16-byte non-temporal stores);
//   step_reset.h   fruit draws, spawn attempts and spawn-ahead records, do_reset
//                  (paint, fruits, encode), the reset worker's job loop;
//   step_logic.h   logic_body: the game rules (snake_env.py:301-374)
//                  lane-parallel, lane (env g, snake k), 4, 8 or 16 lanes per env,
//                  the envs' current grids staged in LDS with 16-byte loads:
//                  targets, collision groups (DPP moves inside the env's lane
//                  group), the fruit-eater tail rule, rewards, and a two-phase
//                  grid update (all tail clears, then all BODY/HEAD/TAIL writes)
//                  that reproduces the reference's snake-order update exactly
//                  ("two-phase update"); dead-body erase
//                  (prefix-scanned direction deque), fruit respawn (lane-chunked
//                  empty-cell ranking + MT19937 rejection sampling resolved by
//                  ballots); envs whose dones are all True are queued;
//   step_fused.h   k_step's claim / wait protocol;
//   snake_diag.h   the counters and the diagnostic builds' stamps.
// snake_step = k_logic, then one shared-phase launch (k_post / k_post_lean:
// reset workers + encodes), with the spawn-ahead attempts in the step or in
// k_spawn on the library's background streams (launch_step).
// Compiled with -ffp-contract=off: rewards/statistics are float64 in the
// reference's order of operations (snake_env.py:365-369, :385-389).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>
#include <mutex>
#include <type_traits>
#include <utility>

#include "snake_internal.h"
#include "snake_device.h"
#include "snake_diag.h"
#include "step_args.h"
#include "step_lanes.h"
#include "step_mt.h"
#include "step_perm.h"
#include "step_encode.h"
#include "step_reset.h"
#include "step_logic.h"
#include "step_fused.h"

constexpr int kResetWavesPerEU = 4;   // reset workers: 128 VGPRs (3 waves/SIMD measured slower)

namespace snake {

// WPB waves per workgroup, each an independent group of envs (no barrier):
// fewer, larger workgroups for the dispatcher.
// BG: background spawn-ahead (KCfg.bg), its queue-set gate and status-word
// atomics; the in-step form carries none of it
template <int MS, int WPB, bool BG>
__global__ void __launch_bounds__(64 * WPB) k_logic(const KArgs)
{
    const KPtr kp = kernel_args();
    WTIME(0);
    const int blk = (int)blockIdx.x * WPB + (int)(threadIdx.x >> 6);
    if (blk * (kWave / MS) >= kargs(kp).c.N) return;
    LogicIn in;
    logic_load<MS, BG>(kp, blk, in);
    logic_body<MS, BG>(kp, blk, in);
    WTIME(1);
}

template <int MS, bool RO, int JL>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kResetWavesPerEU))) k_autoreset(const KArgs)
{
    const KPtr kp = kernel_args();
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    autoreset_worker<MS, RO, JL>(kp, (int)blockIdx.x, (int)gridDim.x, lds);
}

// Background spawn-ahead (KCfg.bg): the step's spawn-ahead jobs, run by
// spawn_slots one-wave workers on a stream of their own that no step waits for
// except the one two steps later, whose k_logic refills this queue set
// (launch_step); do_spawn_bg says how they stay out of the resets' way. Jobs
// are claimed on 16 claim shards like k_autoreset's, whose last worker
// re-zeroes the set's spawn counters.
template <int MS>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kResetWavesPerEU))) k_spawn(const KArgs)
{
    const KPtr kp = kernel_args();
    const KArgs &A = kargs(kp);
    const KCfg &c = A.c;
    const snake_state &st = A.st;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = threadIdx.x;
    if (c.spawn_prio == 0) __builtin_amdgcn_s_setprio(0);
    else if (c.spawn_prio == 1) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(2);
    int *qb = st.resetq + (int64_t)c.qpar * (kNumQ * kQShards * c.q_cap + kQCounters);
    int *qc = qb + kNumQ * kQShards * c.q_cap;
    const int ucnt = qc[(kQShards + lane) * kQSpread], ncnt = qc[(2 * kQShards + lane) * kQSpread];
    const int uincl = wave_scan(ucnt, lane), nincl = wave_scan(ncnt, lane);
    const int U = bcast(uincl, kWave - 1), T = U + bcast(nincl, kWave - 1);
    const int G = (int)gridDim.x, nsh = min(G, kClaimShards);
    const int x = G >= kClaimShards ? (int)(blockIdx.x & (kClaimShards - 1)) : (int)blockIdx.x % nsh;
    auto job_env = [&](int q, int j, int qincl) {
        const int sh = __popcll(__ballot(qincl <= j));
        const int base = sh ? bcast(qincl, sh - 1) : 0;
        return qb[(q * kQShards + sh) * c.q_cap + j - base];
    };
    int nx = -1;   // (a worker with no first job makes one failing claim below)
    int idx = blockIdx.x;
    if (idx >= T) {
        int v = 0;
        if (lane == 0) v = atomicAdd(&qc[(kQSpClaim + x) * kQSpread], 1);
        nx = bcast(v, 0);
    }
    for (; idx < T;) {
        const int ent = idx < U ? job_env(1, idx, uincl) : job_env(2, idx - U, nincl);
        const int e = ent & ((1 << (32 - kQGenBits)) - 1);
        const uint32_t qgen = (uint32_t)ent >> (32 - kQGenBits);
        if (c.diag && lane == 0) DIAG_ADD(g_spawn_jobs);
        const KArgs &J = kargs(kp);
        do_spawn_bg<MS>(J.c, J.st, e, qgen, lds, lane);
        int v = 0;
        if (lane == 0) v = atomicAdd(&qc[(kQSpClaim + x) * kQSpread], 1);
        nx = bcast(v, 0);
        idx = G + x + nsh * nx;
    }
    // the shard's last claim finishes the shard; the last shard re-zeroes (as in
    // k_autoreset, with this kernel's claim and done counters)
    const int jobs_x = T > G + x ? (T - G - x + nsh - 1) / nsh : 0;
    const int workers_x = (G - x + nsh - 1) / nsh;
    if (nx == jobs_x + workers_x - 1) {
        int d = 0;
        if (lane == 0) d = atomicAdd(&qc[kQSpDone * kQSpread], 1);
        if (bcast(d, 0) == nsh - 1) {
            // write-through zeroes, drained, then the set's finished count: a
            // k_logic that reads the count (sc1) then adds to these counters
            // from any XCD (MI355X_MICROARCH.md, inter-workgroup hand-off)
            for (int q = kQShards + lane; q < kNumQ * kQShards; q += kWave)
                st_sc1(reinterpret_cast<uint32_t *>(&qc[q * kQSpread]), 0u);
            if (lane <= kClaimShards) st_sc1(reinterpret_cast<uint32_t *>(&qc[(kQSpClaim + lane) * kQSpread]), 0u);   // (claims + done)
            __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == 0) atomicAdd(reinterpret_cast<unsigned *>(&qc[kQSpGen * kQSpread]), 1u);
        }
    }
}

__global__ void __launch_bounds__(64) k_encode(const KCfg c, const snake_state st, const snake_out o)
{
    encode_one(c, st, o, (int)blockIdx.x);
}

// (four waves per SIMD: at most 128 VGPRs; the rules alone take 100, the
// worker path in k_post 71)
template <int MS, int NPW, int JL>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) k_step(const KArgs)
{
    const KPtr kp = kernel_args();
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    PTIME(0);
    const int b = (int)blockIdx.x;
    const int nlg = kargs(kp).c.nlg, G = kargs(kp).c.reset_slots;
    const int roles = kargs(kp).c.fu_roles;   // (snake_debug_set "fuse_roles": 7 = all)
    const int role = b < nlg ? 0 : (b < nlg + G ? 1 : 2);   // rules, reset worker, encodes
    if (!(roles & (1 << role))) return;
    const int j = b - nlg - G;   // (encodes: envs 4j .. 4j + 3, all of logic group 4j / (64 / MS))
    const int eg = (4 * j) / (kWave / MS);
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    int scan = -1;
    // the rules of every group this wave claims, at ONE inlined site
    for (int it = 0;; it++) {
        int grp = -1;
        if (role == 0) {
            if (it == 0 && fused_claim(kp, b)) grp = b;
        } else if (role == 2) {
            if (it == 0 && !fused_group_done(kp, eg) && fused_claim(kp, eg)) grp = eg;
        } else {
            grp = fused_wait_all(kp, b - nlg, t0, scan);
        }
        if (grp < 0) break;
        LogicIn in;
        logic_load<MS, false>(kp, grp, in);
        logic_body<MS, false, true>(kp, grp, in);
        FDBG_MARK(3);
    }
    if (role == 0) { PTIME(1); return; }
    if (role == 1) {
        // the queues, env records, MT keys and spawn records the groups published
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
        FDBG_MARK(4);
        autoreset_worker<4, false, JL>(kp, b - nlg, G, lds);
        FDBG_MARK(5);
        PTIME(1);
        return;
    }
    if (4 * j >= kargs(kp).c.N && FDBG_BAD(6, j)) return;
    fused_wait_group(kp, eg);
    FDBG_MARK(7);
    const KArgs &A = kargs(kp);
    encode_tbl_block<NPW, kWave, true>(A.c, A.st, A.o, j);
    PTIME(1);
}

// The shared phase as one launch: blocks [0, reset_slots) are the reset workers
// (autoreset_worker), the rest the encodes (NPF = 0: one env per block,
// encode_one; else encode_multi<NPF>). Dispatched in block order, so the workers
// go first; one launch instead of a fork onto a side stream and a join (round 3:
// cfg3 0.0970 -> 0.0941 ms, cfg2 0.0591 -> 0.0539); the kernel's registers and
// LDS are the larger of the two. JL: the workers' draw record (1) or u32 link
// table (2) in LDS, else their global link tables (boards of more than 18 368
// spawn poses).
// NPF > 0: encode_multi<NPF>; 0: encode_one; -NPW: encode_tbl_block<NPW>
// Table encode (NPF < 0): workgroups of c.enc_wpb waves. In a worker workgroup
// only wave 0 works, the others return at once; wave w of encode workgroup b
// encodes env group (b - G) * enc_wpb + w on its own LDS slice, no workgroup
// barrier anywhere (as k_logic's four waves) -- the launch's LDS, the larger
// of the workers' record and enc_wpb table carves, is then charged once per
// enc_wpb encode waves instead of once per wave.
template <int MS, int NPF, bool RO, int JL>
__global__ void __launch_bounds__(NPF < 0 ? kWave * kEncWpbMax : kWave) k_post(const KArgs)
{
    const KPtr kp = kernel_args();
    PTIME(0);
    const int G = kargs(kp).c.reset_slots, b = (int)blockIdx.x;
    int wave = 0;
    if constexpr (NPF < 0) wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (b < G) {
        if (wave) return;
        extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
#ifdef SNAKE_DIAG_ENC2   // (diagnostic: the second, encode-only launch, see launch_step)
        if (kargs(kp).aux) return;
#endif
        autoreset_worker<MS, RO, JL>(kp, b, G, lds);
    } else {
#ifdef SNAKE_DIAG_NO_ENCODE   // (diagnostic build: instruction counts without the encodes)
        return;
#endif
        const KArgs &A = kargs(kp);
        if constexpr (NPF == 0) encode_one(A.c, A.st, A.o, b - G);
        else if constexpr (NPF < 0) {
            const int grp = (b - G) * A.c.enc_wpb + wave;
            if (grp * A.c.enc_per_wave >= A.c.N) return;   // (the last workgroup's spare waves)
            encode_tbl_block<-NPF>(A.c, A.st, A.o, grp, wave);
        }
        else encode_multi<NPF>(A.c, A.st, A.o, b - G);
    }
    PTIME(1);
}

// The shared phase of a board with four-wave lean encodes (cfg5) as one launch:
// workgroups [0, ceil(reset_slots / 4)) hold four independent workers each
// (wave w of workgroup b is worker 4b + w, with its own KCfg.lds_worker bytes of
// LDS -- frames, centres, fruit buffer, no draw record -- and its own global
// link table for the attempts it runs: no workgroup barrier on their path), the
// rest are lean-encode workgroups. RO: background spawn-ahead (the default on
// these boards), the workers run the resets only; else also the in-step
// spawn-ahead attempts. One launch instead of the fork/join of round 2 (12 and
// 16 us of cross-stream latency per step at cfg5).
template <int MS, bool RO, bool TBL>
__global__ void __launch_bounds__(256) k_post_lean(const KArgs)
{
    const KPtr kp = kernel_args();
    PTIME(0);
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int G = kargs(kp).c.reset_slots, GB = (G + 3) >> 2, b = (int)blockIdx.x;
    if (b < GB) {
        const int wave = (int)(threadIdx.x >> 6), wid = 4 * b + wave;
        if (wid < G) autoreset_worker<MS, RO, 0>(kp, wid, G, lds + wave * kargs(kp).c.lds_worker);
    } else {
        const KArgs &A = kargs(kp);
        if constexpr (TBL) encode_tbl_block<8, 256>(A.c, A.st, A.o, b - GB);
        else encode_lean_block<8, 256>(A.c, A.st, A.o, b - GB);
    }
    PTIME(1);
}

template <int MS, int JL>
__global__ void __launch_bounds__(64) k_reset(const KArgs)
{
    const KPtr kp = kernel_args();
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = threadIdx.x;
    // one env per block with the link table in LDS (JL), else reset_slots
    // workers striding over the envs, each with its own global link table
    for (int e = blockIdx.x; e < kargs(kp).c.N; e += gridDim.x) {
        const KArgs &J = kargs(kp);
        const uint8_t *mask = (const uint8_t *)J.aux;
        if (mask && !mask[e]) continue;
        WaveMT mt;
        uint32_t cellw;
        const int spst = J.c.bg ? load_reset_mt_bg(J.c, J.st, e, mt, lane, cellw)
                                : load_reset_mt(J.c, J.st, e, mt, lane, true, cellw);
        do_reset<MS, JL>(J.c, J.st, J.o, e, mt, lds, blockIdx.x, spst, cellw, lane);
        // with spawn-ahead on, the next reset's poses are drawn now, off the step
        const KArgs &J2 = kargs(kp);
        if (J2.c.spawn_thr >= 0) spawn_after_reset<MS, JL>(J2.c, J2.st, e, mt, lds, blockIdx.x, lane);
    }
}

// np.random.seed(s): mt19937_seed (init_genrand), pos = 624.
__global__ void k_seed(const KCfg c, const snake_state st, uint32_t base, long long off)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.N) return;
    uint32_t s = base + (uint32_t)(off + e);
    uint32_t *g = st.mt + (int64_t)e * kMtN;
    for (int pos = 0; pos < kMtN; pos++) {
        g[pos] = s;
        s = 1812433253u * (s ^ (s >> 30)) + (uint32_t)pos + 1u;
    }
    st.env[(int64_t)e * kEnvRec + ENV_MTPOS] = kMtN;
    st.env[(int64_t)e * kEnvRec + ENV_SPAWN] = SPAWN_NONE;
}

// rgb_from_grid (grid_util.py:164-175) of every env's current grid: a palette
// lookup per cell. Each thread writes 4 consecutive cells of the flat
// [N][H][W] image as three 4-byte stores (12 bytes at a 12-byte offset; cells
// past the last whole quad go byte by byte). HBM-bound: reads one
// ring byte and writes 3 bytes per cell, plus the 4-byte cur index per env.
struct RenderPal {
    uint8_t rgb[6 * kMaxSnakes * 3];
};

__device__ __forceinline__ uint32_t render_cell(const KCfg &c, const snake_state &st,
                                                const RenderPal &pal, long long x)
{
    const long long e = x / c.HW;
    const int cell = (int)(x - e * c.HW);
    const int cur = st.env[e * kEnvRec + ENV_CUR];
    const int v = st.grid[e * c.ring_bytes + (long long)cur * c.grid_stride + cell];
    const int code = v % 10, id = v / 10;
    if (code > 5 || id >= kMaxSnakes) return 0u;   // not a reachable grid value
    const uint8_t *p = pal.rgb + (code * kMaxSnakes + id) * 3;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

__global__ void k_render(const KCfg c, const snake_state st, const RenderPal pal, uint8_t *rgb)
{
    const long long total = (long long)c.N * c.HW;
    const long long x0 = 4ll * ((long long)blockIdx.x * blockDim.x + threadIdx.x);
    if (x0 >= total) return;
    if (x0 + 4 <= total) {
        uint32_t q[4];
#pragma unroll
        for (int t = 0; t < 4; t++) q[t] = render_cell(c, st, pal, x0 + t);
        uint32_t *dst = reinterpret_cast<uint32_t *>(rgb + 3 * x0);
        dst[0] = q[0] | (q[1] << 24);
        dst[1] = (q[1] >> 8) | (q[2] << 16);
        dst[2] = (q[2] >> 16) | (q[3] << 8);
    } else {
        for (long long x = x0; x < x0 + 4 && x < total; x++) {
            const uint32_t q = render_cell(c, st, pal, x);
            rgb[3 * x] = (uint8_t)q;
            rgb[3 * x + 1] = (uint8_t)(q >> 8);
            rgb[3 * x + 2] = (uint8_t)(q >> 16);
        }
    }
}

}  // namespace snake

#include "snake_launch.inc"   // the host layer
#ifdef SNAKE_DRAWBENCH   // (diagnostic build: the draw / attempt benchmarks, which use the device functions above)
#include "../../scripts/microbench/drawbench.inc"
#endif
