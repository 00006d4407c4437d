// step_fused.h -- the fused step's (k_step) claim / wait protocol between its
// logic groups, encode blocks and reset workers.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "snake_internal.h"
#include "snake_diag.h"
#include "step_args.h"
#include "step_lanes.h"

namespace snake {

// ------------------------------------------------------------ fused step
// k_step (round 6): the whole step as ONE launch on boards whose encodes take
// the table form in one wave and whose hand-off record holds the crop centres
// (one frame, S <= 4: cfg2, cfg3, cfg4), no background spawn kernel. Blocks
// [0, nlg) are k_logic's env groups, the next reset_slots blocks the reset
// workers, the rest the table encodes (4 envs each). The encodes of a group
// start as soon as that group's rules are done instead of after the last
// group and a kernel boundary, so k_logic's latency chain runs beside the
// encodes' stores.
// Dispatch order, timing and placement are not assumed (MI355X_MICROARCH.md
// "Workgroup dispatch", contract [G]): every logic group is CLAIMED (an atomic
// exchange of the step's epoch) by whichever wave gets it first -- its own
// block, or an encode block of that group that finds it unclaimed, or a reset
// worker that has waited long -- and the claimer runs it at once without
// waiting on anything. A wave waits only for a group that is claimed, i.e.
// running, so the launch cannot deadlock.
// Hand-offs (R1 of the guide's visibility rules): the logic wave's stores that
// another wave of the launch reads or writes are write-through (sc1) stores --
// the new frame, the env record, the queue entries, the spawn status word, a
// rewritten MT key, the encodes' hand-off record -- drained (vmcnt(0)) before
// the group's done flag (sc1 store of the epoch) and its logic-done count (an
// atomic add on shard blk % 64); an env whose episode ended stores nothing its
// auto-reset rewrites. The encodes poll the flag and read their inputs with sc1
// loads only; the workers poll the 64 counts, then one agent-scope acquire,
// then the queues and env state as before. Epochs: the library's per-state step
// count (launch_step); the counts grow by their shard's group count per step.
// Every wait is bounded (kFuseWait): past it the wave carries on and the launch
// counts the timeout ("fused_timeout"), the results are then undefined.
constexpr unsigned long long kFuseWait = 10000000ull;   // 100 ms of the 100 MHz clock
constexpr unsigned long long kFuseHelp = 2000ull;       // 20 us: a waiting worker then claims unclaimed groups

// (Everything here takes k_step's kernarg pointer as an argument: round 6 read
// the segment pointer inside these functions, which a called function does not
// have -- an out-of-line fused_logic read its KCfg from garbage and faulted.)
__device__ __forceinline__ bool fused_claim(KPtr kp, const int g)
{
    const KCfg &c = kargs(kp).c;
    uint32_t *claim = reinterpret_cast<uint32_t *>(kargs(kp).st.resetq + c.fu_claim) + g;
    int won = 0;
    if ((threadIdx.x & (kWave - 1)) == 0) won = atomicExch(claim, c.epoch) != c.epoch ? 1 : 0;
    return __shfl(won, 0) != 0;
}

__device__ __forceinline__ bool fused_group_done(KPtr kp, const int g)
{
    const KCfg &c = kargs(kp).c;
    const uint32_t *done = reinterpret_cast<const uint32_t *>(kargs(kp).st.resetq + c.fu_done) + g;
    return (uint32_t)__shfl((int)ld_sc1(done), 0) == c.epoch;
}

// an encode block's wait for its group's rules, which some wave has claimed
__device__ __forceinline__ void fused_wait_group(KPtr kp, const int g)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (!fused_group_done(kp, g)) {
        if (__builtin_amdgcn_s_memrealtime() - t0 > kFuseWait) {
            if ((threadIdx.x & (kWave - 1)) == 0) DIAG_ADD(g_fused_timeout);
            return;
        }
        __builtin_amdgcn_s_sleep(4);
    }
}

// A reset worker's wait for every group's rules (the queues complete): -1 once
// they are done (or the wait timed out), else a group it has just claimed and
// must run -- once it has waited kFuseHelp, every group still unclaimed, from a
// worker-specific start (`scan`: the next scan position, -1 before the first)
__device__ __forceinline__ int fused_wait_all(KPtr kp, const int wid, const unsigned long long t0, int &scan)
{
    const int lane = threadIdx.x & (kWave - 1);
    for (;;) {
        const KCfg &c = kargs(kp).c;
        const int nlg = c.nlg;
        // shard s (lane s) counts the groups g = s mod 64: (nlg - s + 63) / 64 of them per step
        const uint32_t ns = lane < nlg ? (uint32_t)((nlg - lane + kQShards - 1) / kQShards) : 0u;
        const uint32_t v = ld_sc1(reinterpret_cast<const uint32_t *>(kargs(kp).st.resetq + c.fu_ldone) + lane * kQSpread);
        if (__ballot(v != c.epoch * ns) == 0ull) return -1;
        const unsigned long long dt = __builtin_amdgcn_s_memrealtime() - t0;
        if (dt > kFuseWait) {
            if (lane == 0) DIAG_ADD(g_fused_timeout);
            return -1;
        }
        if (dt > kFuseHelp && scan < nlg) {
            if (scan < 0) scan = 0;
            for (; scan < nlg; scan += kWave) {
                const int g = (wid * 61 + scan + lane) % nlg;
                const KCfg &c2 = kargs(kp).c;
                const uint32_t cl = scan + lane < nlg ? ld_sc1(reinterpret_cast<const uint32_t *>(kargs(kp).st.resetq + c2.fu_claim) + g)
                                                      : c2.epoch;
                unsigned long long m = __ballot(cl != c2.epoch);
                while (m) {
                    const int L = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const int gg = __shfl(g, L);
                    if (fused_claim(kp, gg)) return gg;   // (the next call rescans this pass)
                }
            }
        }
        __builtin_amdgcn_s_sleep(8);
    }
}

}  // namespace snake
