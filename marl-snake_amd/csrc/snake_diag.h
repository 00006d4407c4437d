// snake_diag.h -- the diagnostics of snake_kernels.hip: the always-on counters
// (snake_timing_read) and, in the -DSNAKE_STAMPS / -DSNAKE_FUSE_DEBUG builds, the
// stamps and range checks with their extern "C" readers; empty macros otherwise.
// (SNAKE_DIAG_ENC2 / SNAKE_DIAG_NO_ENCODE: one line each in k_post.)
#pragma once

namespace snake {
__device__ unsigned long long g_resets_run;     // auto-resets run (snake_timing_read "resets")
__device__ unsigned long long g_resets_timed;   // the same, while timing is enabled ("resets_timed")
// (diagnostic counters, spread over 64 lines by block: one address taking a
// device-scope atomic per job serialised thousands of them on the timed steps)
constexpr int kDiagSlots = 64, kDiagSpread = 16;
__device__ unsigned long long g_spawn_hits[kDiagSlots * kDiagSpread];   // auto-resets that found a ready record
__device__ unsigned long long g_spawn_jobs[kDiagSlots * kDiagSpread];   // spawn-ahead jobs dequeued
__device__ unsigned long long g_spawn_void[kDiagSlots * kDiagSpread];   // ready records voided by a fruit draw
__device__ unsigned long long g_reset_part[kDiagSlots * kDiagSpread];   // auto-resets that found a partial record
__device__ unsigned long long g_resp_slow[kDiagSlots * kDiagSpread];    // k_logic respawns on the full-wave path (no room)
__device__ unsigned long long g_resp_slow2[kDiagSlots * kDiagSpread];   // ... (room, too few accepts among the prefetched raws)
__device__ unsigned long long g_gate_shut[kDiagSlots * kDiagSpread];    // k_logic waves that found the background queue set busy
__device__ unsigned long long g_draw_wait[kDiagSlots * kDiagSpread];    // resets that waited for a background job (DRAWING)
__device__ unsigned long long g_draw_timeout[kDiagSlots * kDiagSpread]; // ... and gave up waiting (drew from the env's own state)
__device__ unsigned long long g_fused_timeout[kDiagSlots * kDiagSpread]; // k_step waits that ran into kFuseWait
#define DIAG_ADD(arr) atomicAdd(&(arr)[(blockIdx.x % kDiagSlots) * kDiagSpread], 1ull)
// the counters by their snake_timing_read names (read as the sum of their words, then zeroed)
constexpr int kDiagWords = kDiagSlots * kDiagSpread;
static const struct DiagCounter { const char *name; const void *sym; int words; } kDiagCounters[] = {
    {"resets", &g_resets_run, 1}, {"resets_timed", &g_resets_timed, 1}, {"spawn_hits", g_spawn_hits, kDiagWords},
    {"spawn_jobs", g_spawn_jobs, kDiagWords}, {"spawn_void", g_spawn_void, kDiagWords},
    {"reset_partial", g_reset_part, kDiagWords}, {"respawn_slow", g_resp_slow, kDiagWords},
    {"respawn_slow2", g_resp_slow2, kDiagWords}, {"gate_shut", g_gate_shut, kDiagWords},
    {"draw_wait", g_draw_wait, kDiagWords}, {"draw_timeout", g_draw_timeout, kDiagWords},
    {"fused_timeout", g_fused_timeout, kDiagWords}};

#ifdef SNAKE_FUSE_DEBUG
// (diagnostic build: range checks on the fused step's indices; a violation is
// recorded -- site, value -- and the access skipped)
__device__ unsigned long long g_fdbg[64];
#define FDBG_BAD(site, val) (atomicAdd(&g_fdbg[2 * (site)], 1ull), atomicMax(&g_fdbg[2 * (site) + 1], (unsigned long long)(uint32_t)(val)), true)
#define FDBG_MARK(site) do { if ((threadIdx.x & 63) == 0) atomicAdd(&g_fdbg[2 * (site)], 1ull); } while (0)
// (inside autoreset_worker's job loop: a queued env outside [0, n) ends the worker)
#define FDBG_ENV_OR_STOP(site, e, n) if (((e) < 0 || (e) >= (n)) && FDBG_BAD(site, e)) { idx = 1 << 30; break; }
#else
#define FDBG_BAD(site, val) false
#define FDBG_MARK(site) do {} while (0)
#define FDBG_ENV_OR_STOP(site, e, n)
#endif

#ifdef SNAKE_STAMPS
// Diagnostic build only (scripts/logic_stamps.py): s_memtime stamps of block
// 0's wave at k_logic's phase boundaries, and s_memrealtime (100 MHz) at every
// k_logic wave's start and end (its block index, up to kWaveTimes blocks).
constexpr int kWaveTimes = 8192, kPostTimes = 40960;
__device__ unsigned long long g_stamps[64];
__device__ unsigned long long g_wavetime[2 * kWaveTimes];
__device__ unsigned long long g_posttime[2 * kPostTimes];   // k_post: every block's start and end
#define PTIME(end)                                                                 \
    do {                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                         \
        if ((threadIdx.x & 63) == 0 && blockIdx.x < kPostTimes)                    \
            g_posttime[2 * blockIdx.x + (end)] = __builtin_amdgcn_s_memrealtime(); \
        __builtin_amdgcn_sched_barrier(0);                                         \
    } while (0)
// (and every k_logic wave's s_memrealtime at each phase: g_wphase[wave][idx - 40])
__device__ unsigned long long g_wphase[16 * kWaveTimes];
#define LSTAMP(idx)                                                                \
    do {                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                         \
        if (blockIdx.x == 0) {                                                     \
            unsigned long long _t = __builtin_amdgcn_s_memtime();                  \
            if (threadIdx.x == 0) g_stamps[idx] = _t;                              \
        }                                                                          \
        const unsigned _w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);  \
        if ((threadIdx.x & 63) == 0 && _w < kWaveTimes)                            \
            g_wphase[16 * _w + (idx) - 40] = __builtin_amdgcn_s_memrealtime();     \
        __builtin_amdgcn_sched_barrier(0);                                         \
    } while (0)
#define WTIME(end)                                                                 \
    do {                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                         \
        const unsigned _w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);  \
        if ((threadIdx.x & 63) == 0 && _w < kWaveTimes)                            \
            g_wavetime[2 * _w + (end)] = __builtin_amdgcn_s_memrealtime();         \
        __builtin_amdgcn_sched_barrier(0);                                         \
    } while (0)
// every reset-worker item (scripts/post_items.py): worker | type << 32, start,
// end (s_memrealtime), env; types 0 reset from a ready record, 1 from a partial
// one, 2 without one, 3 queue-1 spawn-ahead job, 4 queue-2 job
constexpr int kItems = 16384;
__device__ unsigned g_nitems;
__device__ unsigned long long g_items[4 * kItems];
#define ITEM_T0() const unsigned long long _it0 = __builtin_amdgcn_s_memrealtime()
#define ITEM_LOG(wid, type, e)                                                                      \
    do {                                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        const unsigned long long _it1 = __builtin_amdgcn_s_memrealtime();                          \
        if ((threadIdx.x & 63) == 0) {                                                             \
            const unsigned _i = atomicAdd(&g_nitems, 1u);                                          \
            if (_i < kItems) {                                                                     \
                g_items[4 * _i] = (unsigned long long)(wid) | ((unsigned long long)(type) << 32);   \
                g_items[4 * _i + 1] = _it0; g_items[4 * _i + 2] = _it1;                             \
                g_items[4 * _i + 3] = (unsigned long long)(e);                                     \
            }                                                                                      \
        }                                                                                          \
    } while (0)
#else
#define ITEM_T0() do {} while (0)
#define ITEM_LOG(wid, type, e) do {} while (0)
#define LSTAMP(idx) do {} while (0)
#define WTIME(end) do {} while (0)
#define PTIME(end) do {} while (0)
#endif

}  // namespace snake

#ifdef SNAKE_FUSE_DEBUG
extern "C" int snake_debug_fdbg(unsigned long long *out)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(snake::g_fdbg), sizeof(unsigned long long) * 64) == hipSuccess ? 0 : -1;
}
#endif

#ifdef SNAKE_STAMPS
// out: 16 * 8192 per-wave phase realtimes of the last k_logic (g_wphase)
extern "C" int snake_debug_wphase(unsigned long long *out)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(snake::g_wphase), sizeof(unsigned long long) * 16 * snake::kWaveTimes) ==
                   hipSuccess ? 0 : -1;
}

// out: the reset workers' items of the launches since the last call (4 words
// each, see g_items), at most cap; returns their number
extern "C" int snake_debug_items(unsigned long long *out, int cap)
{
    unsigned n = 0, z = 0;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(snake::g_nitems), sizeof n) != hipSuccess) return -1;
    n = std::min<unsigned>(n, (unsigned)std::min(cap, snake::kItems));
    if (n && hipMemcpyFromSymbol(out, HIP_SYMBOL(snake::g_items), sizeof(unsigned long long) * 4 * n) != hipSuccess)
        return -1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(snake::g_nitems), &z, sizeof z) != hipSuccess) return -1;
    return (int)n;
}

// out: 64 phase stamps of block 0, 2 * 8192 k_logic wave start/end realtimes,
// 2 * 40960 k_post block start/end realtimes
extern "C" int snake_debug_stamps(unsigned long long *out)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(snake::g_stamps), sizeof(unsigned long long) * 64) != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out + 64, HIP_SYMBOL(snake::g_wavetime),
                            sizeof(unsigned long long) * 2 * snake::kWaveTimes) != hipSuccess) return -1;
    return hipMemcpyFromSymbol(out + 64 + 2 * snake::kWaveTimes, HIP_SYMBOL(snake::g_posttime),
                               sizeof(unsigned long long) * 2 * snake::kPostTimes) == hipSuccess ? 0 : -1;
}
#endif
