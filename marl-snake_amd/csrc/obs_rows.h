// obs_rows.h -- the observation front end of k_safe_actions (policy_kernels.hip)
// and k_greedy (greedy_kernels.hip): a wave's cells -> per-flag bit strings in
// LDS -> one w-bit row word per flag and lane, and the argument
// checks their entry points share. Include after <hip/hip_runtime.h> and
// snake_internal.h.
#pragma once

namespace snake {

constexpr int kMaxSide = 64;       // rows on lanes, columns on the bits of a 64-bit word

// 64-bit words of one flag's bit string for a wave of `cells` cells: two per
// pass (the cells and one cell of alignment, 128 a pass), the zero word after
// the last pass, and a spare that keeps the count even
constexpr int flag_words(int cells) { return 2 * ((cells + 1 + 127) / 128) + 2; }

// 0x80 in every byte of x that equals 1 (exact per byte: no carry crosses a byte):
// the channel == 1 tests of the kernels' cell_flags
__device__ __forceinline__ uint32_t bytes_eq1(uint32_t x)
{
    const uint32_t y = x ^ 0x01010101u;
    const uint32_t t = (y & 0x7f7f7f7fu) + 0x7f7f7f7fu;
    return ~(t | y | 0x7f7f7f7fu);
}

struct FlagStrings {
    int d;          // bit 0 of every string is cell first - d: the start rounded down to 16 bytes
    int count;      // set bits of the flags in COUNT
};

// The wave's cells [first, first + count) of obs (8 bytes each, `cells` in the
// whole tensor) as K bit strings lin[k * nw ...], bit d + p of string k = flag k
// of cell first + p, flags(lo, hi) giving a cell's K flag bits from its channels
// 0-3 and 4-7. 16-byte loads, two cells per lane and 128 per pass; two lane
// exchanges put cell p of the pass on lane p % 64, so one __ballot per flag and
// half-pass is a 64-bit word of the string, stored by lane 0. The word after
// the last pass is zero: a row that ends in the last written word reads it too.
// Needs 2 * passes < nw (flag_words); ends with the wave's fence and barrier, so
// every lane may read every word.
template <int K, uint32_t COUNT, class F>
__device__ __forceinline__ FlagStrings load_flag_strings(const uint8_t *obs, long long cells, long long first,
                                                         int count, uint64_t *lin, int nw, int lane, F flags)
{
    const long long a0 = first & ~1ll;      // (16-byte aligned start)
    FlagStrings r;
    r.d = (int)(first - a0);
    r.count = 0;
    const int passes = (count + r.d + 127) >> 7;
    for (int i = 0; i < passes; i++) {
        const long long c = a0 + (long long)i * 128 + 2 * lane;
        const int rel = (int)(c - first);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (rel < count) {
            if (c + 1 < cells) v = *reinterpret_cast<const uint4 *>(obs + c * 8);
            else {      // the very last cell of an odd tensor
                const uint2 t = *reinterpret_cast<const uint2 *>(obs + c * 8);
                v.x = t.x;
                v.y = t.y;
            }
        }
        const uint32_t f0 = (rel >= 0 && rel < count) ? flags(v.x, v.y) : 0;
        const uint32_t f1 = (rel + 1 < count) ? flags(v.z, v.w) : 0;
        const int pk = (int)(f0 | f1 << 8), sh = 8 * (lane & 1);
        const uint32_t fa = (uint32_t)__shfl(pk, lane >> 1) >> sh;          // cell i*128 + lane
        const uint32_t fb = (uint32_t)__shfl(pk, 32 + (lane >> 1)) >> sh;   // cell i*128 + 64 + lane
        uint64_t wa[K], wb[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            wa[k] = __ballot((fa >> k) & 1);
            wb[k] = __ballot((fb >> k) & 1);
            if ((COUNT >> k) & 1) r.count += __popcll(wa[k]) + __popcll(wb[k]);
        }
        if (lane == 0) {        // (one guarded block for the K strings, not one per flag)
#pragma unroll
            for (int k = 0; k < K; k++) {
                lin[k * nw + 2 * i] = wa[k];
                lin[k * nw + 2 * i + 1] = wb[k];
            }
        }
    }
    if (lane < K) lin[lane * nw + 2 * passes] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    return r;
}

// Bits [start, start + 64) of the string `str`: words start / 64 and the next,
// shifted; the caller masks it to its row's w bits. start < count + d <= 128 *
// passes, so the second index is at most 2 * passes: a written word or the zero
// after them. (One string at a time, looped over by the caller: the row words
// reach the kernel as values, and it compiles as the code written in place did;
// a cut of all K strings into an array passed by reference did not.)
__device__ __forceinline__ uint64_t cut_row(const uint64_t *str, int start)
{
    const int idx = start >> 6, sh = start & 63;
    const uint64_t lo = str[idx], hi = str[idx + 1];
    return (lo >> sh) | (sh ? hi << (64 - sh) : 0);
}

// The checks every observation-policy entry point `fn` starts with: the plan,
// the buffers, and num_envs; *nothing: a valid call of no envs, without a launch.
inline int check_obs_call(const char *fn, const snake_policy_cfg *cfg, const void *obs, const void *dirs,
                          const void *actions, int64_t num_envs, bool *nothing)
{
    if (int rc = snake_policy_plan(cfg)) return rc;
    if (!obs || !dirs || !actions) { set_error("%s: NULL buffer", fn); return SNAKE_E_ARG; }
    if ((uintptr_t)obs & 15) { set_error("%s: obs must be 16-byte aligned", fn); return SNAKE_E_ARG; }
    if (num_envs < 0 || num_envs > (1ll << 26)) {
        set_error("%s: num_envs must be in [0, 2^26] (got %lld)", fn, (long long)num_envs);
        return SNAKE_E_ARG;
    }
    *nothing = num_envs == 0;
    return SNAKE_OK;
}

}  // namespace snake
