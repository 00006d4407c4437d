// step_lanes.h -- the lane-level helpers of the step kernels: link-table
// access, wave and DPP lane-group exchanges (gsel, gscan), small arithmetic,
// wave-mask counts, and the write-through (sc1) loads and stores.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <type_traits>
#include <utility>

#include "snake_internal.h"
#include "step_args.h"

namespace snake {

// Link-table access: LDS atomics are ds_min_u32, global ones L2 atomics; global
// reads bypass the vector L1 (a previous attempt's chase may have cached lines).
__device__ __forceinline__ void link_min(lu32 *p, uint32_t v)
{
    __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void link_min(gu32 *p, uint32_t v)
{
    __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t link_get(const lu32 *p) { return *p; }
__device__ __forceinline__ uint32_t link_get(const gu32 *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A worker's global link table between its writers and its readers, all lanes
// of one wave: the wave's stores and atomics complete at device scope, then a
// wave barrier.
__device__ __forceinline__ void link_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    __builtin_amdgcn_wave_barrier();
}

// Direction (core/snake.py:33-37): 0 UP(-1,0) 1 RIGHT(0,1) 2 DOWN(1,0) 3 LEFT(0,-1)
__device__ __forceinline__ int dir_dr(int d) { return d == 0 ? -1 : (d == 2 ? 1 : 0); }
__device__ __forceinline__ int dir_dc(int d) { return d == 1 ? 1 : (d == 3 ? -1 : 0); }
__device__ __forceinline__ int div10(int v) { return (v * 205) >> 11; }  // exact for 0 <= v < 1029
// x / d by the multiply-high reciprocal m = ceil(2^32 / d) (snake_capi.cpp);
// d == 1 has no 32-bit reciprocal (m wraps to 0)
__device__ __forceinline__ int fdiv(uint32_t x, uint32_t m, int d) { return d == 1 ? (int)x : (int)__umulhi(x, m); }

// LDS hand-off between lanes of the single wave of a workgroup: LDS executes a
// wave's instructions in order, so only the compiler must not move memory
// operations across this point.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int wave_scan(int v, int lane)
{
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int n = __shfl_up(v, o);
        if (lane >= o) v += n;
    }
    return v;
}

__device__ __forceinline__ int bcast(int v, int k) { return __builtin_amdgcn_readlane(v, k); }

// ---- exchanges inside k_logic's env groups of G = 4, 8 or 16 lanes (aligned
// inside a 16-lane DPP row) by DPP moves, not through the LDS: a __shfl
// (ds_bpermute) is an LDS round trip on the rules' dependency chain.
// A DPP move reads its source lane's register only when that lane is active:
// every move here runs with the whole wave active, and its result passes
// through an empty volatile asm, so the compiler cannot sink it into a branch
// that only some lanes take (it did: a select on a DPP result became an
// exec-masked branch around the move, which then read disabled lanes).
__device__ __forceinline__ int dpp_pin(int x)
{
    __asm__ volatile("" : "+v"(x));
    return x;
}

// gsel<G, J>(v): the value of lane J of this lane's group.
template <int G, int J>
__device__ __forceinline__ int gsel(int v)
{
    static_assert(G == 4 || G == 8 || G == 16, "group of 4, 8 or 16 lanes");
    if constexpr (G == 4) {
        return dpp_pin(__builtin_amdgcn_mov_dpp(v, J * 0x55, 0xf, 0xf, false));   // quad_perm:[J,J,J,J]
    } else if constexpr (G == 16) {
        return dpp_pin(__builtin_amdgcn_mov_dpp(v, 0x150 + J, 0xf, 0xf, false));   // row_newbcast:J
    } else {
        // lane J & 3 of the lane's quad; then the group's other quad (DPP banks
        // 1, 3 for J < 4, else 0, 2) takes that value from four lanes over,
        // the bank mask keeping the rest
        const int t = dpp_pin(__builtin_amdgcn_mov_dpp(v, (J & 3) * 0x55, 0xf, 0xf, false));
        if constexpr (J < 4) return dpp_pin(__builtin_amdgcn_update_dpp(t, t, 0x114, 0xf, 0xa, false));   // row_shr:4
        else return dpp_pin(__builtin_amdgcn_update_dpp(t, t, 0x104, 0xf, 0x5, false));                   // row_shl:4
    }
}

template <int G, int J>
__device__ __forceinline__ double gsel(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = gsel<G, J>((int)b), hi = gsel<G, J>((int)(b >> 32));
    return __longlong_as_double(((long long)hi << 32) | (uint32_t)lo);
}

// inclusive prefix sum over the group (k = the lane's index in it)
template <int G>
__device__ __forceinline__ int gscan(int v, int k)
{
    int x = dpp_pin(__builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v += k >= 1 ? x : 0;
    x = dpp_pin(__builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false));       // row_shr:2
    v += k >= 2 ? x : 0;
    if constexpr (G >= 8) {
        x = dpp_pin(__builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false));
        v += k >= 4 ? x : 0;
    }
    if constexpr (G >= 16) {
        x = dpp_pin(__builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false));
        v += k >= 8 ? x : 0;
    }
    return v;
}

// f(integral_constant<int, J>) for J = 0 .. N-1, unrolled at compile time
template <typename F, int... I>
__device__ __forceinline__ void unroll_seq(F &&f, std::integer_sequence<int, I...>)
{
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void unroll(F &&f)
{
    unroll_seq(f, std::make_integer_sequence<int, N>{});
}

// number of zero bytes of x (exact: no borrow between bytes)
__device__ __forceinline__ int zero_bytes(uint32_t x)
{
    const uint32_t t = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
    return __popc(t);
}

// set bits of x below this lane, + add
__device__ __forceinline__ int mbcnt64(unsigned long long x, int add = 0)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(x >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)x, (uint32_t)add));
}

// this lane's bit of a wave mask, as a lane predicate (v_cndmask on the SGPR pair)
__device__ __forceinline__ bool inv_ballot(unsigned long long m) { return __builtin_amdgcn_inverse_ballot_w64(m); }

// population count of a wave mask on the vector ALU (`ones` is an opaque
// all-ones VGPR): the scalar count of a mask a vector compare just wrote costs a
// vector-to-scalar hand-off and a move back in the round's dependency chain
__device__ __forceinline__ int vpopc(unsigned long long x, uint32_t ones)
{
    return __builtin_popcount((uint32_t)x & ones) + __builtin_popcount((uint32_t)(x >> 32) & ones);
}

// Hand-off of a record between concurrently running kernels (background
// spawn-ahead): write-through (sc1) stores, drained, then the status word's
// compare-and-swap; the reader takes the word with an atomic and loads the
// record with sc1 loads (MI355X_MICROARCH.md, inter-workgroup visibility).
__device__ __forceinline__ uint32_t ld_sc1(const uint32_t *p)
{
    return __hip_atomic_load((const gu32 *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1(uint32_t *p, uint32_t v)
{
    __hip_atomic_store((gu32 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// 8-byte forms (global address space: never flat), and 16 bytes as two of them
typedef __attribute__((address_space(1))) unsigned long long gu64;
__device__ __forceinline__ unsigned long long ld_sc1_64(const void *p)
{
    return __hip_atomic_load((const gu64 *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1_64(void *p, unsigned long long v)
{
    __hip_atomic_store((gu64 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1_128(void *p, uint4 v)
{
    st_sc1_64(p, (unsigned long long)v.x | ((unsigned long long)v.y << 32));
    st_sc1_64((uint8_t *)p + 8, (unsigned long long)v.z | ((unsigned long long)v.w << 32));
}
__device__ __forceinline__ uint4 ld_sc1_128(const void *p)
{
    const unsigned long long a = ld_sc1_64(p), b = ld_sc1_64((const uint8_t *)p + 8);
    return make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
}

}  // namespace snake
