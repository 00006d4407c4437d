// step_args.h -- how the step and reset kernels of snake_kernels.hip take their
// arguments (KArgs, kargs), the grid cell codes and the address-space views.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "snake_internal.h"

namespace snake {

enum { C_EMPTY = 0, C_WALL = 1, C_FRUIT = 2, C_HEAD = 3, C_BODY = 4, C_TAIL = 5 };

// The step and reset kernels take their arguments as one struct and read them
// through kargs(kp): the kernarg-segment pointer passed through an empty asm
// that the compiler cannot see through, afresh at each phase or job. Every field
// is then an s_load next to its use (the segment is constant, scalar-cached)
// instead of a value held in an SGPR from the kernel's entry to its end: with
// the whole KCfg, snake_state and snake_out live across a worker's job loop the
// compiler spilled 230-300 SGPRs into VGPR lanes, 1 100-1 700 v_readlane reloads
// and 128 VGPRs (profiles/r03_isa_counts.jsonl).
// The kernel takes the pointer as its first statement (kernel_args(): only
// there does the builtin mean the running kernel's segment) and hands it down
// as an argument, so a device function is right whether or not it is inlined;
// __forceinline__ is for speed only. (encode_tbl_block<8, 64, *> is out of line
// in the product build; it takes c, st, o by reference, which is as safe.)
struct KArgs {
    KCfg c;
    snake_state st;
    snake_out o;
    const void *aux;   // k_logic: the actions; k_reset: the env mask
};

typedef const __attribute__((address_space(4))) KArgs *KPtr;

// only as the first statement of a __global__ kernel (tests/test_capi.py)
__device__ __forceinline__ KPtr kernel_args()
{
    return (KPtr)__builtin_amdgcn_kernarg_segment_ptr();   // (the first explicit argument is at offset 0)
}

__device__ __forceinline__ const KArgs &kargs(KPtr p)
{
    __asm__ volatile("" : "+s"(p));
    return *(const KArgs *)p;
}

// global-memory views (explicit address space: flat accesses would also count
// against lgkmcnt and stall every LDS/cross-lane wait behind them)
typedef __attribute__((address_space(3))) uint16_t lu16;
typedef __attribute__((address_space(1))) uint32_t gu32;
typedef __attribute__((address_space(3))) uint32_t lu32;
typedef uint32_t v4u32 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) v4u32 gu4;
typedef __attribute__((address_space(3))) v4u32 lu4;
constexpr uint32_t kNoLink = 0xffffffffu;

}  // namespace snake
