// dqn_bf16_tile.h -- the 64 x 64 output tile on v_mfma_f32_16x16x32_bf16 that
// the learner's bf16 backward (dqn_train16_kernels.hip) and its bf16 forward
// (dqn_fwd16_kernels.hip) share: the fp32 -> bf16 conversion, the swizzled
// [64][64] bf16 LDS image, the fragment reads and MFMAs of one stage, and the
// workgroup renumbering (not part of the C-ABI).
//
// A 256-thread workgroup owns a 64 x 64 output tile, wave (w/2, w%2) a 32 x 32
// quarter (2 x 2 MFMA tiles). A stage is 64 reduction steps (two MFMA k-steps).
// Both operands are staged in LDS as [64 rows or columns of the output][64
// reduction steps] bf16: 128-byte rows of eight 16-byte slots, slot s holding
// steps 8s .. 8s+7 -- what lane group s % 4 of k-step s / 4 reads with one
// ds_read_b128. Slot s of row r is stored at slot s ^ swz(r): the 16 rows x
// {g, g+1} a ds_read_b128 lane group touches then fall into 16 distinct slots
// of the 256-byte bank row, so the fragment reads are conflict-free.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace snake {
namespace train {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kKT16 = 64;       // reduction steps per LDS stage
constexpr int kRowB = 128;      // bytes of an LDS row: kKT16 bf16

// Two floats to two bf16 in one word, lo in the low half: the conversion
// instruction of gfx950 (v_cvt_pk_bf16_f32), which is what the compiler emits
// for a float -> __bf16 conversion. Round to nearest even, the value
// dqn_kernels.hip bf16_bits computes on the bit pattern (denormals are kept);
// a NaN stays a NaN: sign and top mantissa bits kept, the quiet bit set, as in
// the pack (dqn_pack_kernels.hip bf16_rne). In software the two additions,
// shifts and the NaN test per element made the loaders longer than the MFMAs.
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack2(float lo, float hi)
{
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

// Workgroups are dealt to the eight XCDs (private L2s) round-robin by their
// linear id: neighbours in the grid, which share an operand panel (the column
// tiles of a weight gradient's chunk its dY rows, the row tiles of an input
// gradient's column tile its W columns), each fetch it into another L2. Renumber
// so that XCD j's workgroups j, j + 8, ... take consecutive tiles. A bijection
// of [0, nwg): a matter of speed only, every tile is computed once wherever it
// runs.
__device__ __forceinline__ uint32_t xcd_remap(uint32_t bid, uint32_t nwg)
{
    const uint32_t j = bid & 7, q = nwg >> 3, r = nwg & 7;
    return j * q + (j < r ? j : r) + (bid >> 3);
}

// the slot swizzle of LDS row r (see the head of the file)
__device__ __forceinline__ int swz(int r)
{
    const int u = (r >> 2) & 3, v = r & 3;
    return (((u ^ (u >> 1)) & 1) ^ (2 * u + (v >> 1)) ^ (v & 1) ^ ((r >> 4) & 1)) & 7;
}
__device__ __forceinline__ int slot_off(int r, int s) { return r * kRowB + ((s ^ swz(r)) << 4); }

// 64 reduction steps of the workgroup's LDS tiles into this wave's 2 x 2 tiles
__device__ __forceinline__ void mma64(const uint8_t *As, const uint8_t *Bs, int wr, int wc, int grp, int l16,
                                      f32x4 (&acc)[2][2])
{
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
        bf16x8 a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            a[i] = *reinterpret_cast<const bf16x8 *>(As + slot_off(wr * 32 + i * 16 + l16, 4 * ks + grp));
            b[i] = *reinterpret_cast<const bf16x8 *>(Bs + slot_off(wc * 32 + i * 16 + l16, 4 * ks + grp));
        }
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int c = 0; c < 2; c++)
                acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[c], acc[i][c], 0, 0, 0);
    }
}

}  // namespace train
}  // namespace snake
