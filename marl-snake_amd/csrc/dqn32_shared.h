// dqn32_shared.h -- what the fp32 forward (dqn32_kernels.hip) and the learner
// (dqn_train_kernels.hip) share: the GEMM argument block and its operand modes,
// the configuration check, the forward's scratch layout and the LDS patch sizes,
// and the bf16 forward's (dqn_fwd16_kernels.hip) split-K rule, scratch and
// launch helper (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "snake_internal.h"
#include "snake_device.h"

namespace snake {
namespace dqn32 {

enum { kConvU8 = 0, kConvF32 = 1, kDense = 2 };
struct GemmArgs {
    const void *x;          // A source (see mode)
    const float *xbias;     // bias applied (with ReLU) to the A source (modes 1, 2)
    int bmod;               // bias period along k (mode 2)
    const float *w;         // [N][K]
    float *y;               // [M][N]
    const float *ybias;     // added to the output (the last layer) or NULL
    int64_t M;
    int N, K;
    int H, W, C;            // conv geometry (modes 0, 1): map H x W, input channels C
    const int *scale_flag;  // mode 0: nonzero -> divide the uint8 input by 255
};

constexpr int kConvRows = 128;
constexpr int kPatchMaxBytes = 80 * 1024;   // two workgroups per CU

__host__ __device__ inline int conv_patch_rows(int H, int W)
{
    // tall rows spanned by 128 consecutive positions + the two halo rows
    const int P = H * W;
    return (kConvRows - 1 + W - 1) / W + 1 + (kConvRows - 1 + P - 1) / P + 2;
}

// Cell stride in floats: C + 8 when C % 16 == 0, else C (C % 8 == 0), so that the
// stride in 16-byte slots is 2 mod 4. ds_read_b128 serves a wave in four lane
// groups of 16 ({0-3,12-15,20-27}, {4-11,16-19,28-31}, and the upper half
// alike: MI355X_MICROARCH.md §LDS); a group holds 8 rows of lane group g and
// 8 of g+1, distinct mod 8, so their slots 2m*row + g are all distinct (a
// stride of 1 mod 4 made every group 2-way).
__host__ __device__ inline int conv_cell_stride(int C) { return C + ((C & 15) ? 0 : 8); }

__host__ inline int64_t conv_patch_bytes(int H, int W, int C)
{
    return (int64_t)conv_patch_rows(H, W) * (W + 2) * conv_cell_stride(C) * 4;
}

inline int check_cfg(const snake_dqn_cfg *cfg)
{
    if (!cfg) { set_error("snake_dqn32: NULL cfg"); return SNAKE_E_ARG; }
    if (cfg->height < 1 || cfg->width < 1 || cfg->height > 255 || cfg->width > 255) {
        set_error("snake_dqn32: observation %dx%d out of range", cfg->height, cfg->width);
        return SNAKE_E_CONFIG;
    }
    if (cfg->channels < 8 || cfg->channels % 8 || cfg->channels > 128) {
        set_error("snake_dqn32: channels must be a multiple of 8 in [8, 128] (got %d)", cfg->channels);
        return SNAKE_E_CONFIG;
    }
    if (cfg->num_actions < 1 || cfg->num_actions > 64) {
        set_error("snake_dqn32: num_actions must be in [1, 64] (got %d)", cfg->num_actions);
        return SNAKE_E_CONFIG;
    }
    return SNAKE_OK;
}

// scratch layout (bytes): flag (16) | Y1 | Y2 | Y3 | Y4 | Y5
struct Scratch {
    int *flag;
    float *y1, *y2, *y3, *y4, *y5;
};

inline int64_t scratch_bytes(const snake_dqn_cfg *cfg, int64_t B, void *base, Scratch *out)
{
    const int64_t P = (int64_t)cfg->height * cfg->width;
    const int64_t n1 = B * P * 32, n2 = B * P * 64, n3 = n2, n4 = B * 256, n5 = B * 128;
    if (out) {
        uint8_t *p = reinterpret_cast<uint8_t *>(base);
        out->flag = reinterpret_cast<int *>(p);
        out->y1 = reinterpret_cast<float *>(p + 16);
        out->y2 = out->y1 + n1;
        out->y3 = out->y2 + n2;
        out->y4 = out->y3 + n3;
        out->y5 = out->y4 + n4;
    }
    return 16 + 4 * (n1 + n2 + n3 + n4 + n5);
}

// ---- the bf16 mixed-precision forward (dqn_fwd16_kernels.hip)
// Split K of its dense layers: the K reduction steps are cut into chunks of
// max(1024, ceil(K / 16) rounded up to 64) steps -- at most 16 chunks, a rule of
// K alone, so a row's sums do not depend on the batch it is in.
constexpr int kSplitMinK = 1024, kSplitMaxChunks = 16;
__host__ __device__ inline int split_k_chunk(int K)
{
    const int c = ((K + kSplitMaxChunks - 1) / kSplitMaxChunks + 63) / 64 * 64;
    return c > kSplitMinK ? c : kSplitMinK;
}
inline int split_k_chunks(int K) { return K < 1 ? 1 : (K + split_k_chunk(K) - 1) / split_k_chunk(K); }

// its scratch: dqn32::Scratch's layout, then fc1's split-K partials [chunks][B][256]
// (none with one chunk; fc2's K = 256 is one chunk)
inline int64_t fwd16_scratch_bytes(const snake_dqn_cfg *cfg, int64_t B, void *base, Scratch *out, float **partials)
{
    const int64_t head = scratch_bytes(cfg, B, base, out);
    const int chunks = split_k_chunks(cfg->height * cfg->width * 64);
    if (partials) *partials = reinterpret_cast<float *>(reinterpret_cast<uint8_t *>(base) + head);
    return head + (chunks > 1 ? 4 * (int64_t)chunks * B * 256 : 0);
}

// Y = bf16(act(X)) bf16(W)^T of one layer (mode: kConvU8, kConvF32 or kDense; ybias unused);
// partials: room for the dense layers' split-K partials [chunks][M][N]
int gemm16(int mode, const GemmArgs &g, float *partials, hipStream_t s, const char *what);

}  // namespace dqn32
}  // namespace snake
