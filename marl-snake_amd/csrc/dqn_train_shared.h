// dqn_train_shared.h -- what the learner's fp32 backward (dqn_train_kernels.hip)
// and its bf16 form (dqn_train16_kernels.hip) share: the split-M rule, the two
// GEMM argument blocks, the train scratch and the host-side launch helpers (not
// part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "dqn32_shared.h"

namespace snake {
namespace train {

constexpr int kT = 64;          // output tile: kT rows x kT columns
constexpr int64_t kChunk = 2048;
constexpr int64_t kMaxChunks = 128;

__host__ __device__ inline int64_t chunk_rows(int64_t M)
{
    int64_t c = (M + kMaxChunks - 1) / kMaxChunks;
    c = (c + 15) / 16 * 16;
    return c > kChunk ? c : kChunk;
}
inline int64_t num_chunks(int64_t M) { return M < 1 ? 1 : (M + chunk_rows(M) - 1) / chunk_rows(M); }

// ---- weight gradient: out[chunk][n][k] = sum_{m in chunk} dY[m][n] * act(X)[m][k]
struct WgradArgs {
    const float *dy;        // [M][N], N % 4 == 0
    const void *x;          // the forward's A source (mode)
    const float *xbias;     // its bias (modes 1, 2)
    int bmod;               // bias period along k (mode 2)
    const int *scale_flag;  // mode 0: nonzero -> uint8 / 255
    int N, K;               // K % 4 == 0
    int H, W, C;            // conv geometry (modes 0, 1)
    int64_t M, chunk;
    float *out;             // [chunks][N][K]
    float *bout;            // [chunks][N]: the bias gradient's partials, the column sums of dY
};

// ---- input gradient: out[m][k] = (sum_r A(m, r) * B(r, k)) * (yprev[m][k] + pbias > 0)
//   dense: r = n;         A = dY[m][n],                     B = W[n][k]
//   conv:  r = (tap, co); A = dY[(b, y+1-dy, x+1-dx)][co],  B = W[co][tap*K + k]   (K = Cin)
struct DgradArgs {
    const float *dy;
    const float *w;
    const float *yprev;     // [M][K] pre-activations of the layer below
    const float *pbias;     // their bias, period bmod along k
    int bmod;
    float *out;             // [M][K]
    int64_t M;
    int R;                  // reduction length (dense: N; conv: 9 * Cout), R % 4 == 0
    int K;                  // K % 4 == 0
    int H, W, Cout;         // conv
};

// train scratch (floats): dY5 [B][128] | dY4 [B][256] | dY3 [BP][64] | dY2 [BP][64]
// | dY1 [BP][32] | weight partials | bias partials
struct TrainScratch {
    float *dy5, *dy4, *dy3, *dy2, *dy1, *wpart, *bpart;
};

// dqn_train_kernels.hip
int reduce(const float *wpart, const float *bpart, int64_t chunks, int64_t nw, int64_t nb, float *wout, float *bout,
           hipStream_t s, const char *what);

// dqn_train16_kernels.hip: the bf16 forms of wgrad<MODE> and dgrad<CONV>
int wgrad16(int mode, WgradArgs g, float *grad_w, float *grad_b, const TrainScratch &ts, hipStream_t s,
            const char *what);
int dgrad16(bool conv, const DgradArgs &g, hipStream_t s, const char *what);

}  // namespace train
}  // namespace snake
