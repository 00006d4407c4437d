// dqn_fwd16_kernels.hip -- the learner's forward in bf16 mixed precision
// (snake_dqn32_forward_bf16; the entry point and its launch sequence are in
// dqn32_kernels.hip beside the fp32 forward's). conv1, conv2, conv3, fc1 and fc2
// are one GEMM kernel
//
//   Y[m][n] = sum_k bf16(act(X)[m][k]) * bf16(W[n][k])          (W row-major [N][K])
//
// on v_mfma_f32_16x16x32_bf16 with fp32 accumulators, over the fp32 forward's
// three operand modes (dqn32_shared.h): act(X) is formed in fp32 exactly as
// there -- the byte, or byte / 255 when the flag is set; relu(Y_prev + b_prev),
// zero off the map -- and rounded when it is staged; W is the fp32 master,
// rounded when it is staged; Y is stored as the fp32 sum.
//
// The tile, the LDS image and the MFMA sequence are dqn_bf16_tile.h's (the bf16
// backward's). Both operands are reduction-contiguous in memory: W is [N][K],
// and eight consecutive k of an im2col row lie inside one tap's channels
// because C % 8 == 0. So thread (row t / 4, part t % 4) of the 256 loads
// reduction steps 16 part .. 16 part + 15 of its row of each operand (slots
// 2 part and 2 part + 1) with 16-byte loads, converts and stores two
// ds_write_b128 per operand: no transposed stores, no LDS patch, hence no limit
// on the map's width. The conv rows are gathered per stage: tap (dy, dx) of
// output cell m is cell m + (dy-1) W + (dx-1) where that is on the map, else
// zeros. A stage's loads are issued together, unconditionally (a masked load's
// address falls back to the operand's first bytes), and nothing is done to
// their results until the previous stage's MFMAs are issued; act(X), the mask
// and the conversion happen when the stage is stored to LDS.
//
// Tails are zero-filled: rows past M, columns past N (conv1 has 32: the waves of
// the empty half skip their MFMAs), reduction steps past the chunk's end
// (K = 9 C is no multiple of 64 for C = 8 or 32).
//
// Split K (dense layers): grid.z chunks of split_k_chunk(K) steps; with more
// than one, chunk z writes the partial [z][M][N] and train::reduce adds the
// partials in chunk order. The rule depends on K alone and a row's MFMA
// sequence on its chunk alone, so a row's bits do not depend on its batch.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "dqn_bf16_tile.h"
#include "dqn_train_shared.h"

namespace snake {
namespace dqn32 {

using train::f32x4;
using train::kKT16;
using train::kRowB;
using train::kT;
using train::u32x4;

template <int MODE>
__global__ void __launch_bounds__(256, 4) k_fwd16(const GemmArgs g, const int chunk_k, float *const partials)
{
    __shared__ __attribute__((aligned(16))) uint8_t As[kT * kRowB];
    __shared__ __attribute__((aligned(16))) uint8_t Bs[kT * kRowB];
    __shared__ __attribute__((aligned(16))) float bias[256];    // the A source's bias (C <= 64, bmod <= 256)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, grp = lane >> 4, l16 = lane & 15;
    // the tile: (column tile, row tile, chunk), column tile fastest: the column tiles of a row tile
    // re-read its activation rows, the row tiles of a chunk its W panel
    const uint32_t nrt = gridDim.x, nct = gridDim.y;
    const uint32_t tile = train::xcd_remap(blockIdx.x + nrt * (blockIdx.y + nct * blockIdx.z), nrt * nct * gridDim.z);
    const uint32_t ct = tile % nct, rt = tile / nct % nrt, bz = tile / (nct * nrt);
    const int64_t m0 = (int64_t)rt * kT;
    const int n0 = ct * kT;
    const int kbeg = bz * chunk_k;
    const int kend = kbeg + chunk_k < g.K ? kbeg + chunk_k : g.K;
    // loaders: row arow of each operand, reduction steps 16 part .. 16 part + 15 of the stage
    const int arow = tid >> 2, part = tid & 3;
    const int64_t m = m0 + arow;
    const int n = n0 + arow;
    const bool a_ok = m < g.M, b_ok = n < g.N;
    if constexpr (MODE != kConvU8) {
        const int nbias = MODE == kDense ? g.bmod : g.C;
        if (tid < nbias) bias[tid] = g.xbias[tid];
    }
    float scale255 = 0.f;
    if constexpr (MODE == kConvU8) scale255 = *g.scale_flag ? 1.f : 0.f;
    // the A row: its bytes at tap (1, 1), channel 0 (conv) or at k = 0 (dense)
    constexpr int kElt = MODE == kConvU8 ? 1 : 4;
    const uint8_t *const xbase = reinterpret_cast<const uint8_t *>(g.x);
    const uint8_t *arowp = xbase;
    int y = 0, x = 0;
    int tap[2] = {0, 0}, ci[2] = {0, 0};        // of this thread's two slots at the next fetch
    if constexpr (MODE == kDense) {
        if (a_ok) arowp = xbase + m * g.K * 4;
    } else {
        const int P = g.H * g.W;
        const int64_t bimg = a_ok ? m / P : 0;
        const int p = (int)(a_ok ? m - bimg * P : 0);
        y = p / g.W;
        x = p - y * g.W;
        if (a_ok) arowp = xbase + m * g.C * kElt;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int k = kbeg + 16 * part + 8 * h;
            tap[h] = k / g.C;
            ci[h] = k - tap[h] * g.C;
        }
    }
    const float *const wrowp = g.w + (b_ok ? (int64_t)n * g.K : 0);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    // fetch() only issues the loads; stage() forms act(X), converts and stores
    f32x4 ra[4], rw[4];         // slot h: [2h], [2h+1]
    uint32_t raw8[4];           // kConvU8: slot h's eight bytes in [2h], [2h+1]
    bool a_live[2], w_live[2];
    int boff[2];                // the bias offset of slot h's first step
    auto fetch = [&](int k0) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int k = k0 + 16 * part + 8 * h;
            const bool k_ok = k < kend;
            w_live[h] = b_ok && k_ok;
            const float *wp = wrowp + (w_live[h] ? k : 0);
            rw[2 * h] = *reinterpret_cast<const f32x4 *>(wp);
            rw[2 * h + 1] = *reinterpret_cast<const f32x4 *>(wp + 4);
            const uint8_t *src = xbase;
            if constexpr (MODE == kDense) {
                a_live[h] = a_ok && k_ok;
                if (a_live[h]) src = arowp + (int64_t)k * 4;
                boff[h] = k & (g.bmod - 1);
            } else {
                const int t = tap[h];
                const int dy = (t * 11) >> 5, dx = t - 3 * dy;      // t / 3, t % 3 for t < 9 (k < K)
                const int yy = y + dy - 1, xx = x + dx - 1;
                a_live[h] = a_ok && k_ok && yy >= 0 && yy < g.H && xx >= 0 && xx < g.W;     // else zero padding
                if (a_live[h]) src = arowp + (int64_t)(((dy - 1) * g.W + (dx - 1)) * g.C + ci[h]) * kElt;
                boff[h] = ci[h];
                ci[h] += kKT16;
                while (ci[h] >= g.C) {
                    ci[h] -= g.C;
                    tap[h]++;
                }
            }
            if constexpr (MODE == kConvU8) {
                raw8[2 * h] = *reinterpret_cast<const uint32_t *>(src);
                raw8[2 * h + 1] = *reinterpret_cast<const uint32_t *>(src + 4);
            } else {
                ra[2 * h] = *reinterpret_cast<const f32x4 *>(src);
                ra[2 * h + 1] = *reinterpret_cast<const f32x4 *>(src + 16);
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            f32x4 lo, hi;
            if constexpr (MODE == kConvU8) {
                const uint32_t u = a_live[h] ? raw8[2 * h] : 0u, v = a_live[h] ? raw8[2 * h + 1] : 0u;
                lo = (f32x4){(float)(u & 255u), (float)((u >> 8) & 255u), (float)((u >> 16) & 255u), (float)(u >> 24)};
                hi = (f32x4){(float)(v & 255u), (float)((v >> 8) & 255u), (float)((v >> 16) & 255u), (float)(v >> 24)};
                if (scale255 != 0.f) {
#pragma unroll
                    for (int i = 0; i < 4; i++) {       // (the reference divides)
                        lo[i] = lo[i] / 255.0f;
                        hi[i] = hi[i] / 255.0f;
                    }
                }
            } else {
                const f32x4 b0 = *reinterpret_cast<const f32x4 *>(&bias[boff[h]]);
                const f32x4 b1 = *reinterpret_cast<const f32x4 *>(&bias[boff[h] + 4]);
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const float u = ra[2 * h][i] + b0[i], v = ra[2 * h + 1][i] + b1[i];
                    lo[i] = a_live[h] && u > 0.f ? u : 0.f;
                    hi[i] = a_live[h] && v > 0.f ? v : 0.f;
                }
            }
            const u32x4 a = {train::pack2(lo[0], lo[1]), train::pack2(lo[2], lo[3]), train::pack2(hi[0], hi[1]),
                             train::pack2(hi[2], hi[3])};
            *reinterpret_cast<u32x4 *>(As + train::slot_off(arow, 2 * part + h)) = a;
            const f32x4 w0 = w_live[h] ? rw[2 * h] : zero, w1 = w_live[h] ? rw[2 * h + 1] : zero;
            const u32x4 w = {train::pack2(w0[0], w0[1]), train::pack2(w0[2], w0[3]), train::pack2(w1[0], w1[1]),
                             train::pack2(w1[2], w1[3])};
            *reinterpret_cast<u32x4 *>(Bs + train::slot_off(arow, 2 * part + h)) = w;
        }
    };
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int c = 0; c < 2; c++) acc[i][c] = zero;
    const bool wave_live = n0 + wc * 32 < g.N;      // (conv1: the upper 32 columns do not exist)
    fetch(kbeg);
    __syncthreads();        // bias
    stage();
    __syncthreads();
    for (int k0 = kbeg; k0 < kend; k0 += kKT16) {
        const bool more = k0 + kKT16 < kend;
        if (more) fetch(k0 + kKT16);
        if (wave_live) train::mma64(As, Bs, wr, wc, grp, l16, acc);
        __syncthreads();
        if (more) {
            stage();
            __syncthreads();
        }
    }
    float *out = partials ? partials + (int64_t)bz * g.M * g.N : g.y;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const int nc = n0 + wc * 32 + c * 16 + l16;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int64_t mr = m0 + wr * 32 + i * 16 + 4 * grp + r;
                if (mr < g.M && nc < g.N) out[mr * g.N + nc] = acc[i][c][r];
            }
        }
}

int gemm16(int mode, const GemmArgs &g, float *partials, hipStream_t s, const char *what)
{
    const int chunk = mode == kDense ? split_k_chunk(g.K) : (g.K + kKT16 - 1) / kKT16 * kKT16;
    const int chunks = mode == kDense ? split_k_chunks(g.K) : 1;
    float *part = chunks > 1 ? partials : nullptr;
    const dim3 grid((unsigned)((g.M + kT - 1) / kT), (unsigned)((g.N + kT - 1) / kT), (unsigned)chunks);
    if (mode == kDense)
        hipLaunchKernelGGL(k_fwd16<kDense>, grid, dim3(256), 0, s, g, chunk, part);
    else if (mode == kConvF32)
        hipLaunchKernelGGL(k_fwd16<kConvF32>, grid, dim3(256), 0, s, g, chunk, part);
    else
        hipLaunchKernelGGL(k_fwd16<kConvU8>, grid, dim3(256), 0, s, g, chunk, part);
    int rc = launch_status(what);
    if (!rc && chunks > 1) rc = train::reduce(part, part, chunks, g.M * g.N, 0, g.y, g.y, s, what);
    return rc;
}

}  // namespace dqn32
}  // namespace snake
