// dqn_train16_kernels.hip -- the bf16 form of the learner's two matrix-core
// kernels (dqn_train_kernels.hip k_wgrad<MODE>, k_dgrad<CONV>): the same
// operands from the same fp32 sources, every GEMM operand element rounded to
// bf16 when it is staged, products and sums on v_mfma_f32_16x16x32_bf16 with
// fp32 accumulators. What stays fp32: act(X) is formed in fp32 and rounded
// afterwards, the ReLU mask Y + bias > 0, the stored dX (unrounded: the next
// GEMM rounds it when it stages it), and the bias gradient, the column sums of
// the unrounded dY. fc3, k_reduce, the split-M rule and the train scratch are
// dqn_train_kernels.hip's.
//
// A 256-thread workgroup owns a 64 x 64 output tile, wave (w/2, w%2) a 32 x 32
// quarter (2 x 2 MFMA tiles), as in the fp32 kernels. A stage is 64 reduction
// steps (two MFMA k-steps). Both operands are staged in LDS as [64 rows or
// columns of the output][64 reduction steps] bf16: 128-byte rows of eight
// 16-byte slots, slot s holding steps 8s .. 8s+7 -- what lane group s % 4 of
// k-step s / 4 reads with one ds_read_b128. Slot s of row r is stored at slot
// s ^ swz(r): the 16 rows x {g, g+1} a ds_read_b128 lane group touches then
// fall into 16 distinct slots of the 256-byte bank row, so the fragment reads
// are conflict-free. The reduction-major sources (dY and act(X) of the weight
// gradient, W of the input gradient) are transposed on the way in: a thread
// loads four consecutive reduction steps of four consecutive rows, packs each
// row's four values and stores 8 bytes (ds_write_b64: 2-way, the best a
// 128-byte row allows); the input gradient's A operand is reduction-contiguous
// and goes in as two conflict-free ds_write_b128.
//
// A stage's global loads are issued together and nothing is done to their
// results until the previous stage's MFMAs are issued: the activation, the bias
// sums and the conversion happen when the stage is stored to LDS. Workgroups are
// renumbered so that tiles sharing an operand panel run on one XCD (xcd_remap).
//
// Bias gradient: in the workgroups of column tile 0 every loader thread adds
// its four dY columns, unrounded, as it stages them (stages in order, the four
// steps in order); the 16 loader threads of a column are added in order through
// LDS at the end. A fixed order that depends on the shape alone.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "dqn_bf16_tile.h"
#include "dqn_train_shared.h"

namespace snake {
namespace train {

using dqn32::kConvF32;
using dqn32::kConvU8;
using dqn32::kDense;

// (pack2, xcd_remap, swz, slot_off and mma64: dqn_bf16_tile.h, shared with the bf16 forward)

// p / w for 0 <= p < 2^16 and 1 <= w <= 255 with a quotient below 256: the
// product's error is below 2^-13, the distance of (p + 0.5) / w to an integer at
// least 0.5 / 255
__device__ __forceinline__ int div_small(int p, float rcp_w) { return (int)(((float)p + 0.5f) * rcp_w); }

// reduction steps 4kk .. 4kk+3 (v[0..3]) of rows q4 .. q4+3 (the vector's elements), transposed into the image
__device__ __forceinline__ void stage_transposed(uint8_t *S, int kk, int q4, const f32x4 (&v)[4])
{
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const u32x2 w = {pack2(v[0][i], v[1][i]), pack2(v[2][i], v[3][i])};
        *reinterpret_cast<u32x2 *>(S + slot_off(q4 + i, kk >> 1) + (kk & 1) * 8) = w;
    }
}

// ---- weight gradient (WgradArgs): out[chunk][n][k] = sum_{m in chunk} bf16(dY[m][n]) * bf16(act(X)[m][k])
template <int MODE>
__global__ void __launch_bounds__(256, 4) k_wgrad16(const WgradArgs g)
{
    __shared__ __attribute__((aligned(16))) uint8_t As[kT * kRowB];
    __shared__ __attribute__((aligned(16))) uint8_t Bs[kT * kRowB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, grp = lane >> 4, l16 = lane & 15;
    // the tile: (column tile bx, row tile by, chunk bz), bx fastest
    const uint32_t tile = xcd_remap(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z),
                                    gridDim.x * gridDim.y * gridDim.z);
    const uint32_t bx = tile % gridDim.x, by = tile / gridDim.x % gridDim.y, bz = tile / (gridDim.x * gridDim.y);
    const int k0 = bx * kT, n0 = by * kT;
    const int64_t mbeg = (int64_t)bz * g.chunk;
    const int64_t mend = mbeg + g.chunk < g.M ? mbeg + g.chunk : g.M;
    // loaders: reduction steps 4kk .. 4kk+3, four consecutive rows (n) / columns (k)
    const int kk = tid >> 4, q4 = (tid & 15) * 4;
    const int n = n0 + q4, k = k0 + q4;
    const bool a_ok = n < g.N, b_ok = k < g.K;
    int dy = 0, dx = 0, ci = 0;
    const uint32_t P = (uint32_t)(g.H * g.W);
    if constexpr (MODE != kDense) {
        const int tap = b_ok ? k / g.C : 0;
        ci = b_ok ? k - tap * g.C : 0;
        dy = tap / 3;
        dx = tap - 3 * dy;
    }
    float scale255 = 0.f;
    if constexpr (MODE == kConvU8) scale255 = *g.scale_flag ? 1.f : 0.f;
    float bias[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (MODE == kConvF32) {
#pragma unroll
        for (int i = 0; i < 4; i++) bias[i] = b_ok ? g.xbias[ci + i] : 0.f;
    }
    if constexpr (MODE == kDense) {
#pragma unroll
        for (int i = 0; i < 4; i++) bias[i] = b_ok ? g.xbias[(k + i) & (g.bmod - 1)] : 0.f;
    }
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const bool bias_owner = bx == 0;
    f32x4 bsum = zero;
    f32x4 ra[4], rb[4];
    // the loaders' sources at row mfirst = mt + 4kk, advanced by a stage per fetch. Conv: the patch
    // cell of (row m, tap) is cell m + (dy-1) W + (dx-1) where it is on the map; p = mfirst mod P
    int64_t mfirst = mbeg + 4 * kk;
    const float *pa = g.dy + mfirst * g.N + n;
    const uint8_t *px = reinterpret_cast<const uint8_t *>(g.x);
    int p = 0, pstep = 0;
    float rcp_w = 0.f;
    if constexpr (MODE == kDense) {
        px += (mfirst * g.K + k) * 4;
    } else {
        px += ((mfirst + (dy - 1) * g.W + (dx - 1)) * g.C + ci) * (MODE == kConvU8 ? 1 : 4);
        p = (int)((uint64_t)mfirst % P);
        pstep = kKT16 % (int)P;
        rcp_w = 1.0f / (float)g.W;
    }
    const int64_t xrow = (MODE == kDense ? (int64_t)g.K * 4 : MODE == kConvU8 ? (int64_t)g.C : (int64_t)g.C * 4);
    // fetch() only issues the loads (raw values, zeros where nothing is read), so that a stage's loads
    // are all in flight while the previous stage multiplies; stage() forms act(X) and the bias sums
    uint32_t raw8[4] = {0, 0, 0, 0};    // kConvU8: the four bytes of a row
    int valid = 0;                      // bit j: row j of rb was read
    auto fetch = [&]() {
        int y = 0, x = 0;
        if constexpr (MODE != kDense) {
            y = div_small(p, rcp_w);
            x = p - y * g.W;
        }
        valid = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool ok = mfirst + j < mend;
            ra[j] = zero;
            rb[j] = zero;
            raw8[j] = 0;
            if (ok && a_ok) ra[j] = *reinterpret_cast<const f32x4 *>(pa + (int64_t)j * g.N);
            const uint8_t *src = px + j * xrow;
            if constexpr (MODE == kDense) {
                if (ok && b_ok) {
                    rb[j] = *reinterpret_cast<const f32x4 *>(src);
                    valid |= 1 << j;
                }
            } else {
                const int yy = y + dy - 1, xx = x + dx - 1;
                if (ok && b_ok && yy >= 0 && yy < g.H && xx >= 0 && xx < g.W) {   // else zero padding
                    if constexpr (MODE == kConvU8)
                        raw8[j] = *reinterpret_cast<const uint32_t *>(src);
                    else
                        rb[j] = *reinterpret_cast<const f32x4 *>(src);
                    valid |= 1 << j;
                }
                if (++x == g.W) {
                    x = 0;
                    if (++y == g.H) y = 0;
                }
            }
        }
        mfirst += kKT16;
        pa += (int64_t)kKT16 * g.N;
        px += kKT16 * xrow;
        if constexpr (MODE != kDense) {
            p += pstep;
            if (p >= (int)P) p -= (int)P;
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (bias_owner) bsum += ra[j];
            if constexpr (MODE == kConvU8) {
                const uint32_t u = raw8[j];     // (0 where nothing was read)
                rb[j] = (f32x4){(float)(u & 255u), (float)((u >> 8) & 255u), (float)((u >> 16) & 255u),
                                (float)(u >> 24)};
                if (scale255 != 0.f) {
#pragma unroll
                    for (int i = 0; i < 4; i++) rb[j][i] = rb[j][i] / 255.0f;   // (the reference divides)
                }
            } else {
                const bool read = (valid >> j) & 1;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const float u = rb[j][i] + bias[i];
                    rb[j][i] = read && u > 0.f ? u : 0.f;
                }
            }
        }
        stage_transposed(As, kk, q4, ra);
        stage_transposed(Bs, kk, q4, rb);
    };
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int c = 0; c < 2; c++) acc[i][c] = zero;
    fetch();
    stage();
    __syncthreads();
    for (int64_t mt = mbeg; mt < mend; mt += kKT16) {
        const bool more = mt + kKT16 < mend;
        if (more) fetch();
        mma64(As, Bs, wr, wc, grp, l16, acc);
        __syncthreads();
        if (more) {
            stage();
            __syncthreads();
        }
    }
    if (bias_owner) {       // (the whole workgroup; the images are free after the loop's last barrier)
        float *bs = reinterpret_cast<float *>(As);      // [16 loader rows][64 columns]
        *reinterpret_cast<f32x4 *>(bs + kk * kT + q4) = bsum;
        __syncthreads();
        if (tid < kT && n0 + tid < g.N) {
            float t = 0.f;
#pragma unroll
            for (int r = 0; r < 16; r++) t += bs[r * kT + tid];
            g.bout[(int64_t)bz * g.N + n0 + tid] = t;
        }
    }
    float *out = g.out + (int64_t)bz * g.N * g.K;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const int kc = k0 + wc * 32 + c * 16 + l16;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int nr = n0 + wr * 32 + i * 16 + 4 * grp + r;
                if (nr < g.N && kc < g.K) out[(int64_t)nr * g.K + kc] = acc[i][c][r];
            }
        }
}

// ---- input gradient (DgradArgs): out[m][k] = (sum_r bf16(A(m, r)) * bf16(B(r, k))) * (yprev[m][k] + pbias > 0)
// conv: Cout % 16 == 0 (a loader's 16 reduction steps share a tap)
template <bool CONV>
__global__ void __launch_bounds__(256, 4) k_dgrad16(const DgradArgs g)
{
    __shared__ __attribute__((aligned(16))) uint8_t As[kT * kRowB];
    __shared__ __attribute__((aligned(16))) uint8_t Bs[kT * kRowB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, grp = lane >> 4, l16 = lane & 15;
    // the tile: (row tile, column tile), row tile fastest
    const uint32_t tile = xcd_remap(blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y);
    const int64_t m0 = (int64_t)(tile % gridDim.x) * kT;
    const int k0 = (tile / gridDim.x) * kT;
    // A loader: row arow, reduction steps 16 part .. 16 part + 15; B loader: steps 4kk .. 4kk+3, columns k .. k+3
    const int arow = tid >> 2, part = tid & 3;
    const int kk = tid >> 4, q4 = (tid & 15) * 4;
    const int64_t m = m0 + arow;
    const bool a_ok = m < g.M;
    const int k = k0 + q4;
    const bool b_ok = k < g.K;
    int64_t bimg = 0;
    int y = 0, x = 0;
    if constexpr (CONV) {
        const int P = g.H * g.W;
        bimg = a_ok ? m / P : 0;
        const int p = (int)(a_ok ? m - bimg * P : 0);
        y = p / g.W;
        x = p - y * g.W;
    }
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 ra[4], rb[4];
    auto fetch = [&](int r0) {
        const int ar = r0 + 16 * part, br = r0 + 4 * kk;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            ra[j] = zero;
            rb[j] = zero;
        }
        if constexpr (CONV) {
            if (a_ok && ar < g.R) {
                const int tap = ar / g.Cout, co = ar - tap * g.Cout;
                const int dy = tap / 3, dx = tap - 3 * dy;
                const int yy = y + 1 - dy, xx = x + 1 - dx;
                if (yy >= 0 && yy < g.H && xx >= 0 && xx < g.W) {
                    const float *src = g.dy + (m + (1 - dy) * g.W + (1 - dx)) * g.Cout + co;   // cell (bimg, yy, xx)
#pragma unroll
                    for (int j = 0; j < 4; j++) ra[j] = *reinterpret_cast<const f32x4 *>(src + 4 * j);
                }
            }
            if (b_ok && br < g.R) {
                const int tap = br / g.Cout, co = br - tap * g.Cout;
                const float *src = g.w + (int64_t)co * (9 * g.K) + tap * g.K + k;
#pragma unroll
                for (int j = 0; j < 4; j++) rb[j] = *reinterpret_cast<const f32x4 *>(src + (int64_t)j * (9 * g.K));
            }
        } else {
            if (a_ok) {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (ar + 4 * j < g.R) ra[j] = *reinterpret_cast<const f32x4 *>(g.dy + m * g.R + ar + 4 * j);
            }
            if (b_ok && br < g.R) {
#pragma unroll
                for (int j = 0; j < 4; j++) rb[j] = *reinterpret_cast<const f32x4 *>(g.w + (int64_t)(br + j) * g.K + k);
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const f32x4 lo = ra[2 * h], hi = ra[2 * h + 1];
            const u32x4 w = {pack2(lo[0], lo[1]), pack2(lo[2], lo[3]), pack2(hi[0], hi[1]), pack2(hi[2], hi[3])};
            *reinterpret_cast<u32x4 *>(As + slot_off(arow, 2 * part + h)) = w;
        }
        stage_transposed(Bs, kk, q4, rb);
    };
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int c = 0; c < 2; c++) acc[i][c] = zero;
    fetch(0);
    stage();
    __syncthreads();
    for (int r0 = 0; r0 < g.R; r0 += kKT16) {
        const bool more = r0 + kKT16 < g.R;
        if (more) fetch(r0 + kKT16);
        mma64(As, Bs, wr, wc, grp, l16, acc);
        __syncthreads();
        if (more) {
            stage();
            __syncthreads();
        }
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const int kc = k0 + wc * 32 + c * 16 + l16;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int64_t mr = m0 + wr * 32 + i * 16 + 4 * grp + r;
                if (mr < g.M && kc < g.K) {
                    const float pre = g.yprev[mr * g.K + kc] + g.pbias[kc & (g.bmod - 1)];
                    g.out[mr * g.K + kc] = pre > 0.f ? acc[i][c][r] : 0.f;
                }
            }
        }
}

// ---- host side: wgrad<MODE> and dgrad<CONV> of dqn_train_kernels.hip with the bf16 kernels
int wgrad16(int mode, WgradArgs g, float *grad_w, float *grad_b, const TrainScratch &ts, hipStream_t s,
            const char *what)
{
    const int64_t chunks = num_chunks(g.M);
    g.chunk = chunk_rows(g.M);
    g.out = chunks > 1 ? ts.wpart : grad_w;
    g.bout = chunks > 1 ? ts.bpart : grad_b;
    const dim3 grid((unsigned)((g.K + kT - 1) / kT), (unsigned)((g.N + kT - 1) / kT), (unsigned)chunks);
    if (mode == kDense)
        hipLaunchKernelGGL(k_wgrad16<kDense>, grid, dim3(256), 0, s, g);
    else if (mode == kConvF32)
        hipLaunchKernelGGL(k_wgrad16<kConvF32>, grid, dim3(256), 0, s, g);
    else
        hipLaunchKernelGGL(k_wgrad16<kConvU8>, grid, dim3(256), 0, s, g);
    int rc = launch_status(what);
    if (!rc && chunks > 1) rc = reduce(ts.wpart, ts.bpart, chunks, (int64_t)g.N * g.K, g.N, grad_w, grad_b, s, what);
    return rc;
}

int dgrad16(bool conv, const DgradArgs &g, hipStream_t s, const char *what)
{
    const dim3 grid((unsigned)((g.M + kT - 1) / kT), (unsigned)((g.K + kT - 1) / kT));
    if (conv) {
        if (g.Cout % 16) { set_error("%s: the bf16 input gradient needs Cout %% 16 == 0", what); return SNAKE_E_CONFIG; }
        hipLaunchKernelGGL(k_dgrad16<true>, grid, dim3(256), 0, s, g);
    } else {
        hipLaunchKernelGGL(k_dgrad16<false>, grid, dim3(256), 0, s, g);
    }
    return launch_status(what);
}

}  // namespace train
}  // namespace snake
