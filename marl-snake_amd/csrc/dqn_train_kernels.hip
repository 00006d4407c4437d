// dqn_train_kernels.hip -- the learner of train_dqn.py's Trainer.update_model
// (:228-257) on the device, in fp32: the backward pass of the fp32 forward
// (dqn32_kernels.hip), the TD loss, and clip_grad_norm_ + Adam.
//
// The backward consumes the forward's scratch: every layer's pre-activation
// Y1..Y5 (NHWC, without bias) and the x.max() > 1 flag. A ReLU mask is
// Y + bias > 0. dYi below is the gradient with respect to the pre-activation
// Yi (the mask already applied), so per layer
//
//   dW[n][k] = sum_m dY[m][n] * act(X)[m][k]       k_wgrad   (weight gradient)
//   db[n]    = sum_m dY[m][n]                      in k_wgrad (fc3: k_colsum)
//   dX[m][k] = (sum_n dY[m][n] * W[n][k]) * mask   k_dgrad   (input gradient)
//
// with act(X) formed on the fly in the forward's three operand modes. The
// convolutions' input gradient is the gather form: output cell (b, y, x),
// channel ci sums dY[(b, y+1-dy, x+1-dx)][co] * W[co][(dy*3+dx)*Cin + ci] over
// the nine taps and co (a 3x3 convolution of dY with the flipped, transposed
// weights); nothing is scattered. conv1 has no input gradient.
//
// k_wgrad and k_dgrad run on the fp32 matrix cores (v_mfma_f32_16x16x4_f32) on
// every geometry the forward accepts: a 256-thread workgroup owns a 64 x 64
// output tile, wave (w/2, w%2) a 32 x 32 quarter (2 x 2 MFMA tiles); both
// operands of 16 reduction steps are staged in LDS reduction-major (row stride
// kS = 68 floats), and lane group g of MFMA j reads reduction step 4g + j, so a
// fragment read touches 64 distinct banks. fc3 (A <= 64 outputs) runs on the
// vector ALUs, as in the forward.
//
// Split M: a weight or bias gradient reduces over M = B*h*w rows (B for the fc
// layers). M is cut into chunks of chunk_rows(M) = max(2048, ceil(M/128) rounded
// up to 16) rows -- a function of the shape alone --, every chunk writes a
// partial result, and k_reduce sums the partials in chunk order. With one
// chunk the result goes straight to the gradient. No floating-point atomics:
// every sum has a fixed order, results are bitwise reproducible.
//
// snake_dqn32_backward_bf16 is the same launch sequence with k_wgrad and k_dgrad
// replaced by their bf16 forms (dqn_train16_kernels.hip); what the two files
// share is in dqn_train_shared.h.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "dqn_train_shared.h"

namespace snake {
namespace train {

using dqn32::kConvF32;
using dqn32::kConvU8;
using dqn32::kDense;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kKT = 16;         // reduction steps per LDS stage
constexpr int kS = 68;          // LDS row stride in floats: 4 * 68 = 16 mod 64 banks
// 16 reduction steps of the workgroup's LDS tiles into this wave's 2 x 2 tiles
__device__ inline void mma16(const float *As, const float *Bs, int wr, int wc, int grp, int l16, f32x4 (&acc)[2][2])
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int kk = 4 * grp + j;
        float a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            a[i] = As[kk * kS + wr * 32 + i * 16 + l16];
            b[i] = Bs[kk * kS + wc * 32 + i * 16 + l16];
        }
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int c = 0; c < 2; c++)
                acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[c], acc[i][c], 0, 0, 0);
    }
}

// ---- weight gradient (WgradArgs): out[chunk][n][k] = sum_{m in chunk} dY[m][n] * act(X)[m][k]
template <int MODE>
__global__ void __launch_bounds__(256) k_wgrad(const WgradArgs g)
{
    __shared__ __attribute__((aligned(16))) float As[kKT * kS];
    __shared__ __attribute__((aligned(16))) float Bs[kKT * kS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, grp = lane >> 4, l16 = lane & 15;
    const int k0 = blockIdx.x * kT, n0 = blockIdx.y * kT;
    const int64_t mbeg = (int64_t)blockIdx.z * g.chunk;
    const int64_t mend = mbeg + g.chunk < g.M ? mbeg + g.chunk : g.M;
    // loaders: reduction step kk, four consecutive rows (n) / columns (k)
    const int kk = tid >> 4, q4 = (tid & 15) * 4;
    const int n = n0 + q4, k = k0 + q4;
    const bool a_ok = n < g.N, b_ok = k < g.K;
    int dy = 0, dx = 0, ci = 0;
    const int P = g.H * g.W;
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
    f32x4 ra, rb;
    auto fetch = [&](int64_t mt) {
        const int64_t m = mt + kk;
        const bool ok = m < mend;
        ra = zero;
        rb = zero;
        if (ok && a_ok) ra = *reinterpret_cast<const f32x4 *>(g.dy + m * g.N + n);
        if (!(ok && b_ok)) return;
        if constexpr (MODE == kDense) {
            rb = *reinterpret_cast<const f32x4 *>(reinterpret_cast<const float *>(g.x) + m * g.K + k);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float u = rb[i] + bias[i];
                rb[i] = u > 0.f ? u : 0.f;
            }
        } else {
            const int64_t b = m / P;
            const int p = (int)(m - b * P);
            const int y = p / g.W, x = p - y * g.W;
            const int yy = y + dy - 1, xx = x + dx - 1;
            if (yy < 0 || yy >= g.H || xx < 0 || xx >= g.W) return;   // zero padding
            const int64_t off = ((b * g.H + yy) * g.W + xx) * g.C + ci;
            if constexpr (MODE == kConvU8) {
                const uchar4 u = *reinterpret_cast<const uchar4 *>(reinterpret_cast<const uint8_t *>(g.x) + off);
                rb = (f32x4){(float)u.x, (float)u.y, (float)u.z, (float)u.w};
                if (scale255 != 0.f) {
#pragma unroll
                    for (int i = 0; i < 4; i++) rb[i] = rb[i] / 255.0f;   // (the reference divides)
                }
            } else {
                rb = *reinterpret_cast<const f32x4 *>(reinterpret_cast<const float *>(g.x) + off);
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const float u = rb[i] + bias[i];
                    rb[i] = u > 0.f ? u : 0.f;
                }
            }
        }
    };
    auto stage = [&]() {
        *reinterpret_cast<f32x4 *>(&As[kk * kS + q4]) = ra;
        *reinterpret_cast<f32x4 *>(&Bs[kk * kS + q4]) = rb;
    };
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int c = 0; c < 2; c++) acc[i][c] = zero;
    // the bias gradient rides along: in the workgroups of column tile 0, thread
    // t < 64 adds column n0 + t of every staged dY tile, rows in order
    const bool bias_owner = blockIdx.x == 0 && tid < kT;
    float bsum = 0.f;
    fetch(mbeg);
    stage();
    __syncthreads();
    for (int64_t mt = mbeg; mt < mend; mt += kKT) {
        const bool more = mt + kKT < mend;
        if (more) fetch(mt + kKT);
        if (bias_owner) {
#pragma unroll
            for (int r = 0; r < kKT; r++) bsum += As[r * kS + tid];
        }
        mma16(As, Bs, wr, wc, grp, l16, acc);
        __syncthreads();
        if (more) {
            stage();
            __syncthreads();
        }
    }
    if (bias_owner && n0 + tid < g.N) g.bout[(int64_t)blockIdx.z * g.N + n0 + tid] = bsum;
    float *out = g.out + (int64_t)blockIdx.z * g.N * g.K;
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

// ---- input gradient (DgradArgs): out[m][k] = (sum_r A(m, r) * B(r, k)) * (yprev[m][k] + pbias > 0)
template <bool CONV>
__global__ void __launch_bounds__(256) k_dgrad(const DgradArgs g)
{
    __shared__ __attribute__((aligned(16))) float As[kKT * kS];
    __shared__ __attribute__((aligned(16))) float Bs[kKT * kS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, grp = lane >> 4, l16 = lane & 15;
    const int64_t m0 = (int64_t)blockIdx.x * kT;
    const int k0 = blockIdx.y * kT;
    // A loader: row arow, reduction steps rq .. rq+3; B loader: step kk, columns k .. k+3
    const int arow = tid >> 2, rq = (tid & 3) * 4;
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
    f32x4 ra, rb;
    auto fetch = [&](int r0) {
        ra = zero;
        rb = zero;
        const int ar = r0 + rq, br = r0 + kk;
        if constexpr (CONV) {
            if (a_ok && ar < g.R) {
                const int tap = ar / g.Cout, co = ar - tap * g.Cout;
                const int dy = tap / 3, dx = tap - 3 * dy;
                const int yy = y + 1 - dy, xx = x + 1 - dx;
                if (yy >= 0 && yy < g.H && xx >= 0 && xx < g.W)
                    ra = *reinterpret_cast<const f32x4 *>(g.dy + ((bimg * g.H + yy) * g.W + xx) * g.Cout + co);
            }
            if (b_ok && br < g.R) {
                const int tap = br / g.Cout, co = br - tap * g.Cout;
                rb = *reinterpret_cast<const f32x4 *>(g.w + (int64_t)co * (9 * g.K) + tap * g.K + k);
            }
        } else {
            if (a_ok && ar < g.R) ra = *reinterpret_cast<const f32x4 *>(g.dy + m * g.R + ar);
            if (b_ok && br < g.R) rb = *reinterpret_cast<const f32x4 *>(g.w + (int64_t)br * g.K + k);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < 4; i++) As[(rq + i) * kS + arow] = ra[i];
        *reinterpret_cast<f32x4 *>(&Bs[kk * kS + q4]) = rb;
    };
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int c = 0; c < 2; c++) acc[i][c] = zero;
    fetch(0);
    stage();
    __syncthreads();
    for (int r0 = 0; r0 < g.R; r0 += kKT) {
        const bool more = r0 + kKT < g.R;
        if (more) fetch(r0 + kKT);
        mma16(As, Bs, wr, wc, grp, l16, acc);
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

// ---- bias gradient: out[chunk][n] = sum_{m in chunk} dY[m][n], N <= 256. Thread
// (rp, col) = (t / N, t % N) sums rows mbeg + rp, + R, ... (R = 256 / N), thread
// (0, col) then adds the R sums in rp order.
__global__ void __launch_bounds__(256) k_colsum(const float *dy, int64_t M, int N, int64_t chunk, float *out)
{
    __shared__ float s[256];
    const int tid = threadIdx.x, R = 256 / N, rp = tid / N, col = tid - rp * N;
    const int64_t mbeg = (int64_t)blockIdx.x * chunk;
    const int64_t mend = mbeg + chunk < M ? mbeg + chunk : M;
    float sum = 0.f;
    if (rp < R)
        for (int64_t m = mbeg + rp; m < mend; m += R) sum += dy[m * N + col];
    s[tid] = sum;
    __syncthreads();
    if (rp == 0) {
        float t = 0.f;
        for (int j = 0; j < R; j++) t += s[j * N + col];
        out[(int64_t)blockIdx.x * N + col] = t;
    }
}

// out[i] = partial[0][i] + partial[1][i] + ... in chunk order, for a weight
// gradient (nw elements) and its bias gradient (nb elements, may be 0) at once
__global__ void __launch_bounds__(256) k_reduce(const float *wpart, const float *bpart, int chunks, int64_t nw,
                                                int64_t nb, float *wout, float *bout)
{
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nw + nb) return;
    const bool is_w = i < nw;
    const int64_t n = is_w ? nw : nb;
    if (!is_w) i -= nw;
    const float *p = (is_w ? wpart : bpart) + i;
    float t = 0.f;
    int c = 0;
    for (; c + 8 <= chunks; c += 8) {       // eight loads in flight, added in chunk order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = p[(int64_t)(c + u) * n];
#pragma unroll
        for (int u = 0; u < 8; u++) t += v[u];
    }
    for (; c < chunks; c++) t += p[(int64_t)c * n];
    (is_w ? wout : bout)[i] = t;
}

// ---- fc3 on the vector ALUs (A <= 64 outputs)
// out[chunk][a][k] = sum_{m in chunk} dq[m][a] * relu(Y5[m][k] + b[k]); grid (chunks, A), 1024 threads:
// thread (ph, k) = (t / 128, t % 128) takes rows mbeg + ph, + 8, ...; thread (0, k) adds the eight sums in ph order
__global__ void __launch_bounds__(1024) k_fc3_wgrad(const float *dq, const float *y5, const float *b2, int64_t M,
                                                    int A, int64_t chunk, float *out)
{
    __shared__ float s[1024];
    const int k = threadIdx.x & 127, ph = threadIdx.x >> 7, a = blockIdx.y;
    const int64_t mbeg = (int64_t)blockIdx.x * chunk;
    const int64_t mend = mbeg + chunk < M ? mbeg + chunk : M;
    const float bias = b2[k];
    float t = 0.f;
    for (int64_t m = mbeg + ph; m < mend; m += 8) {
        const float u = y5[m * 128 + k] + bias;
        t = __builtin_fmaf(dq[m * A + a], u > 0.f ? u : 0.f, t);
    }
    s[threadIdx.x] = t;
    __syncthreads();
    if (ph == 0) {
        float r = 0.f;
        for (int j = 0; j < 8; j++) r += s[j * 128 + k];
        out[((int64_t)blockIdx.x * A + a) * 128 + k] = r;
    }
}

// dY5[m][k] = (sum_a dq[m][a] * W3[a][k]) * (Y5[m][k] + b[k] > 0)
__global__ void __launch_bounds__(256) k_fc3_dgrad(const float *dq, const float *w3, const float *y5,
                                                   const float *b2, int64_t M, int A, float *out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * 128) return;
    const int64_t m = i >> 7;
    const int k = (int)(i & 127);
    float t = 0.f;
    for (int a = 0; a < A; a++) t = __builtin_fmaf(dq[m * A + a], w3[a * 128 + k], t);
    out[i] = (y5[i] + b2[k] > 0.f) ? t : 0.f;
}

// ---- TD loss (train_dqn.py:243-250), one workgroup. Thread t takes rows t,
// t + 256, ...; the 256 sums are added by a fixed tree.
__global__ void __launch_bounds__(256) k_td_loss(const float *q, const int64_t *action, const float *reward,
                                                 const float *done, const float *next_q, int64_t B, int A,
                                                 float gamma, float *loss, float *dq, int *err)
{
    __shared__ float s[256];
    const int tid = threadIdx.x;
    const float fB = (float)B;
    float sum = 0.f;
    for (int64_t b = tid; b < B; b += 256) {
        int64_t a = action[b];
        if (a < 0 || a >= A) {
            a = a < 0 ? 0 : A - 1;
            if (err) atomicOr(err, 1);
        }
        float mx = next_q[b * A];
        for (int j = 1; j < A; j++) mx = fmaxf(mx, next_q[b * A + j]);
        const float target = reward[b] + ((1.f - done[b]) * gamma) * mx;
        const float d = q[b * A + a] - target;
        const float ad = fabsf(d);
        sum += ad < 1.f ? (0.5f * d) * d : ad - 0.5f;
        for (int j = 0; j < A; j++) dq[b * A + j] = 0.f;
        dq[b * A + a] = fminf(fmaxf(d, -1.f), 1.f) / fB;
    }
    s[tid] = sum;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) s[tid] += s[tid + h];
        __syncthreads();
    }
    if (tid == 0) *loss = s[0] / fB;
}

// ---- clip_grad_norm_ + Adam. Norm: block j of G sums the squares of elements
// [j*L, (j+1)*L) (thread t: j*L + t, + 256, ...; fixed tree), one block adds the
// G partials the same way. scratch: float [kNormBlocks] partials, then the norm.
constexpr int kNormBlocks = 1024;

__device__ inline float block_sum256(float v, float *s, int tid)
{
    s[tid] = v;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) s[tid] += s[tid + h];
        __syncthreads();
    }
    return s[0];
}

__global__ void __launch_bounds__(256) k_sumsq(const float *g, int64_t n, int64_t L, float *partial)
{
    __shared__ float s[256];
    const int tid = threadIdx.x;
    const int64_t beg = (int64_t)blockIdx.x * L, end = beg + L < n ? beg + L : n;
    float sum = 0.f;
    for (int64_t i = beg + tid; i < end; i += 256) sum += g[i] * g[i];
    const float t = block_sum256(sum, s, tid);
    if (tid == 0) partial[blockIdx.x] = t;
}

__global__ void __launch_bounds__(256) k_norm(float *scratch, int G, float *norm_out)
{
    __shared__ float s[256];
    const int tid = threadIdx.x;
    float sum = 0.f;
    for (int i = tid; i < G; i += 256) sum += scratch[i];
    const float t = block_sum256(sum, s, tid);
    if (tid == 0) {
        const float nrm = sqrtf(t);
        scratch[kNormBlocks] = nrm;
        if (norm_out) *norm_out = nrm;
    }
}

__global__ void __launch_bounds__(256) k_adam(float *p, const float *g, float *m, float *v, int64_t n,
                                              const float *norm, float max_norm, float beta1, float beta2,
                                              float step_size, float bc2_sqrt, float eps)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float coef = fminf(1.f, max_norm / (*norm + 1e-6f));
    const float gi = g[i] * coef;
    const float mi = beta1 * m[i] + (1.f - beta1) * gi;
    const float vi = beta2 * v[i] + ((1.f - beta2) * gi) * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = p[i] - step_size * (mi / denom);
}

// ---- host side
// (the train scratch: TrainScratch in dqn_train_shared.h)
int64_t train_scratch_bytes(const snake_dqn_cfg *cfg, int64_t B, void *base, TrainScratch *out)
{
    const int64_t P = (int64_t)cfg->height * cfg->width, BP = B * P;
    const int64_t cb = num_chunks(B), cp = num_chunks(BP);
    int64_t wp = 4;
    auto need = [&](int64_t chunks, int64_t N, int64_t K) {
        if (chunks > 1) wp = std::max(wp, chunks * N * K);
    };
    need(cb, cfg->num_actions, 128);
    need(cb, 128, 256);
    need(cb, 256, 64 * P);
    need(cp, 64, 576);
    need(cp, 64, 288);
    need(cp, 32, 9 * (int64_t)cfg->channels);
    wp = (wp + 3) / 4 * 4;
    const int64_t bp = std::max(cb, cp) * 256;
    const int64_t n5 = B * 128, n4 = B * 256, n3 = BP * 64, n2 = n3, n1 = BP * 32;
    if (out) {
        float *p = reinterpret_cast<float *>(base);
        out->dy5 = p;
        out->dy4 = out->dy5 + n5;
        out->dy3 = out->dy4 + n4;
        out->dy2 = out->dy3 + n3;
        out->dy1 = out->dy2 + n2;
        out->wpart = out->dy1 + n1;
        out->bpart = out->wpart + wp;
    }
    return 4 * (n5 + n4 + n3 + n2 + n1 + wp + bp);
}

int reduce(const float *wpart, const float *bpart, int64_t chunks, int64_t nw, int64_t nb, float *wout, float *bout,
           hipStream_t s, const char *what)
{
    hipLaunchKernelGGL(k_reduce, dim3((unsigned)((nw + nb + 255) / 256)), dim3(256), 0, s, wpart, bpart, (int)chunks,
                       nw, nb, wout, bout);
    return launch_status(what);
}

// a layer's weight and bias gradient
template <int MODE>
int wgrad(WgradArgs g, float *grad_w, float *grad_b, const TrainScratch &ts, hipStream_t s, const char *what)
{
    const int64_t chunks = num_chunks(g.M);
    g.chunk = chunk_rows(g.M);
    g.out = chunks > 1 ? ts.wpart : grad_w;
    g.bout = chunks > 1 ? ts.bpart : grad_b;
    const dim3 grid((unsigned)((g.K + kT - 1) / kT), (unsigned)((g.N + kT - 1) / kT), (unsigned)chunks);
    hipLaunchKernelGGL(k_wgrad<MODE>, grid, dim3(256), 0, s, g);
    int rc = launch_status(what);
    if (!rc && chunks > 1) rc = reduce(ts.wpart, ts.bpart, chunks, (int64_t)g.N * g.K, g.N, grad_w, grad_b, s, what);
    return rc;
}

int colsum(const float *dy, int64_t M, int N, float *grad, float *bpart, hipStream_t s, const char *what)
{
    const int64_t chunks = num_chunks(M);
    hipLaunchKernelGGL(k_colsum, dim3((unsigned)chunks), dim3(256), 0, s, dy, M, N, chunk_rows(M),
                       chunks > 1 ? bpart : grad);
    int rc = launch_status(what);
    if (!rc && chunks > 1) rc = reduce(bpart, bpart, chunks, N, 0, grad, grad, s, what);
    return rc;
}

template <bool CONV>
int dgrad(const DgradArgs &g, hipStream_t s, const char *what)
{
    const dim3 grid((unsigned)((g.M + kT - 1) / kT), (unsigned)((g.K + kT - 1) / kT));
    hipLaunchKernelGGL(k_dgrad<CONV>, grid, dim3(256), 0, s, g);
    return launch_status(what);
}

int check_train(const snake_dqn_cfg *cfg, int64_t batch, const char *who)
{
    const int rc = dqn32::check_cfg(cfg);
    if (rc) return rc;
    // (k_dgrad's grid: h*w column tiles for fc1, batch*h*w / 64 row tiles)
    if (batch < 0 || batch * cfg->height * cfg->width > ((int64_t)1 << 31)) {
        set_error("%s: batch must be at least 0 and batch * height * width at most 2^31 (got batch %lld)", who,
                  (long long)batch);
        return SNAKE_E_ARG;
    }
    return SNAKE_OK;
}

}  // namespace train
}  // namespace snake

using namespace snake;

extern "C" int64_t snake_dqn32_train_scratch(const snake_dqn_cfg *cfg, int64_t batch)
{
    const int rc = train::check_train(cfg, batch, "snake_dqn32_train_scratch");
    if (rc) return rc;
    return train::train_scratch_bytes(cfg, batch, nullptr, nullptr);
}

// The backward of both precisions: one validation and one launch sequence. With
// bf16 the five weight gradients and four input gradients of the matrix cores
// go to dqn_train16_kernels.hip's kernels; fc3 and the reductions are the same.
static int backward(const char *who, bool bf16, const snake_dqn_cfg *cfg, const snake_dqn32_net *net,
                    const uint8_t *obs, int64_t batch, const void *fwd_scratch, const float *dq, void *train_scratch,
                    const snake_dqn32_net *grad_net, void *stream)
{
    int rc = train::check_train(cfg, batch, who);
    if (rc) return rc;
    if (!net || !obs || !fwd_scratch || !dq || !train_scratch || !grad_net) {
        set_error("%s: NULL buffer", who);
        return SNAKE_E_ARG;
    }
    // the gradient block: snake_dqn32_net's twelve pointers, written here
    struct Grad {
        float *conv1_w, *conv2_w, *conv3_w, *fc1_w, *fc2_w, *fc3_w, *conv1_b, *conv2_b, *conv3_b, *fc1_b, *fc2_b, *fc3_b;
    };
    static_assert(sizeof(Grad) == sizeof(snake_dqn32_net), "one pointer per parameter");
    const Grad *grad = reinterpret_cast<const Grad *>(grad_net);
    const float *const wts[12] = {net->conv1_w, net->conv2_w, net->conv3_w, net->fc1_w, net->fc2_w, net->fc3_w,
                                  net->conv1_b, net->conv2_b, net->conv3_b, net->fc1_b, net->fc2_b, net->fc3_b};
    float *const grads[12] = {grad->conv1_w, grad->conv2_w, grad->conv3_w, grad->fc1_w, grad->fc2_w, grad->fc3_w,
                              grad->conv1_b, grad->conv2_b, grad->conv3_b, grad->fc1_b, grad->fc2_b, grad->fc3_b};
    for (int i = 0; i < 12; i++) {
        if (!wts[i] || !grads[i]) { set_error("%s: NULL weight or gradient pointer", who); return SNAKE_E_ARG; }
        if (((uintptr_t)wts[i] | (uintptr_t)grads[i]) & 15) {
            set_error("%s: weights and gradients must be 16-byte aligned", who);
            return SNAKE_E_ARG;
        }
    }
    if (((uintptr_t)fwd_scratch | (uintptr_t)train_scratch) & 15) {
        set_error("%s: the scratch buffers must be 16-byte aligned", who);
        return SNAKE_E_ARG;
    }
    if (batch == 0) return SNAKE_OK;
    const hipStream_t s = (hipStream_t)stream;
    DeviceGuard guard(s);       // (dg is the input gradient's argument block below)
    if (guard.dev < 0) return SNAKE_E_LAUNCH;
    dqn32::Scratch fw;
    dqn32::scratch_bytes(cfg, batch, const_cast<void *>(fwd_scratch), &fw);
    train::TrainScratch ts;
    train::train_scratch_bytes(cfg, batch, train_scratch, &ts);
    const int H = cfg->height, W = cfg->width, C = cfg->channels, A = cfg->num_actions;
    const int64_t P = (int64_t)H * W, BP = batch * P;
    // ---- fc3 (vector ALUs)
    {
        const int64_t chunks = train::num_chunks(batch);
        hipLaunchKernelGGL(train::k_fc3_wgrad, dim3((unsigned)chunks, (unsigned)A), dim3(1024), 0, s, dq, fw.y5,
                           net->fc2_b, batch, A, train::chunk_rows(batch), chunks > 1 ? ts.wpart : grad->fc3_w);
        if ((rc = launch_status("fc3 weight gradient"))) return rc;
        if (chunks > 1 && (rc = train::reduce(ts.wpart, ts.wpart, chunks, (int64_t)A * 128, 0, grad->fc3_w,
                                              grad->fc3_w, s, "fc3 weight gradient")))
            return rc;
        if ((rc = train::colsum(dq, batch, A, grad->fc3_b, ts.bpart, s, "fc3 bias gradient"))) return rc;
        hipLaunchKernelGGL(train::k_fc3_dgrad, dim3((unsigned)((batch * 128 + 255) / 256)), dim3(256), 0, s, dq,
                           net->fc3_w, fw.y5, net->fc2_b, batch, A, ts.dy5);
        if ((rc = launch_status("fc3 input gradient"))) return rc;
    }
    auto wgrad = [&](int mode, const train::WgradArgs &g, float *gw, float *gb, const train::TrainScratch &t,
                     hipStream_t st, const char *what) {
        if (bf16) return train::wgrad16(mode, g, gw, gb, t, st, what);
        if (mode == dqn32::kDense) return train::wgrad<dqn32::kDense>(g, gw, gb, t, st, what);
        if (mode == dqn32::kConvF32) return train::wgrad<dqn32::kConvF32>(g, gw, gb, t, st, what);
        return train::wgrad<dqn32::kConvU8>(g, gw, gb, t, st, what);
    };
    auto dgrad = [&](bool conv, const train::DgradArgs &g, hipStream_t st, const char *what) {
        if (bf16) return train::dgrad16(conv, g, st, what);
        return conv ? train::dgrad<true>(g, st, what) : train::dgrad<false>(g, st, what);
    };
    train::WgradArgs wg{};
    train::DgradArgs dg{};
    wg.H = dg.H = H;
    wg.W = dg.W = W;
    wg.scale_flag = fw.flag;
    // ---- fc2: dY5 [B][128], A = relu(Y4 + bfc1) [B][256]
    wg.dy = ts.dy5; wg.N = 128; wg.x = fw.y4; wg.xbias = net->fc1_b; wg.bmod = 256; wg.K = 256; wg.M = batch;
    if ((rc = wgrad(dqn32::kDense, wg, grad->fc2_w, grad->fc2_b, ts, s, "fc2 weight and bias gradient"))) return rc;
    dg.dy = ts.dy5; dg.w = net->fc2_w; dg.yprev = fw.y4; dg.pbias = net->fc1_b; dg.bmod = 256; dg.out = ts.dy4;
    dg.M = batch; dg.R = 128; dg.K = 256;
    if ((rc = dgrad(false, dg, s, "fc2 input gradient"))) return rc;
    // ---- fc1: dY4 [B][256], A = relu(Y3 + b3) flattened NHWC [B][64 P]
    wg.dy = ts.dy4; wg.N = 256; wg.x = fw.y3; wg.xbias = net->conv3_b; wg.bmod = 64; wg.K = (int)(64 * P);
    if ((rc = wgrad(dqn32::kDense, wg, grad->fc1_w, grad->fc1_b, ts, s, "fc1 weight and bias gradient"))) return rc;
    dg.dy = ts.dy4; dg.w = net->fc1_w; dg.yprev = fw.y3; dg.pbias = net->conv3_b; dg.bmod = 64; dg.out = ts.dy3;
    dg.R = 256; dg.K = (int)(64 * P);
    if ((rc = dgrad(false, dg, s, "fc1 input gradient"))) return rc;
    // ---- conv3: dY3 [BP][64], A = relu(Y2 + b2) patches
    wg.dy = ts.dy3; wg.N = 64; wg.x = fw.y2; wg.xbias = net->conv2_b; wg.C = 64; wg.K = 576; wg.M = BP;
    if ((rc = wgrad(dqn32::kConvF32, wg, grad->conv3_w, grad->conv3_b, ts, s, "conv3 weight and bias gradient"))) return rc;
    dg.dy = ts.dy3; dg.w = net->conv3_w; dg.yprev = fw.y2; dg.pbias = net->conv2_b; dg.bmod = 64; dg.out = ts.dy2;
    dg.M = BP; dg.R = 576; dg.K = 64; dg.Cout = 64;
    if ((rc = dgrad(true, dg, s, "conv3 input gradient"))) return rc;
    // ---- conv2: dY2 [BP][64], A = relu(Y1 + b1) patches
    wg.dy = ts.dy2; wg.x = fw.y1; wg.xbias = net->conv1_b; wg.C = 32; wg.K = 288;
    if ((rc = wgrad(dqn32::kConvF32, wg, grad->conv2_w, grad->conv2_b, ts, s, "conv2 weight and bias gradient"))) return rc;
    dg.dy = ts.dy2; dg.w = net->conv2_w; dg.yprev = fw.y1; dg.pbias = net->conv1_b; dg.bmod = 32; dg.out = ts.dy1;
    dg.K = 32;
    if ((rc = dgrad(true, dg, s, "conv2 input gradient"))) return rc;
    // ---- conv1: dY1 [BP][32], A = the observation as the forward read it
    wg.dy = ts.dy1; wg.N = 32; wg.x = obs; wg.xbias = nullptr; wg.C = C; wg.K = 9 * C;
    return wgrad(dqn32::kConvU8, wg, grad->conv1_w, grad->conv1_b, ts, s, "conv1 weight and bias gradient");
}

extern "C" int snake_dqn32_backward(const snake_dqn_cfg *cfg, const snake_dqn32_net *net, const uint8_t *obs,
                                    int64_t batch, const void *fwd_scratch, const float *dq, void *train_scratch,
                                    const snake_dqn32_net *grad_net, void *stream)
{
    return backward("snake_dqn32_backward", false, cfg, net, obs, batch, fwd_scratch, dq, train_scratch, grad_net,
                    stream);
}

extern "C" int snake_dqn32_backward_bf16(const snake_dqn_cfg *cfg, const snake_dqn32_net *net, const uint8_t *obs,
                                         int64_t batch, const void *fwd_scratch, const float *dq,
                                         void *train_scratch, const snake_dqn32_net *grad_net, void *stream)
{
    return backward("snake_dqn32_backward_bf16", true, cfg, net, obs, batch, fwd_scratch, dq, train_scratch,
                    grad_net, stream);
}

extern "C" int snake_dqn_td_loss(const float *q, const int64_t *action, const float *reward, const float *done,
                                 const float *next_q, int64_t batch, int32_t num_actions, float gamma,
                                 float *loss_out, float *dq, int32_t *err, void *stream)
{
    if (!q || !action || !reward || !done || !next_q || !loss_out || !dq) {
        set_error("snake_dqn_td_loss: NULL buffer");
        return SNAKE_E_ARG;
    }
    if (batch < 1 || batch > ((int64_t)1 << 24)) {
        set_error("snake_dqn_td_loss: batch must be in [1, 2^24] (got %lld)", (long long)batch);
        return SNAKE_E_ARG;
    }
    if (num_actions < 1 || num_actions > 64) {
        set_error("snake_dqn_td_loss: num_actions must be in [1, 64] (got %d)", num_actions);
        return SNAKE_E_CONFIG;
    }
    DeviceGuard dg((hipStream_t)stream);
    if (dg.dev < 0) return SNAKE_E_LAUNCH;
    hipLaunchKernelGGL(train::k_td_loss, dim3(1), dim3(256), 0, (hipStream_t)stream, q, action, reward, done, next_q,
                       batch, num_actions, gamma, loss_out, dq, err);
    return launch_status("k_td_loss");
}

extern "C" int snake_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                               int64_t step, float lr, float beta1, float beta2, float eps, float max_norm,
                               void *scratch, float *norm_out, void *stream)
{
    if (!param || !grad || !exp_avg || !exp_avg_sq || !scratch) {
        set_error("snake_adam_step: NULL buffer");
        return SNAKE_E_ARG;
    }
    if (n < 1) { set_error("snake_adam_step: n must be at least 1 (got %lld)", (long long)n); return SNAKE_E_ARG; }
    if (step < 1) { set_error("snake_adam_step: step must be at least 1 (got %lld)", (long long)step); return SNAKE_E_ARG; }
    if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) {
        set_error("snake_adam_step: beta1 and beta2 must be in [0, 1)");
        return SNAKE_E_CONFIG;
    }
    if (!(max_norm > 0.f)) { set_error("snake_adam_step: max_norm must be positive"); return SNAKE_E_CONFIG; }
    const hipStream_t s = (hipStream_t)stream;
    DeviceGuard dg(s);
    if (dg.dev < 0) return SNAKE_E_LAUNCH;
    float *sc = reinterpret_cast<float *>(scratch);
    const int G = (int)std::min<int64_t>(train::kNormBlocks, (n + 1023) / 1024);
    const int64_t L = ((n + G - 1) / G + 255) / 256 * 256;
    hipLaunchKernelGGL(train::k_sumsq, dim3(G), dim3(256), 0, s, grad, n, L, sc);
    int rc = launch_status("k_sumsq");
    if (rc) return rc;
    hipLaunchKernelGGL(train::k_norm, dim3(1), dim3(256), 0, s, sc, G, norm_out);
    if ((rc = launch_status("k_norm"))) return rc;
    // the bias corrections in double from the fp32 betas, as torch's Python scalars
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    const float step_size = (float)((double)lr / bc1), bc2_sqrt = (float)sqrt(bc2);
    hipLaunchKernelGGL(train::k_adam, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, param, grad, exp_avg,
                       exp_avg_sq, n, sc + train::kNormBlocks, max_norm, beta1, beta2, step_size, bc2_sqrt, eps);
    return launch_status("k_adam");
}
