// dqn32_kernels.hip -- the fp32 mode of the fused consumer: the reference's DQN
// forward (train_dqn.py:104-151) in fp32 arithmetic on any observation size,
// including train_dqn.py's own 20x20 full-map Config (:29-33).
//
// Every layer is one GEMM launch
//
//   Y[m][n] = sum_k act(X)[m][k] * W[n][k]          (W row-major [N][K])
//
// on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32
// accumulation; gfx950's fp32 matrix and vector peaks are both 157 TF, the
// matrix form needs far fewer issue slots): k_conv32_mfma for the convolutions
// (A from an LDS patch of the input maps), k_fc32_mfma for fc1/fc2 (LDS-staged
// tiles; up to 2 048 rows k_fc32_mfma_small, the same sums in 32 x 32 tiles,
// bit-equal per row). k_gemm32, a 128x64-tile GEMM on the vector ALUs, runs
// fc3 (A <= 64 outputs) and the convolutions of maps too wide for the patch.
// The A operand is formed on the fly (no im2col buffer):
//   kConvU8   conv1: m = (b, y, x), k = (tap, ci); X = the uint8 NHWC
//             observation, zero outside the map (padding 1), / 255 when the
//             batch holds a value > 1 (train_dqn.py:122: x / 255 if x.max() > 1)
//   kConvF32  conv2/conv3: the previous layer's pre-activation NHWC, with its
//             bias and ReLU applied as it is read (zero padding after the ReLU)
//   kDense    fc1/fc2/fc3: relu(Y + bias[k % bmod]) of the previous layer; fc1's
//             weight columns are permuted once on the host from the reference's
//             NCHW flatten (ch*h*w + p) to NHWC (p*64 + ch)
// Layers store pre-activations; the last adds fc3's bias, forward_features is
// relu(fc2 + bias). Scratch: Y1 [B*P][32], Y2, Y3 [B*P][64], Y4 [B][256],
// Y5 [B][128] fp32 + a 16-byte flag word (snake_dqn32_scratch).
//
// snake_dqn32_forward_bf16 is the same launch sequence with the five GEMMs of
// the matrix cores handed to dqn_fwd16_kernels.hip (bf16 operands, fp32 sums);
// the flag kernel, fc3 and the features are the launches below.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <stdlib.h>

#include <algorithm>

#include "dqn32_shared.h"   // GemmArgs, the operand modes, check_cfg, Scratch, the patch sizes

namespace snake {
namespace dqn32 {

constexpr int BM = 128, BN = 64, BK = 16, kThreads = 256;

// One 128 x 64 output tile per 256-thread workgroup: thread (tx, ty) of 16 x 16
// owns rows ty*4 .. +3 and 64 + ty*4 .. +3 and columns tx*4 .. +3 (32 fp32
// accumulators; per k one 16-byte LDS read of each operand quad feeds 32 FMAs).
// The next k tile's global loads are issued before the current tile's FMAs.
template <int MODE>
__global__ void __launch_bounds__(kThreads) k_gemm32(const GemmArgs g)
{
    __shared__ __attribute__((aligned(16))) float As[BK][BM + 4];
    __shared__ __attribute__((aligned(16))) float Bs[BK][BN + 4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int ar = tid >> 1, ak = (tid & 1) * 8;    // A loader: row ar, k ak .. ak+7
    const int br = tid >> 2, bk = (tid & 3) * 4;    // B loader: row br, k bk .. bk+3
    float acc[8][4] = {};
    float a[8], b[4];
    // A loader state: the row's map cell (conv modes) and the (tap, channel) of
    // its k offset, advanced by BK per tile without divisions
    const int64_t m = m0 + ar;
    const bool row_ok = m < g.M;
    int y = 0, x = 0, tap = 0, ci = 0;
    int64_t rowbase = 0;
    if constexpr (MODE != kDense) {
        const int P = g.H * g.W;
        const int64_t bb = row_ok ? m / P : 0;
        const int p = (int)(row_ok ? m - bb * P : 0);
        y = p / g.W;
        x = p - y * g.W;
        rowbase = ((bb * g.H + y) * g.W + x) * g.C;
        tap = ak / g.C;
        ci = ak - tap * g.C;
    } else {
        rowbase = m * g.K;
    }
    auto gather = [&](int k0, int c0, float (&v)[4]) {      // A[m][k0 .. k0+3], channel c0 (conv)
        v[0] = v[1] = v[2] = v[3] = 0.f;
        if (!row_ok || k0 >= g.K) return;
        if constexpr (MODE == kDense) {
            const float4 f = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(g.x) + rowbase + k0);
            const float t[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float u = t[i] + g.xbias[(k0 + i) & (g.bmod - 1)];
                v[i] = u > 0.f ? u : 0.f;
            }
        } else {
            const int dy = (tap * 11) >> 5, dx = tap - 3 * dy;      // tap / 3, tap % 3 for tap < 9
            const int yy = y + dy - 1, xx = x + dx - 1;
            if (yy < 0 || yy >= g.H || xx < 0 || xx >= g.W) return;   // zero padding
            const int64_t off = rowbase + (int64_t)(((dy - 1) * g.W + (dx - 1)) * g.C + c0);
            if constexpr (MODE == kConvU8) {
                const uchar4 u = *reinterpret_cast<const uchar4 *>(reinterpret_cast<const uint8_t *>(g.x) + off);
                v[0] = (float)u.x; v[1] = (float)u.y; v[2] = (float)u.z; v[3] = (float)u.w;
                if (*g.scale_flag) {
#pragma unroll
                    for (int i = 0; i < 4; i++) v[i] = v[i] / 255.0f;
                }
            } else {
                const float4 f = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(g.x) + off);
                const float t[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const float u = t[i] + g.xbias[c0 + i];
                    v[i] = u > 0.f ? u : 0.f;
                }
            }
        }
    };
    auto load = [&](int k0) {
        float t0[4], t1[4];
        gather(k0 + ak, ci, t0);
        gather(k0 + ak + 4, ci + 4, t1);          // same tap: C % 8 == 0
        if constexpr (MODE != kDense) {
            ci += BK;
            while (ci >= g.C) { ci -= g.C; tap++; }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) { a[i] = t0[i]; a[4 + i] = t1[i]; }
        const int n = n0 + br, kk = k0 + bk;
        b[0] = b[1] = b[2] = b[3] = 0.f;
        if (n < g.N && kk < g.K) {
            const float *wr = g.w + (int64_t)n * g.K + kk;
            if (kk + 4 <= g.K) {
                const float4 f = *reinterpret_cast<const float4 *>(wr);
                b[0] = f.x; b[1] = f.y; b[2] = f.z; b[3] = f.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) b[i] = (kk + i < g.K) ? wr[i] : 0.f;
            }
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < 8; i++) As[ak + i][ar] = a[i];
#pragma unroll
        for (int i = 0; i < 4; i++) Bs[bk + i][br] = b[i];
    };
    load(0);
    store();
    __syncthreads();
    for (int k0 = 0; k0 < g.K; k0 += BK) {
        const bool more = k0 + BK < g.K;
        if (more) load(k0 + BK);
#pragma unroll
        for (int k = 0; k < BK; k++) {
            const float4 a0 = *reinterpret_cast<const float4 *>(&As[k][ty * 4]);
            const float4 a1 = *reinterpret_cast<const float4 *>(&As[k][64 + ty * 4]);
            const float4 bq = *reinterpret_cast<const float4 *>(&Bs[k][tx * 4]);
            const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const float bv[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
            for (int i = 0; i < 8; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[i][j] = __builtin_fmaf(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
        if (more) {
            store();
            __syncthreads();
        }
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int64_t m = m0 + (i < 4 ? ty * 4 + i : 64 + ty * 4 + i - 4);
        if (m >= g.M) continue;
        const int n = n0 + tx * 4;
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; j++) o[j] = acc[i][j] + ((g.ybias && n + j < g.N) ? g.ybias[n + j] : 0.f);
        if (n + 4 <= g.N && (g.N & 3) == 0) {
            *reinterpret_cast<float4 *>(g.y + m * g.N + n) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (n + j < g.N) g.y[m * g.N + n + j] = o[j];
        }
    }
}

// ------------------------------------------------------------------------
// The convolutions on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: exact fp32
// products, fp32 accumulation). Implicit GEMM, rows = output positions of the
// batch flattened (b, y, x), columns = output channels, k = (tap, ci).
//
// The A operand comes from an LDS patch, not from global gathers: the batch's
// maps are seen as one tall image, map b's row y at tall row b*(H+1)+y+1, with
// one zero row between maps (and above the first), so a 3x3 tap never needs a
// bounds test. A workgroup's 128 consecutive rows need tall rows
// [T(m0)-1, T(m0+127)+1] x all W+2 bordered columns; they are staged once,
// with the previous layer's bias and ReLU (or the uint8 scaling) applied and
// zeros written for borders, separators and rows past the batch. A cell holds
// C channels padded to conv_cell_stride(C) floats (bank-conflict-free
// ds_read_b128 rows).
//
// MFMA k order: in a 16-k block, lane group g = lane/16 owns k0+4g .. k0+4g+3
// and MFMA j of the block takes k0+4g+j from every group, so one ds_read_b128
// (A: four consecutive channels of one cell) and one 16-byte global load (B: W
// row-major [N][K]) feed four MFMAs. Output fragment: lane l, register r ->
// row 4*(l/16)+r, column l%16.
// (kConvRows, the patch sizes and the cell stride: dqn32_shared.h)
typedef float f32x4 __attribute__((ext_vector_type(4)));

// NT = output channels / 16 (2: conv1, 4: conv2/conv3). Wave w takes column
// tile w % NT and 16*NT/... row tiles: NT == 4 -> all 8 row tiles, NT == 2 ->
// row tiles 4*(w/2) .. +3. WT (NT == 4 only): wave tiles of 4 row x 2 column
// tiles instead -- wave w takes column tiles 2*(w%2), +1 and row tiles
// 4*(w/2) .. +3: each A fragment feeds two MFMAs (half the LDS reads per MFMA),
// each block loads two B fragments.
template <int MODE, int NT, bool WT = false>
__global__ void __launch_bounds__(256) k_conv32_mfma(const GemmArgs g)
{
    static_assert(!WT || NT == 4, "wave tiles of 4 x 2 need four column tiles");
    extern __shared__ __attribute__((aligned(16))) float patch[];
    __shared__ int offs[4 * 76];   // K <= 9 * 128: 72 blocks + padding + 1
    constexpr int RT = WT ? 4 : (NT == 4 ? 8 : 4);   // row tiles per wave
    constexpr int CT = WT ? 2 : 1;                   // column tiles per wave
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = g.H, W = g.W, C = g.C, K = g.K, N = g.N;
    const int W2 = W + 2, CS = conv_cell_stride(C), P = H * W;
    const int64_t M = g.M, m0 = (int64_t)blockIdx.x * kConvRows;
    const int64_t B = M / P;
    // tall row of the first position
    const int64_t b0 = m0 / P;
    const int p0 = (int)(m0 - b0 * P);
    const int64_t t0 = b0 * (H + 1) + p0 / W + 1 - 1;   // first patch row (halo above)
    const int PR = conv_patch_rows(H, W);
    // ---- stage the patch: cell (r, c) = tall row t0 + r, bordered column c
    const int C4 = C >> 2, cells = PR * W2;
    float scale = 1.f;
    if constexpr (MODE == kConvU8) scale = *g.scale_flag ? (1.f / 255.f) : 1.f;
    // 8 loads in flight per thread, then the conversions and LDS stores
    constexpr int kBatch = 8;
    const int total = cells * C4;
    for (int q0 = tid; q0 < total; q0 += 256 * kBatch) {
        f32x4 v[kBatch];
        int dst[kBatch];
        bool live[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; u++) {
            const int q = q0 + 256 * u;
            const int cell = q / C4, c4 = q - cell * C4;
            const int r = cell / W2, c = cell - r * W2;
            const int64_t t = t0 + r;
            const int64_t b = t / (H + 1);
            const int yy = (int)(t - b * (H + 1)) - 1, xx = c - 1;
            dst[u] = q < total ? cell * CS + 4 * c4 : -1;
            // unconditional loads (element 0 for cells outside the maps, zeroed
            // below): a load under a branch is waited for inside the branch
            live[u] = q < total && yy >= 0 && xx >= 0 && xx < W && b < B;
            const int64_t off = live[u] ? ((b * H + yy) * W + xx) * C + 4 * c4 : 0;
            if constexpr (MODE == kConvU8) {
                const uchar4 uc = *reinterpret_cast<const uchar4 *>(reinterpret_cast<const uint8_t *>(g.x) + off);
                v[u].x = (float)uc.x; v[u].y = (float)uc.y; v[u].z = (float)uc.z; v[u].w = (float)uc.w;
            } else {
                v[u] = *reinterpret_cast<const f32x4 *>(reinterpret_cast<const float *>(g.x) + off);
            }
        }
#pragma unroll
        for (int u = 0; u < kBatch; u++) {
            f32x4 w = v[u];
            if constexpr (MODE == kConvU8) {
                // (the reference divides: x / 255)
                if (scale != 1.f) { w.x = w.x / 255.0f; w.y = w.y / 255.0f; w.z = w.z / 255.0f; w.w = w.w / 255.0f; }
            } else {
                const int c4 = (q0 + 256 * u) % C4;
                const float *bb = g.xbias + 4 * c4;   // (the caller's bias: no alignment assumed)
                w.x += bb[0]; w.y += bb[1]; w.z += bb[2]; w.w += bb[3];
                w.x = w.x > 0.f ? w.x : 0.f; w.y = w.y > 0.f ? w.y : 0.f;
                w.z = w.z > 0.f ? w.z : 0.f; w.w = w.w > 0.f ? w.w : 0.f;
            }
            if (!live[u]) w = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (dst[u] >= 0) *reinterpret_cast<f32x4 *>(patch + dst[u]) = w;
        }
    }
    __syncthreads();
    // ---- this wave's tiles
    const int ct = WT ? 2 * (wave & 1) : wave % NT;
    const int rt0 = WT ? 4 * (wave >> 1) : (NT == 4 ? 0 : 4 * (wave / 2));
    const int grp = lane >> 4, l16 = lane & 15;
    int abase[RT];   // LDS 16-byte index of each row tile's lane-row cell (tap (1,1), channel 0)
#pragma unroll
    for (int i = 0; i < RT; i++) {
        int64_t m = m0 + (rt0 + i) * 16 + l16;
        if (m >= M) m = M - 1;   // computed, never stored
        const int64_t b = m / P;
        const int p = (int)(m - b * P), y = p / W, x = p - y * W;
        const int r = (int)(b * (H + 1) + y + 1 - t0);
        abase[i] = ((r * W2 + x + 1) * CS) >> 2;
    }
    int col[CT];
    const float *wrow[CT];
#pragma unroll
    for (int c = 0; c < CT; c++) {
        col[c] = (ct + c) * 16 + l16;
        wrow[c] = g.w + (int64_t)col[c] * K;
    }
    f32x4 acc[RT][CT];
#pragma unroll
    for (int i = 0; i < RT; i++)
#pragma unroll
        for (int c = 0; c < CT; c++) acc[i][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // per 16-k block and lane group: the LDS offset (in 16-byte units) of its
    // (tap, channel) from a row's centre cell; blocks are processed kRing at a
    // time, and k past K (the padding blocks, one extra entry for the last
    // prefetch) reads the centre cell with a zero B operand
    constexpr int kRing = 2;
    const int nb = (K + 15) >> 4, nbp = (nb + kRing - 1) / kRing * kRing;
    for (int q = tid; q < 4 * (nbp + 1); q += 256) {
        const int kq = 4 * q;
        int o = 0;
        if (kq < K) {
            const int tap = kq / C, ci = kq - tap * C;
            const int dy = (tap * 11) >> 5, dx = tap - 3 * dy;
            o = (((dy - 1) * W2 + (dx - 1)) * CS + ci) >> 2;
        }
        offs[q] = o;
    }
    __syncthreads();
    // B: kRing blocks of loads in flight (unconditional, clamped addresses);
    // A: the next block's fragments are read before this block's MFMAs
    const f32x4 *patch4 = reinterpret_cast<const f32x4 *>(patch);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 bq[kRing][CT];
#pragma unroll
    for (int d = 0; d < kRing; d++)
#pragma unroll
        for (int c = 0; c < CT; c++)
            bq[d][c] = *reinterpret_cast<const f32x4 *>(wrow[c] + min(16 * d + 4 * grp, K - 4));
    f32x4 a[RT];
    {
        const int off = offs[grp];
#pragma unroll
        for (int i = 0; i < RT; i++) a[i] = patch4[abase[i] + off];
    }
    // two blocks per iteration: the B ring and the A fragments ping-pong
    // between fixed registers (a register copy would wait for the load it copies)
    f32x4 a2[RT];
    auto block = [&](int kb, f32x4 (&acur)[RT], f32x4 (&anext)[RT], f32x4 (&bslot)[CT]) {
        const int off = offs[4 * (kb + 1) + grp];
#pragma unroll
        for (int i = 0; i < RT; i++) anext[i] = patch4[abase[i] + off];
        // (conv2/conv3: K = 9 * 32 or 9 * 64, a multiple of 16 -- no mask, so
        // nothing ties the ring's loads to a select at issue time)
        f32x4 bv[CT];
#pragma unroll
        for (int c = 0; c < CT; c++) {
            bv[c] = bslot[c];
            if constexpr (MODE == kConvU8) bv[c] = 16 * kb + 4 * grp < K ? bv[c] : zero;
            bslot[c] = *reinterpret_cast<const f32x4 *>(wrow[c] + min(16 * (kb + kRing) + 4 * grp, K - 4));
        }
        // (the loads stay issued ahead of this block's MFMAs: without the
        // barriers the scheduler sinks them next to their uses)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int i = 0; i < RT; i++)
#pragma unroll
                for (int c = 0; c < CT; c++)
                    acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(acur[i][j], bv[c][j], acc[i][c], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    for (int kb = 0; kb < nbp; kb += 2) {
        block(kb, a, a2, bq[0]);
        block(kb + 1, a2, a, bq[1]);
    }
    // ---- pre-activations out: Y[m][n]
#pragma unroll
    for (int i = 0; i < RT; i++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int64_t m = m0 + (rt0 + i) * 16 + 4 * grp + r;
#pragma unroll
            for (int c = 0; c < CT; c++)
                if (m < M) g.y[m * N + col[c]] = acc[i][c][r];
        }
    }
}

template <int MODE, int NT>
int conv_mfma(const GemmArgs &g, hipStream_t s, const char *what)
{
    const int64_t lds = conv_patch_bytes(g.H, g.W, g.C);
    const dim3 grid((unsigned)((g.M + kConvRows - 1) / kConvRows));
    // 4 x 2 wave tiles for the 64-channel layers (20x20x8, 16 384 observations:
    // conv2/conv3 3 715 -> 3 666 us per launch on average against 8 x 1, forward
    // 9.84 -> 9.75 ms; parity green)
    if constexpr (NT == 4) hipLaunchKernelGGL((k_conv32_mfma<MODE, 4, true>), grid, dim3(256), (size_t)lds, s, g);
    else hipLaunchKernelGGL((k_conv32_mfma<MODE, NT>), grid, dim3(256), (size_t)lds, s, g);
    return launch_status(what);
}

// The dense layers with N a multiple of 128 (fc1: 64hw -> 256, fc2: 256 -> 128)
// on the fp32 matrix cores: Y = relu(X + bias[k % bmod]) W^T. A workgroup of
// 8 waves owns 128 rows x 128 columns; wave (rg, cg) = (w % 4, w / 4) owns rows
// 32 rg .. +31 and columns 64 cg .. +63 (2 x 4 tiles of 16 x 16). Per 32-k block
// the A tile (bias and ReLU applied once) and the W tile are staged in LDS,
// double-buffered: the next block's global loads are issued before this
// block's MFMAs and stored after them, one barrier per block. Rows of 32 k
// padded to 40 floats: the row lanes of a ds_read_b128 group hit distinct banks.
constexpr int kFcK = 32, kFcS = kFcK + 8;   // rows of 10 slots: 2 mod 4 (see conv_cell_stride)

__global__ void __launch_bounds__(512) k_fc32_mfma(const GemmArgs g)
{
    __shared__ __attribute__((aligned(16))) float As[2][128 * kFcS];
    __shared__ __attribute__((aligned(16))) float Bs[2][128 * kFcS];
    __shared__ __attribute__((aligned(16))) float bias[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rg = wave & 3, cg = wave >> 2, grp = lane >> 4, l16 = lane & 15;
    const int K = g.K, N = g.N;
    const int64_t M = g.M;
    for (int q = tid; q < g.bmod; q += 512) bias[q] = g.xbias[q];
    const int64_t m0 = (int64_t)blockIdx.x * 128;
    const int n0 = blockIdx.y * 128;
    // stager: thread t loads float4 (row t/8 and 64 + t/8, k 4*(t%8)) of A and of W
    const int sr = tid >> 3, sk = 4 * (tid & 7);
    const float *ap[2];
    const float *wp[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        int64_t m = m0 + sr + 64 * h;
        if (m >= M) m = M - 1;   // computed, never stored
        ap[h] = reinterpret_cast<const float *>(g.x) + m * K + sk;
        wp[h] = g.w + (int64_t)(n0 + sr + 64 * h) * K + sk;
    }
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 ra[2], rw[2];
    auto fetch = [&](int k0) {
        const bool ok = k0 + sk < K;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            ra[h] = ok ? *reinterpret_cast<const f32x4 *>(ap[h] + k0) : zero;
            rw[h] = ok ? *reinterpret_cast<const f32x4 *>(wp[h] + k0) : zero;
        }
    };
    const int bm = g.bmod - 1;
    auto stage = [&](int buf, int k0) {
        const f32x4 bv = *reinterpret_cast<const f32x4 *>(&bias[(k0 + sk) & bm]);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            f32x4 a;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float u = ra[h][j] + bv[j];
                a[j] = u > 0.f ? u : 0.f;   // (k past K: W is zero there)
            }
            *reinterpret_cast<f32x4 *>(&As[buf][(sr + 64 * h) * kFcS + sk]) = a;
            *reinterpret_cast<f32x4 *>(&Bs[buf][(sr + 64 * h) * kFcS + sk]) = rw[h];
        }
    };
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int c = 0; c < 4; c++) acc[i][c] = zero;
    fetch(0);
    __syncthreads();   // bias
    stage(0, 0);
    __syncthreads();
    const int nb = (K + kFcK - 1) / kFcK;
    for (int kb = 0; kb < nb; kb++) {
        const int cur = kb & 1;
        if (kb + 1 < nb) fetch((kb + 1) * kFcK);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            f32x4 a[2], b[4];
#pragma unroll
            for (int i = 0; i < 2; i++)
                a[i] = *reinterpret_cast<const f32x4 *>(&As[cur][(rg * 32 + i * 16 + l16) * kFcS + 16 * h + 4 * grp]);
#pragma unroll
            for (int c = 0; c < 4; c++)
                b[c] = *reinterpret_cast<const f32x4 *>(&Bs[cur][(cg * 64 + c * 16 + l16) * kFcS + 16 * h + 4 * grp]);
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int c = 0; c < 4; c++)
                        acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][j], b[c][j], acc[i][c], 0, 0, 0);
        }
        if (kb + 1 < nb) stage(cur ^ 1, (kb + 1) * kFcK);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int n = n0 + cg * 64 + c * 16 + l16;
            const float yb = g.ybias ? g.ybias[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int64_t m = m0 + rg * 32 + i * 16 + 4 * grp + r;
                if (m < M) g.y[m * N + n] = acc[i][c][r] + yb;
            }
        }
}

// The same layers at small batches (a learner's B = 512: k_fc32_mfma's grid for
// fc1 would be 4 x 2 workgroups, each walking K = 64 h w alone): 32 x 32 tiles,
// four waves of one 16 x 16 tile each, wave (rg, cg) = (w % 2, w / 2). Staging,
// the k order inside a 32-k block and the MFMA sequence per output element are
// k_fc32_mfma's, so every output has the same bits on either kernel.
__global__ void __launch_bounds__(256) k_fc32_mfma_small(const GemmArgs g)
{
    __shared__ __attribute__((aligned(16))) float As[2][32 * kFcS];
    __shared__ __attribute__((aligned(16))) float Bs[2][32 * kFcS];
    __shared__ __attribute__((aligned(16))) float bias[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rg = wave & 1, cg = wave >> 1, grp = lane >> 4, l16 = lane & 15;
    const int K = g.K, N = g.N;
    const int64_t M = g.M;
    for (int q = tid; q < g.bmod; q += 256) bias[q] = g.xbias[q];
    const int64_t m0 = (int64_t)blockIdx.x * 32;
    const int n0 = blockIdx.y * 32;
    // stager: thread t loads float4 (row t/8, k 4*(t%8)) of A and of W
    const int sr = tid >> 3, sk = 4 * (tid & 7);
    int64_t ms = m0 + sr;
    if (ms >= M) ms = M - 1;   // computed, never stored
    const float *ap = reinterpret_cast<const float *>(g.x) + ms * K + sk;
    const float *wp = g.w + (int64_t)(n0 + sr) * K + sk;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    // kAhead blocks of global loads in flight (one block ahead, a wave spent a
    // memory latency per 32-k block: 128 workgroups cannot hide it by occupancy);
    // the loop is unrolled by kAhead so that the ring's slots are fixed registers
    constexpr int kAhead = 4;
    f32x4 ra[kAhead], rw[kAhead];
    auto fetch = [&](int slot, int k0) {
        const bool ok = k0 + sk < K;
        ra[slot] = ok ? *reinterpret_cast<const f32x4 *>(ap + k0) : zero;
        rw[slot] = ok ? *reinterpret_cast<const f32x4 *>(wp + k0) : zero;
    };
    const int bm = g.bmod - 1;
    auto stage = [&](int buf, int slot, int k0) {
        const f32x4 bv = *reinterpret_cast<const f32x4 *>(&bias[(k0 + sk) & bm]);
        f32x4 a;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float u = ra[slot][j] + bv[j];
            a[j] = u > 0.f ? u : 0.f;   // (k past K: W is zero there)
        }
        *reinterpret_cast<f32x4 *>(&As[buf][sr * kFcS + sk]) = a;
        *reinterpret_cast<f32x4 *>(&Bs[buf][sr * kFcS + sk]) = rw[slot];
    };
    f32x4 acc = zero;
#pragma unroll
    for (int u = 0; u < kAhead; u++) fetch(u, u * kFcK);   // (blocks past K: zeros, no load)
    __syncthreads();   // bias
    stage(0, 0, 0);
    fetch(0, kAhead * kFcK);
    __syncthreads();
    const int nb = (K + kFcK - 1) / kFcK;
    for (int kb0 = 0; kb0 < nb; kb0 += kAhead) {
#pragma unroll
        for (int u = 0; u < kAhead; u++) {
            const int kb = kb0 + u;
            if (kb >= nb) break;   // (uniform)
            const int cur = u & 1;   // kb & 1: kAhead is even
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const f32x4 a = *reinterpret_cast<const f32x4 *>(&As[cur][(rg * 16 + l16) * kFcS + 16 * h + 4 * grp]);
                const f32x4 b = *reinterpret_cast<const f32x4 *>(&Bs[cur][(cg * 16 + l16) * kFcS + 16 * h + 4 * grp]);
#pragma unroll
                for (int j = 0; j < 4; j++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc, 0, 0, 0);
            }
            if (kb + 1 < nb) {
                const int slot = (u + 1) % kAhead;   // block kb + 1's registers
                stage(cur ^ 1, slot, (kb + 1) * kFcK);
                fetch(slot, (kb + 1 + kAhead) * kFcK);
            }
            __syncthreads();
        }
    }
    const int n = n0 + cg * 16 + l16;
    const float yb = g.ybias ? g.ybias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int64_t m = m0 + rg * 16 + 4 * grp + r;
        if (m < M) g.y[m * N + n] = acc[r] + yb;
    }
}

constexpr int64_t kFcSmallRows = 2048;   // up to this many rows: k_fc32_mfma_small

int fc_mfma(const GemmArgs &g, hipStream_t s, const char *what)
{
    const dim3 grid((unsigned)((g.M + 127) / 128), (unsigned)(g.N / 128));
    if (g.M <= kFcSmallRows)
        hipLaunchKernelGGL(k_fc32_mfma_small, dim3((unsigned)((g.M + 31) / 32), (unsigned)(g.N / 32)), dim3(256), 0, s, g);
    else
        hipLaunchKernelGGL(k_fc32_mfma, grid, dim3(512), 0, s, g);
    return launch_status(what);
}

// flag = any observation byte > 1 (the reference's x.max() > 1.0 test)
__global__ void k_obs_max(const uint8_t *obs, int64_t n, int *flag)
{
    int hit = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        hit |= obs[i] > 1;
    if (__any(hit) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// forward_features = relu(fc2 pre-activation + bias)
__global__ void k_bias_relu(const float *y, const float *bias, int n, int64_t total, float *out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const float t = y[i] + bias[i % n];
        out[i] = t > 0.f ? t : 0.f;
    }
}

template <int MODE>
int gemm(const GemmArgs &g, hipStream_t s, const char *what)
{
    const dim3 grid((unsigned)((g.M + BM - 1) / BM), (unsigned)((g.N + BN - 1) / BN));
    hipLaunchKernelGGL(k_gemm32<MODE>, grid, dim3(kThreads), 0, s, g);
    return launch_status(what);
}

}  // namespace dqn32
}  // namespace snake

using namespace snake;

extern "C" int64_t snake_dqn32_scratch(const snake_dqn_cfg *cfg, int64_t batch)
{
    const int rc = dqn32::check_cfg(cfg);
    if (rc) return rc;
    if (batch < 0) { set_error("snake_dqn32_scratch: batch < 0"); return SNAKE_E_ARG; }
    return dqn32::scratch_bytes(cfg, batch, nullptr, nullptr);
}

// The forward of both precisions: one validation and one launch sequence. With
// bf16 the five GEMMs of the matrix cores go to dqn_fwd16_kernels.hip's kernel
// (any map width, fc1 split along K); the flag kernel, fc3 and the features are
// the same launches.
static int forward(const char *who, bool bf16, const snake_dqn_cfg *cfg, const snake_dqn32_net *net,
                   const uint8_t *obs, int64_t batch, void *scratch, float *q_out, float *feat_out, void *stream)
{
    int rc = dqn32::check_cfg(cfg);
    if (rc) return rc;
    if (!net || !obs || !scratch || !q_out || !net->conv1_w || !net->conv2_w || !net->conv3_w || !net->fc1_w ||
        !net->fc2_w || !net->fc3_w || !net->conv1_b || !net->conv2_b || !net->conv3_b || !net->fc1_b ||
        !net->fc2_b || !net->fc3_b) {
        set_error("%s: NULL buffer", who);
        return SNAKE_E_ARG;
    }
    if (batch < 0) { set_error("%s: batch < 0", who); return SNAKE_E_ARG; }
    if (batch == 0) return SNAKE_OK;
    const hipStream_t s = (hipStream_t)stream;
    DeviceGuard dg(s);
    if (dg.dev < 0) return SNAKE_E_LAUNCH;
    dqn32::Scratch sc;
    float *partials = nullptr;
    if (bf16) dqn32::fwd16_scratch_bytes(cfg, batch, scratch, &sc, &partials);
    else dqn32::scratch_bytes(cfg, batch, scratch, &sc);
    const int H = cfg->height, W = cfg->width, C = cfg->channels, A = cfg->num_actions;
    const int64_t P = (int64_t)H * W, BP = batch * P;
    if (hipMemsetAsync(sc.flag, 0, 16, s) != hipSuccess) { set_error("snake_dqn32: memset failed"); return SNAKE_E_LAUNCH; }
    {
        const int64_t n = BP * C;
        const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
        hipLaunchKernelGGL(dqn32::k_obs_max, dim3(blocks), dim3(256), 0, s, obs, n, sc.flag);
        if ((rc = launch_status("k_obs_max"))) return rc;
    }
    dqn32::GemmArgs g{};
    g.H = H; g.W = W;
    // the convolutions on the matrix cores when the widest layer's LDS patch
    // fits (every map up to ~40 wide), else the vector-ALU GEMM
    const bool mfma = dqn32::conv_patch_bytes(H, W, std::max(C, 64)) <= dqn32::kPatchMaxBytes;
    // conv1: uint8 NHWC obs -> Y1 [B*P][32]
    g.x = obs; g.xbias = nullptr; g.w = net->conv1_w; g.y = sc.y1; g.ybias = nullptr;
    g.M = BP; g.N = 32; g.K = 9 * C; g.C = C; g.scale_flag = sc.flag;
    if ((rc = bf16   ? dqn32::gemm16(dqn32::kConvU8, g, partials, s, "conv1")
              : mfma ? dqn32::conv_mfma<dqn32::kConvU8, 2>(g, s, "conv1")
                     : dqn32::gemm<dqn32::kConvU8>(g, s, "conv1")))
        return rc;
    // conv2: relu(Y1 + b1) -> Y2 [B*P][64]
    g.x = sc.y1; g.xbias = net->conv1_b; g.w = net->conv2_w; g.y = sc.y2;
    g.N = 64; g.K = 9 * 32; g.C = 32;
    if ((rc = bf16   ? dqn32::gemm16(dqn32::kConvF32, g, partials, s, "conv2")
              : mfma ? dqn32::conv_mfma<dqn32::kConvF32, 4>(g, s, "conv2")
                     : dqn32::gemm<dqn32::kConvF32>(g, s, "conv2")))
        return rc;
    // conv3: relu(Y2 + b2) -> Y3
    g.x = sc.y2; g.xbias = net->conv2_b; g.w = net->conv3_w; g.y = sc.y3;
    g.N = 64; g.K = 9 * 64; g.C = 64;
    if ((rc = bf16   ? dqn32::gemm16(dqn32::kConvF32, g, partials, s, "conv3")
              : mfma ? dqn32::conv_mfma<dqn32::kConvF32, 4>(g, s, "conv3")
                     : dqn32::gemm<dqn32::kConvF32>(g, s, "conv3")))
        return rc;
    // fc1: relu(Y3 + b3) flattened NHWC (P*64) -> Y4 [B][256]
    g.x = sc.y3; g.xbias = net->conv3_b; g.bmod = 64; g.w = net->fc1_w; g.y = sc.y4;
    g.M = batch; g.N = 256; g.K = (int)(P * 64);
    if ((rc = bf16 ? dqn32::gemm16(dqn32::kDense, g, partials, s, "fc1") : dqn32::fc_mfma(g, s, "fc1"))) return rc;
    // fc2: relu(Y4 + bfc1) -> Y5 [B][128]
    g.x = sc.y4; g.xbias = net->fc1_b; g.bmod = 256; g.w = net->fc2_w; g.y = sc.y5;
    g.N = 128; g.K = 256;
    if ((rc = bf16 ? dqn32::gemm16(dqn32::kDense, g, partials, s, "fc2") : dqn32::fc_mfma(g, s, "fc2"))) return rc;
    // fc3: relu(Y5 + bfc2) -> q [B][A] + bfc3
    g.x = sc.y5; g.xbias = net->fc2_b; g.bmod = 128; g.w = net->fc3_w; g.y = q_out; g.ybias = net->fc3_b;
    g.N = A; g.K = 128;
    if ((rc = dqn32::gemm<dqn32::kDense>(g, s, "fc3"))) return rc;
    if (feat_out) {
        const int64_t total = batch * 128;
        hipLaunchKernelGGL(dqn32::k_bias_relu, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, sc.y5,
                           net->fc2_b, 128, total, feat_out);
        if ((rc = launch_status("k_bias_relu"))) return rc;
    }
    return SNAKE_OK;
}

extern "C" int snake_dqn32_forward(const snake_dqn_cfg *cfg, const snake_dqn32_net *net, const uint8_t *obs,
                                   int64_t batch, void *scratch, float *q_out, float *feat_out, void *stream)
{
    return forward("snake_dqn32_forward", false, cfg, net, obs, batch, scratch, q_out, feat_out, stream);
}

extern "C" int64_t snake_dqn32_forward_bf16_scratch(const snake_dqn_cfg *cfg, int64_t batch)
{
    const int rc = dqn32::check_cfg(cfg);
    if (rc) return rc;
    if (batch < 0) { set_error("snake_dqn32_forward_bf16_scratch: batch < 0"); return SNAKE_E_ARG; }
    return dqn32::fwd16_scratch_bytes(cfg, batch, nullptr, nullptr, nullptr);
}

extern "C" int snake_dqn32_forward_bf16(const snake_dqn_cfg *cfg, const snake_dqn32_net *net, const uint8_t *obs,
                                        int64_t batch, void *scratch, float *q_out, float *feat_out, void *stream)
{
    return forward("snake_dqn32_forward_bf16", true, cfg, net, obs, batch, scratch, q_out, feat_out, stream);
}
