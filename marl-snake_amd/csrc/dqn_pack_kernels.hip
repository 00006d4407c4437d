// dqn_pack_kernels.hip -- the learner's fp32 master weights (snake_dqn32_net,
// the layouts of dqn32_kernels.hip) converted into the bf16 forward's layouts
// (snake_dqn_layout, dqn_kernels.hip) on the device: stream-ordered, no host
// sync, no allocation, so that a training loop can act and form its targets on
// the bf16 matrix cores with the weights it is training.
//
//   conv1..3  fp32 [out][(ky*3 + kx)*cin + ci] -> bf16 [out][k = tap*cpad + ci]
//             in MFMA fragment order, zero where ci >= cin or k >= 9*cpad
//   fc1       fp32 [256][p*64 + ch] -> bf16 [256][64*p16] in conv3's fragment
//             order (GEMM row i = position rows[i]; zero where that is -1)
//   fc2       fp32 [128][256] -> bf16 [128][256]
//   the five biases, fc3's weights and bias: copied as fp32
//
// Every element of every destination is written on every call.
//
// One kernel, k_dqn_pack, one launch, work items by workgroup range:
//   workgroups [0, fc1_blocks)  four waves, each one (n, m) tile of fc1: 16
//       positions x 64 channels = 1 024 bf16 that lie contiguously (2 KB) in the
//       destination. The wave reads the sixteen 256-byte source rows with four
//       16-byte loads per lane (lane = (quad, four channels), load r = position
//       4*quad + r), so a lane holds r = 0..3 of four channels: four bf16 that
//       are adjacent in the destination. It writes them as 8-byte words into
//       the wave's own 2 KB of LDS at their destination offset and reads the
//       image back 16 bytes per lane for two 1 KB stores to consecutive
//       addresses. The 16-byte slots of the image are XOR-swizzled (lds_slot):
//       unswizzled, the 16 lanes of an 8-byte store group hit two slots of
//       every 128 bytes, a 4-way bank conflict; the swizzle permutes only
//       within aligned groups of four slots, which keeps the 16-byte reads
//       conflict-free.
//   the workgroups after them   one thread per 16-byte destination chunk of the
//       conv weights and fc2 (eight consecutive k of a fragment are eight
//       consecutive source channels: two 16-byte loads, one 16-byte store),
//       then one thread per element of the fp32 copies.
// No atomics; plain vector loads and stores only.
//
// The index mappings (conv_chunk_src, fc1_dst) and the rounding (bf16_rne) are
// __host__ __device__ and shared with snake_dqn_pack32_host, the same
// conversion as plain loops over host memory (tests/test_dqn_pack_cpu.py).
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include "snake_internal.h"
#include "snake_device.h"

namespace snake {
namespace pack {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Round to nearest even on the bit pattern (dqn_kernels.hip bf16_bits: equal
// to torch's .to(bfloat16) on everything that is not a NaN); a NaN keeps its
// sign and top mantissa bits and gets the quiet bit, so it stays a NaN.
__host__ __device__ inline uint32_t bf16_rne(float x)
{
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// Chunk q (8 bf16, 16 bytes) of a conv weight B[out][K] in fragment order holds
// k0 .. k0 + 7 of one output channel: element (o, k) sits at ((o/16 * K/32 +
// k/32) * 4 + (k%32)/8) * 128 + (o%16) * 8 + k%8. Returns the index of the
// first of its eight source floats in [out][(tap, ci)] (cpad and cin are
// multiples of 8, so the eight are one tap's consecutive channels), or -1 for
// a chunk of zeros (ci >= cin: channel padding; tap >= 9: k padding).
__host__ __device__ inline int conv_chunk_src(int q, int K, int cpad, int cin)
{
    const int o16 = q % 16, k8 = (q / 16) % 4, blk = q / 64;
    const int o = blk / (K / 32) * 16 + o16, k = blk % (K / 32) * 32 + k8 * 8;
    const int tap = k / cpad, ci = k % cpad;
    return tap < 9 && ci < cin ? (o * 9 + tap) * cin + ci : -1;
}

// fc1: the offset inside an (n, m) tile of 1 024 bf16 of GEMM row i (0..15) and
// channel ch (snake_dqn_layout.fc1_w: half*512 + quad*128 + c16*8 + j*4 + r
// with i = 4*quad + r, ch = (2*half + j)*16 + c16).
__host__ __device__ inline int fc1_dst(int i, int ch)
{
    return (ch / 32) * 512 + (i / 4) * 128 + (ch % 16) * 8 + ((ch / 16) % 2) * 4 + i % 4;
}

// The position of GEMM row i of row tile m: -1 (zero weights) for a padding row
// and for anything that is not a position of the map.
__host__ __device__ inline int fc1_pos(const int32_t *rows, int m, int i, int P)
{
    const int p = rows[m * 16 + i];
    return (uint32_t)p < (uint32_t)P ? p : -1;
}

// 16-byte slot of chunk u in a wave's LDS image (see the header)
__device__ __forceinline__ int lds_slot(int u) { return u ^ ((u >> 3) & 1) ^ (((u >> 6) & 1) << 1); }

constexpr int kCopies = 7;      // conv1_b conv2_b conv3_b fc1_b fc2_b fc3_w fc3_b

struct PackArgs {
    const float *conv[3], *fc1, *fc2;   // fp32 sources
    uint16_t *dconv[3], *dfc1, *dfc2;   // bf16 destinations
    const float *csrc[kCopies];
    float *cdst[kCopies];
    int cnum[kCopies];
    const int32_t *rows;
    int P, MT;                  // positions h*w, row tiles p16/16
    int K[3], cpad[3], cin[3];  // the convs' K, padded and real input channels
    int fc1_blocks;             // workgroups of four fc1 tiles
    int end_conv[3], end_fc2;   // ends of the chunk ranges of the small tensors
};

__device__ __forceinline__ void chunk_store(uint16_t *dst, int q, const float *src)
{
    u32x4 w = {0u, 0u, 0u, 0u};
    if (src) {
        const f32x4 a = *(const f32x4 *)src, b = *(const f32x4 *)(src + 4);
        w[0] = bf16_rne(a[0]) | bf16_rne(a[1]) << 16;
        w[1] = bf16_rne(a[2]) | bf16_rne(a[3]) << 16;
        w[2] = bf16_rne(b[0]) | bf16_rne(b[1]) << 16;
        w[3] = bf16_rne(b[2]) | bf16_rne(b[3]) << 16;
    }
    *(u32x4 *)(dst + (size_t)q * 8) = w;
}

__global__ void __launch_bounds__(256) k_dqn_pack(const PackArgs a)
{
    __shared__ u32x4 image[4][128];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < a.fc1_blocks) {
        const int wave = tid >> 6, lane = tid & 63;
        const int tile = blockIdx.x * 4 + wave;         // 256 * MT tiles: a multiple of four
        const int n = tile / a.MT, m = tile - n * a.MT;
        const int quad = lane >> 4, c4 = lane & 15;
        const float *row = a.fc1 + (size_t)n * 64 * a.P + 4 * c4;
        f32x4 v[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int p = fc1_pos(a.rows, m, 4 * quad + r, a.P);
            v[r] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (p >= 0) v[r] = *(const f32x4 *)(row + (size_t)p * 64);
        }
        u32x2 *img2 = (u32x2 *)image[wave];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int t = fc1_dst(4 * quad, 4 * c4 + e);        // r = 0: a multiple of four
            u32x2 w;
            w[0] = bf16_rne(v[0][e]) | bf16_rne(v[1][e]) << 16;
            w[1] = bf16_rne(v[2][e]) | bf16_rne(v[3][e]) << 16;
            img2[lds_slot(t >> 3) * 2 + ((t >> 2) & 1)] = w;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        u32x4 *out = (u32x4 *)a.dfc1 + (size_t)tile * 128;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int u = lane + 64 * h;
            out[u] = image[wave][lds_slot(u)];
        }
        return;
    }
    int g = ((int)blockIdx.x - a.fc1_blocks) * 256 + tid;
    if (g < a.end_fc2) {
#pragma unroll
        for (int t = 0; t < 3; t++) {
            const int q = g - (t ? a.end_conv[t - 1] : 0);
            if (g < a.end_conv[t]) {
                const int s = conv_chunk_src(q, a.K[t], a.cpad[t], a.cin[t]);
                chunk_store(a.dconv[t], q, s >= 0 ? a.conv[t] + s : nullptr);
                return;
            }
        }
        const int q = g - a.end_conv[2];
        chunk_store(a.dfc2, q, a.fc2 + (size_t)q * 8);
        return;
    }
    g -= a.end_fc2;
#pragma unroll
    for (int t = 0; t < kCopies; t++) {
        if (g < a.cnum[t]) {
            a.cdst[t][g] = a.csrc[t][g];
            return;
        }
        g -= a.cnum[t];
    }
}

}  // namespace pack
}  // namespace snake

using namespace snake;
using namespace snake::pack;

namespace {

// The plan's checks and the argument checks both entry points share; fills the
// sizes and pointers of PackArgs (no launch geometry).
int pack_args(const char *who, const snake_dqn_cfg *cfg, int32_t map_plan, const snake_dqn32_net *src,
              const snake_dqn_net *dst, const int32_t *rows, bool device, PackArgs *a)
{
    if (!cfg) { set_error("%s: NULL argument", who); return SNAKE_E_ARG; }
    if (map_plan != 0 && map_plan != 1) { set_error("%s: map_plan must be 0 or 1 (got %d)", who, map_plan); return SNAKE_E_ARG; }
    snake_dqn_layout lay;
    const int rc = map_plan ? snake_dqn_map_plan(cfg, &lay) : snake_dqn_plan(cfg, &lay);
    if (rc) return rc;
    if (!src || !dst || !rows) { set_error("%s: NULL argument", who); return SNAKE_E_ARG; }
    const int A = cfg->num_actions;
    const void *sp[12] = {src->conv1_w, src->conv2_w, src->conv3_w, src->fc1_w, src->fc2_w, src->conv1_b, src->conv2_b,
                          src->conv3_b, src->fc1_b, src->fc2_b, src->fc3_w, src->fc3_b};
    const void *dp[12] = {dst->conv1_w, dst->conv2_w, dst->conv3_w, dst->fc1_w, dst->fc2_w, dst->conv1_b, dst->conv2_b,
                          dst->conv3_b, dst->fc1_b, dst->fc2_b, dst->fc3_w, dst->fc3_b};
    for (int i = 0; i < 12; i++) {
        if (!sp[i] || !dp[i]) { set_error("%s: NULL buffer", who); return SNAKE_E_ARG; }
        // the kernel moves the five weight tensors 16 bytes at a time
        if (device && i < 5 && (((uintptr_t)sp[i] | (uintptr_t)dp[i]) & 15)) {
            set_error("%s: the weight tensors must be 16-byte aligned", who);
            return SNAKE_E_ARG;
        }
    }
    for (int i = 0; i < 3; i++) {
        a->conv[i] = (const float *)sp[i];
        a->dconv[i] = (uint16_t *)dp[i];
    }
    a->fc1 = src->fc1_w; a->fc2 = src->fc2_w;
    a->dfc1 = (uint16_t *)dst->fc1_w; a->dfc2 = (uint16_t *)dst->fc2_w;
    const int cnum[kCopies] = {32, 64, 64, 256, 128, A * 128, A};
    for (int i = 0; i < kCopies; i++) {
        a->csrc[i] = (const float *)sp[5 + i];
        a->cdst[i] = (float *)dp[5 + i];
        a->cnum[i] = cnum[i];
    }
    a->rows = rows;
    a->P = cfg->height * cfg->width;
    a->MT = lay.p16 / 16;
    a->K[0] = lay.k1; a->K[1] = 288; a->K[2] = 576;
    a->cpad[0] = lay.cpad; a->cpad[1] = 32; a->cpad[2] = 64;
    a->cin[0] = cfg->channels; a->cin[1] = 32; a->cin[2] = 64;
    a->fc1_blocks = 256 * a->MT / 4;
    a->end_conv[0] = 32 * lay.k1 / 8;
    a->end_conv[1] = a->end_conv[0] + 64 * 288 / 8;
    a->end_conv[2] = a->end_conv[1] + 64 * 576 / 8;
    a->end_fc2 = a->end_conv[2] + 128 * 256 / 8;
    return SNAKE_OK;
}

}  // namespace

extern "C" int snake_dqn_pack32(const snake_dqn_cfg *cfg, int32_t map_plan, const snake_dqn32_net *src,
                                const snake_dqn_net *dst, const int32_t *rows, void *stream)
{
    PackArgs a;
    const int rc = pack_args("snake_dqn_pack32", cfg, map_plan, src, dst, rows, true, &a);
    if (rc) return rc;
    int small = a.end_fc2;
    for (int i = 0; i < kCopies; i++) small += a.cnum[i];
    const unsigned grid = (unsigned)(a.fc1_blocks + (small + 255) / 256);
    DeviceGuard dg((hipStream_t)stream);
    if (dg.dev < 0) return SNAKE_E_LAUNCH;
    hipLaunchKernelGGL(k_dqn_pack, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("k_dqn_pack");
}

extern "C" int snake_dqn_pack32_host(const snake_dqn_cfg *cfg, int32_t map_plan, const snake_dqn32_net *src,
                                     const snake_dqn_net *dst, const int32_t *rows)
{
    PackArgs a;
    const int rc = pack_args("snake_dqn_pack32_host", cfg, map_plan, src, dst, rows, false, &a);
    if (rc) return rc;
    for (int t = 0; t < 3; t++) {
        const int chunks = a.end_conv[t] - (t ? a.end_conv[t - 1] : 0);
        for (int q = 0; q < chunks; q++) {
            const int s = conv_chunk_src(q, a.K[t], a.cpad[t], a.cin[t]);
            for (int e = 0; e < 8; e++) a.dconv[t][(size_t)q * 8 + e] = s >= 0 ? (uint16_t)bf16_rne(a.conv[t][s + e]) : 0;
        }
    }
    for (int n = 0; n < 256; n++) {
        for (int m = 0; m < a.MT; m++) {
            uint16_t *tile = a.dfc1 + ((size_t)n * a.MT + m) * 1024;
            for (int i = 0; i < 16; i++) {
                const int p = fc1_pos(rows, m, i, a.P);
                const float *s = a.fc1 + ((size_t)n * a.P + (p >= 0 ? p : 0)) * 64;
                for (int ch = 0; ch < 64; ch++) tile[fc1_dst(i, ch)] = p >= 0 ? (uint16_t)bf16_rne(s[ch]) : 0;
            }
        }
    }
    for (int i = 0; i < 128 * 256; i++) a.dfc2[i] = (uint16_t)bf16_rne(a.fc2[i]);
    for (int t = 0; t < kCopies; t++) memcpy(a.cdst[t], a.csrc[t], sizeof(float) * (size_t)a.cnum[t]);
    return SNAKE_OK;
}
