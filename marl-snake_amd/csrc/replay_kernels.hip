// replay_kernels.hip -- the reference trainer's replay buffer (train_dqn.py:89-100,
// filled at :290-298, sampled at :228-240) as rings in device memory; semantics
// in include/snake_env.h (snake_replay_push, snake_replay_gather).
//
// Every observation byte is 0 or 1 and channels come in groups of 8, so the 8
// channel bytes of one cell and frame are one byte of information: the rings
// hold that byte. A row is P = h*w*fs packed bytes at a 16-byte pitch.
//
// Push, three launches whose grids depend on N only:
//   k_replay_count  one thread per env: the env's stored snakes (S <= 16 skip
//                   bytes), an exclusive scan over the block's 1 024 envs, the
//                   block's total.
//   k_replay_scan   one workgroup: the exclusive scan of the block totals, then
//                   one thread reads `count`, leaves the call's header (the slot
//                   of the first transition kept, how many are dropped because
//                   more than `capacity` arrive at once, the total) and adds
//                   the total to `count`.
//   k_replay_store  G lanes per snake (G the power of two that covers the row
//                   with four packed bytes per lane, 64 / G snakes per wave).
//                   The group's first lane finds the snake's slot -- block
//                   offset + env offset + the stored snakes before it in its
//                   env -- and writes action, reward and done; every lane packs
//                   4 cells of obs and 4 of next_obs (one 8-byte load per cell
//                   and frame, eight in flight) into one 4-byte store each.
// The slot of a transition is a prefix count, never an atomic: the rings'
// contents do not depend on the order in which workgroups run.
//
// Gather, one launch: a capped grid walks the output tensors in 16-byte pieces
// (grid.y: state / next_state), so every store is an aligned, fully coalesced
// dwordx4 whatever the parity of h*w; the ring bytes it expands are 1/8 (uint8)
// or 1/32 (float) of what it writes. (row, position) advance by the grid's
// stride in mixed radix, without a division in the loop.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "snake_internal.h"
#include "snake_device.h"

namespace snake {
namespace replay {

constexpr int kScanBlock = 1024;        // envs per k_replay_count block
constexpr int kMaxSide = 1024;
constexpr int kMaxChannels = 512;
constexpr int kMaxRow = 1 << 20;        // packed bytes of a row
constexpr long long kMaxCapacity = 1ll << 40;
constexpr long long kMaxEnvs = 1ll << 26;
constexpr int kGatherBlocks = 2048;     // per output tensor
enum { HDR_START = 0, HDR_DROP = 1, HDR_TOTAL = 2, HDR_WORDS = 4 };    // int64 words

struct PushArgs {
    const uint8_t *obs, *next_obs;
    const int8_t *actions;
    const double *rewards;
    const uint8_t *done, *skip;     // skip may be NULL
    const int32_t *step;            // may be NULL
    snake_replay_rings r;
    long long *hdr;                 // scratch: the header, the block offsets, the env offsets
    int32_t *blk, *env_off;
    long long capacity;
    uint32_t N, snakes;             // envs, N * S
    int nb;                         // k_replay_count blocks
    int S, P, pitch, gshift;        // G = 1 << gshift lanes per snake
    int ed_steps;
    double ed_pen;
};

struct GatherArgs {
    snake_replay_rings r;
    const long long *idx;
    void *out[2];                   // state, next_state
    long long *action;
    float *reward, *done;
    long long capacity;
    uint32_t B;
    int P, pitch, fs, hw, C;
};

// exclusive scan of v over the workgroup's 1 024 threads; *total: the sum
__device__ __forceinline__ int block_scan(int v, int *total)
{
    __shared__ int wsum[kScanBlock / kWave];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    __syncthreads();                // (a second call: the first one's reads are over)
    if (lane == kWave - 1) wsum[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < kScanBlock / kWave; i++) {
        const int s = wsum[i];
        if (i < wave) before += s;
        all += s;
    }
    *total = all;
    return before + inc - v;
}

__global__ void __launch_bounds__(kScanBlock) k_replay_count(const PushArgs g)
{
    const uint32_t env = blockIdx.x * kScanBlock + threadIdx.x;
    int c = 0;
    if (env < g.N) {
        if (g.skip == nullptr) c = g.S;
        else
            for (int s = 0; s < g.S; s++) c += g.skip[(size_t)env * g.S + s] == 0;
    }
    int total;
    const int off = block_scan(c, &total);
    if (env < g.N) g.env_off[env] = off;
    if (threadIdx.x == 0) g.blk[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kScanBlock) k_replay_scan(const PushArgs g)
{
    const int per = (g.nb + kScanBlock - 1) / kScanBlock;
    const int i0 = threadIdx.x * per, i1 = min(i0 + per, g.nb);
    int s = 0;
    for (int i = i0; i < i1; i++) s += g.blk[i];
    int total;
    int run = block_scan(s, &total);
    for (int i = i0; i < i1; i++) {
        const int t = g.blk[i];
        g.blk[i] = run;
        run += t;
    }
    if (threadIdx.x == 0) {
        const long long count = *g.r.count;
        const long long drop = total > g.capacity ? total - g.capacity : 0;
        g.hdr[HDR_START] = (count + drop) % g.capacity;
        g.hdr[HDR_DROP] = drop;
        g.hdr[HDR_TOTAL] = total;
        *g.r.count = count + total;
    }
}

// 0x80 in every nonzero byte of x (exact per byte: no carry crosses a byte)
__device__ __forceinline__ uint32_t bytes_nonzero(uint32_t x)
{
    return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
}

// the 8 channel bytes of one cell and frame -> bit k = channel k is nonzero
__device__ __forceinline__ uint32_t pack8(uint2 v)
{
    // bits 0, 8, 16, 24 -> bits 24..27 (the partial products never share a bit)
    const uint32_t lo = ((bytes_nonzero(v.x) >> 7) * 0x01020408u) >> 24;
    const uint32_t hi = ((bytes_nonzero(v.y) >> 7) * 0x01020408u) >> 24;
    return (lo & 15u) | (hi & 15u) << 4;
}

// bits 0..3 of b -> 0/1 in bytes 0..3
__device__ __forceinline__ uint32_t unpack4(uint32_t b)
{
    return ((b & 15u) * 0x00204081u) & 0x01010101u;
}

__global__ void __launch_bounds__(256) k_replay_store(const PushArgs g)
{
    const int lane = threadIdx.x & 63;
    const int G = 1 << g.gshift, sub = lane & (G - 1);
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t row = (wave << (6 - g.gshift)) + (uint32_t)(lane >> g.gshift);
    long long slot = -1;
    if (sub == 0 && row < g.snakes && (g.skip == nullptr || g.skip[row] == 0)) {
        const uint32_t env = row / (uint32_t)g.S;
        int rank = (int)(row - env * (uint32_t)g.S);
        if (g.skip != nullptr) {
            int r = 0;
            for (uint32_t j = env * (uint32_t)g.S; j < row; j++) r += g.skip[j] == 0;
            rank = r;
        }
        const long long k = (long long)g.blk[env / kScanBlock] + g.env_off[env] + rank - g.hdr[HDR_DROP];
        if (k >= 0) {       // (else: more than `capacity` arrive at once, and this one is evicted by the same call)
            slot = g.hdr[HDR_START] + k;
            if (slot >= g.capacity) slot -= g.capacity;
            const bool d = g.done[row] != 0;
            double r = g.rewards[row];
            if (d && g.step != nullptr && g.step[env] < g.ed_steps) r += g.ed_pen;
            g.r.action[slot] = g.actions[row];
            g.r.reward[slot] = (float)r;
            g.r.done[slot] = d ? 1 : 0;
        }
    }
    slot = __shfl(slot, lane & ~(G - 1));
    if (slot < 0) return;
    const uint2 *src0 = reinterpret_cast<const uint2 *>(g.obs) + (size_t)row * g.P;
    const uint2 *src1 = reinterpret_cast<const uint2 *>(g.next_obs) + (size_t)row * g.P;
    uint8_t *dst0 = g.r.state + (size_t)slot * g.pitch, *dst1 = g.r.next_state + (size_t)slot * g.pitch;
    for (int p = sub * 4; p < g.P; p += G * 4) {
        uint2 a[4], b[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            a[k] = b[k] = make_uint2(0, 0);
            if (p + k < g.P) {
                a[k] = src0[p + k];
                b[k] = src1[p + k];
            }
        }
        uint32_t wa = 0, wb = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            wa |= pack8(a[k]) << (8 * k);
            wb |= pack8(b[k]) << (8 * k);
        }
        // p + 4 <= pitch: p is a multiple of 4 below P, the pitch a multiple of 16
        *reinterpret_cast<uint32_t *>(dst0 + p) = wa;
        *reinterpret_cast<uint32_t *>(dst1 + p) = wb;
    }
}

// logical index -> slot (head: the slot of the oldest transition)
struct Window {
    long long last, head, capacity;     // last = max(size, 1) - 1
    __device__ __forceinline__ long long slot(long long j) const
    {
        j = j < 0 ? 0 : (j > last ? last : j);
        const long long s = head + j;
        return s >= capacity ? s - capacity : s;
    }
};

__device__ __forceinline__ Window window_of(const GatherArgs &g)
{
    const long long count = *g.r.count;
    Window w;
    w.capacity = g.capacity;
    w.last = (count < g.capacity ? count : g.capacity) - 1;
    if (w.last < 0) w.last = 0;
    w.head = count <= g.capacity ? 0 : count % g.capacity;
    return w;
}

__device__ __forceinline__ void gather_small(const GatherArgs &g, const Window &w)
{
    if (blockIdx.y != 0) return;
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < g.B; b += gridDim.x * blockDim.x) {
        const long long s = w.slot(g.idx[b]);
        g.action[b] = g.r.action[s];
        g.reward[b] = g.r.reward[s];
        g.done[b] = g.r.done[s] ? 1.f : 0.f;
    }
}

// uint8 [B][h][w][C]: a thread's piece is two cells-and-frames (16 bytes)
__global__ void __launch_bounds__(256) k_replay_gather_u8(const GatherArgs g)
{
    const Window w = window_of(g);
    gather_small(g, w);
    const uint8_t *ring = blockIdx.y ? g.r.next_state : g.r.state;
    uint8_t *out = static_cast<uint8_t *>(g.out[blockIdx.y]);
    const uint32_t P = g.P, groups = g.B * P;               // (< 2^31)
    const uint32_t stride = 2u * gridDim.x * blockDim.x, sq = stride / P, sr = stride % P;
    uint32_t t = 2u * (blockIdx.x * blockDim.x + threadIdx.x);
    uint32_t b = t / P, i = t % P;
    for (; t < groups; t += stride) {
        const uint32_t v0 = ring[w.slot(g.idx[b]) * g.pitch + i];
        uint4 o;
        o.x = unpack4(v0);
        o.y = unpack4(v0 >> 4);
        if (t + 1 < groups) {
            const uint32_t b1 = i + 1 == P ? b + 1 : b, i1 = i + 1 == P ? 0 : i + 1;
            const uint32_t v1 = ring[w.slot(g.idx[b1]) * g.pitch + i1];
            o.z = unpack4(v1);
            o.w = unpack4(v1 >> 4);
            *reinterpret_cast<uint4 *>(out + (size_t)t * 8) = o;
        } else {
            *reinterpret_cast<uint2 *>(out + (size_t)t * 8) = make_uint2(o.x, o.y);
        }
        b += sq;
        i += sr;
        if (i >= P) {
            i -= P;
            b++;
        }
    }
}

// float [B][C][h][w]: a thread's piece is four floats; C*h*w is a multiple of 8,
// so a piece never leaves its row
__global__ void __launch_bounds__(256) k_replay_gather_f32(const GatherArgs g)
{
    const Window w = window_of(g);
    gather_small(g, w);
    const uint8_t *ring = blockIdx.y ? g.r.next_state : g.r.state;
    float *out = static_cast<float *>(g.out[blockIdx.y]);
    const uint32_t hw = g.hw, C = g.C, rowlen = C * hw, quads = g.B * (rowlen / 4);   // (< 2^31)
    const uint32_t stride = gridDim.x * blockDim.x;
    // the stride in floats as (rows, channels, cells)
    const uint64_t se = (uint64_t)stride * 4;
    const uint32_t sb = (uint32_t)(se / rowlen), srem = (uint32_t)(se % rowlen), sc = srem / hw, scell = srem % hw;
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t b = t / (rowlen / 4), v = (t % (rowlen / 4)) * 4, c = v / hw, cell = v % hw;
    for (; t < quads; t += stride) {
        const uint8_t *row = ring + w.slot(g.idx[b]) * g.pitch;
        float f[4];
        uint32_t ck = c, cellk = cell;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            f[k] = (float)((row[cellk * g.fs + (ck >> 3)] >> (ck & 7)) & 1);
            if (++cellk == hw) {
                cellk = 0;
                ck++;
            }
        }
        *reinterpret_cast<float4 *>(out + ((size_t)b * rowlen + (size_t)c * hw + cell)) =
            make_float4(f[0], f[1], f[2], f[3]);
        cell += scell;
        if (cell >= hw) {
            cell -= hw;
            c++;
        }
        c += sc;
        if (c >= C) {
            c -= C;
            b++;
        }
        b += sb;
    }
}

int check_cfg(const snake_replay_cfg *c)
{
    if (!c) { set_error("snake_replay: cfg is NULL"); return SNAKE_E_CONFIG; }
    if (c->obs_h < 1 || c->obs_h > kMaxSide || c->obs_w < 1 || c->obs_w > kMaxSide) {
        set_error("snake_replay: obs_h and obs_w must be in [1, %d] (got %d x %d)", kMaxSide, c->obs_h, c->obs_w);
        return SNAKE_E_CONFIG;
    }
    if (c->obs_c < 8 || c->obs_c > kMaxChannels || c->obs_c % 8) {
        set_error("snake_replay: obs_c must be a multiple of 8 in [8, %d] (got %d)", kMaxChannels, c->obs_c);
        return SNAKE_E_CONFIG;
    }
    if ((long long)c->obs_h * c->obs_w * (c->obs_c / 8) > kMaxRow) {
        set_error("snake_replay: obs_h * obs_w * obs_c / 8 must be at most %d", kMaxRow);
        return SNAKE_E_CONFIG;
    }
    if (c->num_snakes < 1 || c->num_snakes > kMaxSnakes) {
        set_error("snake_replay: num_snakes must be in [1, %d] (got %d)", kMaxSnakes, c->num_snakes);
        return SNAKE_E_CONFIG;
    }
    if (c->capacity < 1 || c->capacity > kMaxCapacity) {
        set_error("snake_replay: capacity must be in [1, 2^40] (got %lld)", (long long)c->capacity);
        return SNAKE_E_CONFIG;
    }
    if (!(c->early_death_penalty == c->early_death_penalty)) {
        set_error("snake_replay: early_death_penalty is NaN");
        return SNAKE_E_CONFIG;
    }
    return SNAKE_OK;
}

int check_envs(const char *who, int64_t num_envs)
{
    if (num_envs < 0 || num_envs > kMaxEnvs) {
        set_error("%s: num_envs must be in [0, 2^26] (got %lld)", who, (long long)num_envs);
        return SNAKE_E_ARG;
    }
    return SNAKE_OK;
}

inline int packed_row(const snake_replay_cfg *c) { return c->obs_h * c->obs_w * (c->obs_c / 8); }
inline int pitch_of(int P) { return (P + 15) / 16 * 16; }
inline int64_t scan_blocks(int64_t N) { return (N + kScanBlock - 1) / kScanBlock; }
// scratch: the header, the block offsets (a multiple of four words), the env offsets
inline int64_t blk_words(int64_t N) { return (scan_blocks(N) + 3) / 4 * 4; }

}  // namespace replay
}  // namespace snake

using namespace snake;

extern "C" int snake_replay_plan(const snake_replay_cfg *cfg, int64_t num_envs, snake_replay_layout *out)
{
    if (int rc = replay::check_cfg(cfg)) return rc;
    if (int rc = replay::check_envs("snake_replay_plan", num_envs)) return rc;
    if (!out) { set_error("snake_replay_plan: out is NULL"); return SNAKE_E_ARG; }
    const int P = replay::packed_row(cfg), pitch = replay::pitch_of(P);
    out->packed_row = P;
    out->pitch = pitch;
    out->state = out->next_state = cfg->capacity * pitch;
    out->action = cfg->capacity;
    out->reward = cfg->capacity * 4;
    out->done = cfg->capacity;
    out->count = 8;
    out->scratch = replay::HDR_WORDS * 8 + replay::blk_words(num_envs) * 4 + (num_envs + 3) / 4 * 16;
    return SNAKE_OK;
}

extern "C" int snake_replay_push(const snake_replay_cfg *cfg, const snake_replay_rings *rings, const uint8_t *obs,
                                 const uint8_t *next_obs, const int8_t *actions, const double *rewards,
                                 const uint8_t *done, const uint8_t *skip, const int32_t *step, int64_t num_envs,
                                 void *scratch, void *stream)
{
    if (int rc = replay::check_cfg(cfg)) return rc;
    if (int rc = replay::check_envs("snake_replay_push", num_envs)) return rc;
    if (!rings || !rings->state || !rings->next_state || !rings->action || !rings->reward || !rings->done ||
        !rings->count) {
        set_error("snake_replay_push: NULL ring buffer");
        return SNAKE_E_ARG;
    }
    if (num_envs == 0) return SNAKE_OK;
    if (!obs || !next_obs || !actions || !rewards || !done || !scratch) {
        set_error("snake_replay_push: NULL buffer");
        return SNAKE_E_ARG;
    }
    if (((uintptr_t)obs | (uintptr_t)next_obs | (uintptr_t)rewards | (uintptr_t)scratch) & 7) {
        set_error("snake_replay_push: obs, next_obs, rewards and scratch must be 8-byte aligned");
        return SNAKE_E_ARG;
    }
    if (((uintptr_t)rings->state | (uintptr_t)rings->next_state) & 15) {
        set_error("snake_replay_push: the state rings must be 16-byte aligned");
        return SNAKE_E_ARG;
    }
    replay::PushArgs g;
    g.obs = obs;
    g.next_obs = next_obs;
    g.actions = actions;
    g.rewards = rewards;
    g.done = done;
    g.skip = skip;
    g.step = step;
    g.r = *rings;
    g.hdr = static_cast<long long *>(scratch);
    g.blk = reinterpret_cast<int32_t *>(g.hdr + replay::HDR_WORDS);
    g.env_off = g.blk + replay::blk_words(num_envs);
    g.capacity = cfg->capacity;
    g.N = (uint32_t)num_envs;
    g.snakes = (uint32_t)(num_envs * cfg->num_snakes);
    g.nb = (int)replay::scan_blocks(num_envs);
    g.S = cfg->num_snakes;
    g.P = replay::packed_row(cfg);
    g.pitch = replay::pitch_of(g.P);
    g.gshift = 0;
    while (g.gshift < 6 && (4 << g.gshift) < g.P) g.gshift++;
    g.ed_steps = cfg->early_death_steps;
    g.ed_pen = cfg->early_death_penalty;
    const hipStream_t s = (hipStream_t)stream;
    DeviceGuard dg(s);
    if (dg.dev < 0) return SNAKE_E_LAUNCH;
    hipLaunchKernelGGL(replay::k_replay_count, dim3((unsigned)g.nb), dim3(replay::kScanBlock), 0, s, g);
    if (int rc = launch_status("k_replay_count")) return rc;
    hipLaunchKernelGGL(replay::k_replay_scan, dim3(1), dim3(replay::kScanBlock), 0, s, g);
    if (int rc = launch_status("k_replay_scan")) return rc;
    const uint32_t rows_per_block = 4u << (6 - g.gshift);
    const uint32_t blocks = (g.snakes + rows_per_block - 1) / rows_per_block;
    hipLaunchKernelGGL(replay::k_replay_store, dim3(blocks), dim3(256), 0, s, g);
    return launch_status("k_replay_store");
}

extern "C" int snake_replay_gather(const snake_replay_cfg *cfg, const snake_replay_rings *rings, const int64_t *idx,
                                   int64_t batch, int32_t format, void *state, void *next_state, int64_t *action,
                                   float *reward, float *done, void *stream)
{
    if (int rc = replay::check_cfg(cfg)) return rc;
    if (format != SNAKE_REPLAY_U8_NHWC && format != SNAKE_REPLAY_F32_NCHW) {
        set_error("snake_replay_gather: format must be 0 (uint8 NHWC) or 1 (float NCHW) (got %d)", format);
        return SNAKE_E_ARG;
    }
    const int P = replay::packed_row(cfg);
    // 16-byte pieces of one output tensor stay below 2^31 in both formats
    if (batch < 0 || batch > (1ll << 30) || batch * P >= (1ll << 30)) {
        set_error("snake_replay_gather: batch * h*w*obs_c/8 must be in [0, 2^30) (batch %lld)", (long long)batch);
        return SNAKE_E_ARG;
    }
    if (batch == 0) return SNAKE_OK;
    if (!rings || !rings->state || !rings->next_state || !rings->action || !rings->reward || !rings->done ||
        !rings->count || !idx || !state || !next_state || !action || !reward || !done) {
        set_error("snake_replay_gather: NULL buffer");
        return SNAKE_E_ARG;
    }
    if (((uintptr_t)state | (uintptr_t)next_state) & 15) {
        set_error("snake_replay_gather: state and next_state must be 16-byte aligned");
        return SNAKE_E_ARG;
    }
    replay::GatherArgs g;
    g.r = *rings;
    g.idx = reinterpret_cast<const long long *>(idx);
    g.out[0] = state;
    g.out[1] = next_state;
    g.action = reinterpret_cast<long long *>(action);
    g.reward = reward;
    g.done = done;
    g.capacity = cfg->capacity;
    g.B = (uint32_t)batch;
    g.P = P;
    g.pitch = replay::pitch_of(P);
    g.fs = cfg->obs_c / 8;
    g.hw = cfg->obs_h * cfg->obs_w;
    g.C = cfg->obs_c;
    // 16-byte pieces per output tensor (at least one thread per row, for the small outputs)
    int64_t pieces = format == SNAKE_REPLAY_U8_NHWC ? (batch * P + 1) / 2 : batch * P * 2;
    if (pieces < batch) pieces = batch;
    int64_t blocks = (pieces + 255) / 256;
    if (blocks > replay::kGatherBlocks) blocks = replay::kGatherBlocks;
    const hipStream_t s = (hipStream_t)stream;
    DeviceGuard dg(s);
    if (dg.dev < 0) return SNAKE_E_LAUNCH;
    if (format == SNAKE_REPLAY_U8_NHWC) {
        hipLaunchKernelGGL(replay::k_replay_gather_u8, dim3((unsigned)blocks, 2), dim3(256), 0, s, g);
        return launch_status("k_replay_gather_u8");
    }
    hipLaunchKernelGGL(replay::k_replay_gather_f32, dim3((unsigned)blocks, 2), dim3(256), 0, s, g);
    return launch_status("k_replay_gather_f32");
}
