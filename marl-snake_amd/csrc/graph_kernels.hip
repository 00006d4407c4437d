// graph_kernels.hip -- the graph observation of the reference's SnakeGraph-v1
// (graph_snake_env.py:47-103 GraphSnakeEnv._process_obs): five ray-cast feature
// vectors per snake, from the step's observation tensor and the snake records;
// semantics in include/snake_env.h (snake_graph_obs).
//
// k_graph_obs: one lane per (snake, ray, channel pair), the flat lane index
// t = ((env * S + snake) * 5 + ray) * C/2 + pair. The lane walks its ray, reads
// its two channel bytes and the wall byte (channel 0) of every cell and keeps
// two float64 sums; it stores them as one 16-byte word at out + 16 t, so a
// wave's store is 1 KiB of consecutive addresses whatever C is. The
// C/2 lanes of a ray read the same cells, the walks of one ray are identical:
// divergence is between rays only, and bounded by the n steps.
//
// The steps are taken kChunk at a time: the loads of a chunk's cells are all
// issued before the first is used (a cell outside the observation reads cell 0
// instead and is not used), then the sums are taken in order up to the wall.
// With kChunk = 5 the full-map rule (n = 5) and vision ranges up to 5 do not
// wait for memory once per step; cells behind a wall are read and not used.
//
// The weights come in the kernel's arguments (2 x 127 doubles at most, built on
// the host in the arithmetic the reference uses): the step index is the same
// on every lane, so a weight is a scalar load from the constant cache.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "snake_internal.h"
#include "snake_device.h"

#ifndef SNAKE_GRAPH_CHUNK
#define SNAKE_GRAPH_CHUNK 5
#endif

namespace snake {
namespace graph {

constexpr int kRays = 5;
constexpr int kMaxSteps = 127;      // vision_range limit: the weight table rides in the kernel arguments
constexpr int kMaxSide = 255;       // a head's row and column are bytes of the snake record
constexpr int kMaxChannels = 128;
constexpr int kFullMapSteps = 5;    // graph_snake_env.py:56
constexpr int kBlock = 256;
constexpr long long kMaxLanes = 1ll << 31;      // lanes of one launch (32 GiB of float64 output)
constexpr int kChunk = SNAKE_GRAPH_CHUNK;

struct Args {
    const uint8_t *obs;
    const int32_t *rec;     // snake records, int32 [N][S][4]
    void *out;
    long long lanes;        // N * S * 5 * C/2
    int S, h, w, C, pairs, n, vr, reference, f32;
    double wt[2][kMaxSteps];    // [0]: rays 0-2, [1]: the diagonals; n of each used
};

__global__ void __launch_bounds__(kBlock) k_graph_obs(const Args g)
{
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= g.lanes) return;
    const int per_snake = kRays * g.pairs;
    const int snake = (int)(t / per_snake);             // env * S + s, below 2^30
    const int rem = (int)(t - (long long)snake * per_snake);
    const int ray = rem / g.pairs, p = rem - ray * g.pairs;
    const int env = snake / g.S, s = snake - env * g.S;
    const int2 rec = *reinterpret_cast<const int2 *>(g.rec + (long long)snake * 4);
    double a = 0.0, b = 0.0;
    if ((rec.y >> 8) & 1) {
        int slot = s;
        if (g.reference) {      // the reference's counter of live snakes
            slot = 0;
            for (int j = 0; j < s; j++) slot += (g.rec[((long long)env * g.S + j) * 4 + 1] >> 8) & 1;
        }
        const int h = g.h, w = g.w, C = g.C;
        const uint8_t *o = g.obs + ((long long)env * g.S + slot) * h * w * C;
        const int r0 = g.vr ? g.vr : rec.x & 255, c0 = g.vr ? g.vr : (rec.x >> 8) & 255;
        const int d = rec.y & 3;
        const int dr = d == 0 ? -1 : d == 2 ? 1 : 0, dc = d == 1 ? 1 : d == 3 ? -1 : 0;
        // F = (dr, dc), L = (-dc, dr), R = (dc, -dr), F + L, F + R
        const int sr = ray == 0 ? dr : ray == 1 ? -dc : ray == 2 ? dc : ray == 3 ? dr - dc : dr + dc;
        const int sc = ray == 0 ? dc : ray == 1 ? dr : ray == 2 ? -dr : ray == 3 ? dc + dr : dc - dr;
        const bool diag = ray >= 3;
        bool going = true;
        for (int i0 = 0; i0 < g.n && going; i0 += kChunk) {
            uint32_t v[kChunk];     // the wall byte | the lane's two channel bytes << 8
            bool in[kChunk];
#pragma unroll
            for (int j = 0; j < kChunk; j++) {
                const int i = i0 + j, r = r0 + (i + 1) * sr, c = c0 + (i + 1) * sc;
                in[j] = i < g.n && (unsigned)r < (unsigned)h && (unsigned)c < (unsigned)w;
                // (no branch around the loads, which would wait for each in turn: a
                // cell that is not inside reads cell 0 of the observation, unused)
                const uint8_t *cell = o + (in[j] ? (r * w + c) * C : 0);
                v[j] = cell[0] | (uint32_t) * reinterpret_cast<const uint16_t *>(cell + 2 * p) << 8;
            }
#pragma unroll
            for (int j = 0; j < kChunk; j++) {
                if (!going) break;
                if (!in[j]) {       // outside the observation (or past step n): the ray ends
                    going = false;
                    break;
                }
                const int i = i0 + j;
                const double wa = g.wt[0][i], wd = g.wt[1][i];
                const double wi = diag ? wd : wa;
                if (((v[j] >> 8) & 255) == 1) a += wi;
                if ((v[j] >> 16) == 1) b += wi;
                if ((v[j] & 255) == 1) going = false;       // the wall cell is counted
            }
        }
    }
    if (g.f32) reinterpret_cast<float2 *>(g.out)[t] = make_float2((float)a, (float)b);
    else reinterpret_cast<double2 *>(g.out)[t] = make_double2(a, b);
}

int check_cfg(const snake_graph_cfg *c)
{
    if (!c) { set_error("snake_graph: cfg is NULL"); return SNAKE_E_CONFIG; }
    if (c->obs_c < 8 || c->obs_c > kMaxChannels || c->obs_c % 8) {
        set_error("snake_graph: obs_c must be a multiple of 8 in [8, %d] (got %d)", kMaxChannels, c->obs_c);
        return SNAKE_E_CONFIG;
    }
    if (c->num_snakes < 1 || c->num_snakes > kMaxSnakes) {
        set_error("snake_graph: num_snakes must be in [1, %d] (got %d)", kMaxSnakes, c->num_snakes);
        return SNAKE_E_CONFIG;
    }
    if (c->vision_range < 0 || c->vision_range > kMaxSteps) {
        set_error("snake_graph: vision_range must be in [0, %d] (got %d)", kMaxSteps, c->vision_range);
        return SNAKE_E_CONFIG;
    }
    if (c->obs_h < 1 || c->obs_h > kMaxSide || c->obs_w < 1 || c->obs_w > kMaxSide) {
        set_error("snake_graph: obs_h and obs_w must be in [1, %d] (got %d x %d)", kMaxSide, c->obs_h, c->obs_w);
        return SNAKE_E_CONFIG;
    }
    const int win = 2 * c->vision_range + 1;
    if (c->vision_range > 0 && (c->obs_h != win || c->obs_w != win)) {
        set_error("snake_graph: with vision_range %d obs_h and obs_w must be %d (got %d x %d)", c->vision_range, win,
                  c->obs_h, c->obs_w);
        return SNAKE_E_CONFIG;
    }
    if (c->source != 0 && c->source != 1) {
        set_error("snake_graph: source must be 0 (own) or 1 (reference) (got %d)", c->source);
        return SNAKE_E_CONFIG;
    }
    if (c->out_f32 != 0 && c->out_f32 != 1) {
        set_error("snake_graph: out_f32 must be 0 or 1 (got %d)", c->out_f32);
        return SNAKE_E_CONFIG;
    }
    return SNAKE_OK;
}

inline int steps_of(const snake_graph_cfg *c) { return c->vision_range ? c->vision_range : kFullMapSteps; }

// wt[0][i] = 1 / (i + 1), wt[1][i] = 1 / ((i + 1) * sqrt(2)). With a window the
// reference's observation is float64 and so is the quotient; its full-map
// observation is float32, where numpy takes the quotient in float32 (the
// divisor rounded to float32 first) and the sum widens it.
void fill_weights(int n, bool float32_quotient, double *axis, double *diag)
{
    const double sqrt2 = sqrt(2.0);
    for (int i = 0; i < n; i++) {
        const double da = (double)(i + 1), dd = (double)(i + 1) * sqrt2;
        if (float32_quotient) {
            axis[i] = (double)(1.0f / (float)da);
            diag[i] = (double)(1.0f / (float)dd);
        } else {
            axis[i] = 1.0 / da;
            diag[i] = 1.0 / dd;
        }
    }
}

}  // namespace graph
}  // namespace snake

using namespace snake;

extern "C" int snake_graph_plan(const snake_graph_cfg *cfg) { return graph::check_cfg(cfg); }

extern "C" int snake_graph_weights(int32_t steps, int32_t float32_quotient, double *host_out)
{
    if (steps < 1 || steps > graph::kMaxSteps || !host_out) {
        set_error("snake_graph_weights: steps must be in [1, %d] (got %d) and host_out not NULL", graph::kMaxSteps,
                  steps);
        return SNAKE_E_ARG;
    }
    graph::fill_weights(steps, float32_quotient != 0, host_out, host_out + steps);
    return SNAKE_OK;
}

extern "C" int snake_graph_obs(const snake_graph_cfg *cfg, const uint8_t *obs, const int32_t *snake_records,
                               void *out, int64_t num_envs, void *stream)
{
    if (int rc = graph::check_cfg(cfg)) return rc;
    if (!obs || !snake_records || !out) { set_error("snake_graph_obs: NULL buffer"); return SNAKE_E_ARG; }
    if (((uintptr_t)obs & 7) || ((uintptr_t)snake_records & 15) || ((uintptr_t)out & 15)) {
        set_error("snake_graph_obs: obs must be 8-byte aligned, snake_records and out 16-byte aligned");
        return SNAKE_E_ARG;
    }
    if (num_envs < 0 || num_envs > (1ll << 26)) {
        set_error("snake_graph_obs: num_envs must be in [0, 2^26] (got %lld)", (long long)num_envs);
        return SNAKE_E_ARG;
    }
    if (num_envs == 0) return SNAKE_OK;
    graph::Args g;
    g.obs = obs;
    g.rec = snake_records;
    g.out = out;
    g.S = cfg->num_snakes;
    g.h = cfg->obs_h;
    g.w = cfg->obs_w;
    g.C = cfg->obs_c;
    g.pairs = g.C / 2;
    g.n = graph::steps_of(cfg);
    g.vr = cfg->vision_range;
    g.reference = cfg->source;
    g.f32 = cfg->out_f32;
    g.lanes = (long long)num_envs * g.S * graph::kRays * g.pairs;
    if (g.lanes > graph::kMaxLanes) {
        set_error("snake_graph_obs: num_envs * num_snakes * 5 * obs_c / 2 must be at most 2^31 (got %lld)", g.lanes);
        return SNAKE_E_ARG;
    }
    for (int i = 0; i < graph::kMaxSteps; i++) g.wt[0][i] = g.wt[1][i] = 0.0;
    graph::fill_weights(g.n, cfg->vision_range == 0, g.wt[0], g.wt[1]);
    const long long blocks = (g.lanes + graph::kBlock - 1) / graph::kBlock;     // at most 2^23
    const hipStream_t s = (hipStream_t)stream;
    DeviceGuard dg(s);
    if (dg.dev < 0) return SNAKE_E_LAUNCH;
    hipLaunchKernelGGL(graph::k_graph_obs, dim3((unsigned)blocks), dim3(graph::kBlock), 0, s, g);
    return launch_status("k_graph_obs");
}
