// policy_kernels.hip -- the reference evaluator's safe-action selection
// (train_dqn.py:433-580 DQN_Evaluator.get_action and the loop at :625-646) for
// every env of a batch; semantics in include/snake_env.h (snake_safe_actions).
//
// k_safe_actions: one workgroup per env, one wave per snake.
//
//  1. The wave's cells are its snake's h*w; the front end of obs_rows.h turns
//     them into six flag bits per cell (channel == 1 tests) and lane r's six
//     w-bit row words of row r (deadly-but-tail, fruit, other head, my head, my
//     body, my tail), and counts the snake's own cells on the way.
//  2. Everything that depends on the snake's own observation alone: the head,
//     the direction, the three targets, the out-of-map / deadly / beside-a-head
//     tests, and the flood fill of the three targets as a fixpoint of
//         reach = ((reach | reach << 1 | reach >> 1 | up | down) & free) | start
//     with the rows above and below taken from the neighbouring lanes. The
//     reference's BFS pops at most `limit` cells of the target's component, so
//     its count is min(limit, component size) whatever the order, and the move
//     is masked when that is less than the length L the snake will have: always
//     when L > limit, else when the component has fewer than L cells. So a fill
//     stops when nothing changes (masked) or it has counted L cells (not
//     masked); a changing pass adds at least one cell, so `limit` passes always
//     suffice. The count is a sum over the lanes' row popcounts, bit by bit
//     (one __ballot per bit), with no lane exchange.
//  3. After a barrier thread 0 takes the env's snakes in order: the cells
//     claimed by earlier snakes, the argmax of the masked Q-values, the new
//     direction and the claim of head + move.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "snake_internal.h"
#include "snake_device.h"
#include "obs_rows.h"

namespace snake {
namespace policy {

constexpr int kMaxLimit = 4096;    // = kMaxSide^2: a larger limit never binds
constexpr int kFlags = 6;
enum { F_DEAD6 = 0, F_FRUIT = 1, F_OHEAD = 2, F_MYHEAD = 3, F_MYBODY = 4, F_MYTAIL = 5 };
constexpr uint32_t kLengthFlags = 1u << F_MYHEAD | 1u << F_MYBODY | 1u << F_MYTAIL;     // the snake's own cells

struct Args {
    const uint8_t *obs;
    const float *q;
    const uint8_t *skip;    // may be NULL
    int8_t *dirs;
    int8_t *actions;
    long long cells;        // N * S * h * w: cells in obs
    int S, h, w, limit;
    int nw;                 // 64-bit words of one flag's bit string in LDS
    int cbits;              // bits of a row's cell count: w < 2^cbits
};

// What the wave of snake s leaves for the env's sequential pass.
struct Rec {
    int state;              // 0 skipped, 1 no head, 2 head found
    int hy, hx, dy, dx;
    int masked;             // bit a: move a is masked by the snake's own observation
};

// the six flag bits of one cell: lo = channels 0-3, hi = channels 4-7
__device__ __forceinline__ uint32_t cell_flags(uint32_t lo, uint32_t hi)
{
    const uint32_t a = bytes_eq1(lo), b = bytes_eq1(hi);
    uint32_t f = 0;
    if ((a & 0x80800080u) | (b & 0x00800080u)) f |= 1u << F_DEAD6;   // channels 0, 2, 3, 4, 6
    if (a & 0x00008000u) f |= 1u << F_FRUIT;
    if (a & 0x00800000u) f |= 1u << F_OHEAD;
    if (b & 0x00008000u) f |= 1u << F_MYHEAD;
    if (b & 0x00800000u) f |= 1u << F_MYBODY;
    if (b & 0x80000000u) f |= 1u << F_MYTAIL;
    return f;
}

// bit (y, x) of the map whose row r is `word` on lane r; (y, x) is tested against
// the bounds first
__device__ __forceinline__ bool bit_at(uint64_t word, int lane, int y, int x, int h, int w)
{
    const bool in = y >= 0 && y < h && x >= 0 && x < w;
    return __ballot(in && lane == y && ((word >> (x & 63)) & 1)) != 0;
}

__device__ __forceinline__ uint64_t row_above(uint64_t v, int lane)
{
    const uint64_t t = __shfl_up(v, 1);
    return lane == 0 ? 0 : t;
}

__device__ __forceinline__ uint64_t row_below(uint64_t v, int lane)
{
    const uint64_t t = __shfl_down(v, 1);
    return lane == 63 ? 0 : t;
}

// the set bits of v over the wave; cbits: bits of a lane's count (<= w < 2^cbits)
__device__ __forceinline__ int wave_popcount(uint64_t v, int cbits)
{
    const int pc = __popcll(v);
    int c = 0;
    for (int b = 0; b < cbits; b++) c += __popcll(__ballot((pc >> b) & 1)) << b;
    return c;
}

__global__ void __launch_bounds__(1024) k_safe_actions(const Args g)
{
    extern __shared__ uint64_t lin_all[];       // [S][kFlags][nw]
    __shared__ Rec recs[kMaxSnakes];
    const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
    const long long n = blockIdx.x;
    const int h = g.h, w = g.w, hw = h * w;
    const long long snake = n * g.S + s;

    const bool skipped = g.skip != nullptr && g.skip[snake] != 0;
    if (!skipped) {
        uint64_t *lin = lin_all + (size_t)s * kFlags * g.nw;
        // ---- 1. the cells -> row words
        const FlagStrings fs = load_flag_strings<kFlags, kLengthFlags>(
            g.obs, g.cells, snake * hw, hw, lin, g.nw, lane, cell_flags);
        const int length = fs.count;
        // row r = bits [r*w + d, r*w + d + w) of each string
        const uint64_t wmask = w == 64 ? ~0ull : (1ull << w) - 1;
        const uint64_t rowmask = lane < h ? wmask : 0;
        const int start = (lane < h ? lane : 0) * w + fs.d;
        uint64_t m[kFlags];
#pragma unroll
        for (int k = 0; k < kFlags; k++) m[k] = cut_row(lin + k * g.nw, start) & rowmask;
        // ---- 2. the snake's own observation
        Rec r;
        r.state = 1;
        r.hy = r.hx = r.dy = r.dx = 0;
        r.masked = 0;
        const uint64_t hrows = __ballot(m[F_MYHEAD] != 0);
        if (hrows) {
            const int hy = __builtin_ctzll(hrows);
            const int hx = __shfl(m[F_MYHEAD] ? __builtin_ctzll(m[F_MYHEAD]) : 0, hy);
            const uint64_t trows = __ballot(m[F_MYTAIL] != 0);
            const int ty = trows ? __builtin_ctzll(trows) : -1;
            const int tx = __shfl(m[F_MYTAIL] ? __builtin_ctzll(m[F_MYTAIL]) : 0, ty < 0 ? 0 : ty);
            int dy = g.dirs[snake * 2], dx = g.dirs[snake * 2 + 1];
            if (dy == SNAKE_DIR_UNKNOWN && dx == SNAKE_DIR_UNKNOWN) {
                // get_current_direction: the body or tail cell behind the head
                const uint64_t bt = m[F_MYBODY] | m[F_MYTAIL];
                if (bit_at(bt, lane, hy + 1, hx, h, w)) dy = -1, dx = 0;
                else if (bit_at(bt, lane, hy - 1, hx, h, w)) dy = 1, dx = 0;
                else if (bit_at(bt, lane, hy, hx + 1, h, w)) dy = 0, dx = -1;
                else if (bit_at(bt, lane, hy, hx - 1, h, w)) dy = 0, dx = 1;
                else dy = -1, dx = 0;
            }
            const uint64_t deadly = m[F_DEAD6] | m[F_MYTAIL];
            const uint64_t oh = m[F_OHEAD];
            const uint64_t near = oh << 1 | oh >> 1 | row_above(oh, lane) | row_below(oh, lane);
            const uint64_t headbit = lane == hy ? 1ull << hx : 0;
            const uint64_t free0 = ~deadly & rowmask & ~headbit;
            // no fruit at the target: the tail cell moves away (it stays blocked when
            // another deadly channel is set there or it is the old head cell)
            const uint64_t free1 = free0 | ((lane == ty ? 1ull << tx : 0) & ~m[F_DEAD6] & ~headbit & rowmask);
            const int my[3] = {dy, -dx, dx}, mx[3] = {dx, dy, -dy};
            uint64_t fr[3], st[3], re[3];
            int need[3];
            bool act[3];
            int masked = 0;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const int y = hy + my[a], x = hx + mx[a];
                const bool in = y >= 0 && y < h && x >= 0 && x < w;
                const bool bad = !in || bit_at(deadly, lane, y, x, h, w) || bit_at(near, lane, y, x, h, w);
                const bool fruit = bit_at(m[F_FRUIT], lane, y, x, h, w);
                if (bad) masked |= 1 << a;
                fr[a] = fruit ? free0 : free1;
                st[a] = (!bad && lane == y) ? 1ull << (x & 63) : 0;
                re[a] = st[a];
                need[a] = length + (fruit ? 1 : 0);
                // min(limit, component) < need is all that is asked: a snake longer
                // than the limit is masked without a fill, any other fill may stop
                // once it has counted `need` cells
                act[a] = !bad && need[a] <= g.limit;
                if (!bad && need[a] > g.limit) masked |= 1 << a;
            }
            // the three fills. A pass that leaves a fill unfinished adds at least one
            // cell to it, so pass `it` starts with more than `it` cells: need <= limit
            // cells are counted, or the component is exhausted, within `limit` passes.
            for (int it = 0; it < g.limit && (act[0] || act[1] || act[2]); it++) {
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    if (!act[a]) continue;      // (wave-uniform)
                    const uint64_t v = re[a];
                    if (wave_popcount(v, g.cbits) >= need[a]) {
                        act[a] = false;
                        continue;
                    }
                    const uint64_t nv =
                        ((v | v << 1 | v >> 1 | row_above(v, lane) | row_below(v, lane)) & fr[a]) | st[a];
                    if (__ballot(nv != v) == 0) {       // the whole component, and too small
                        masked |= 1 << a;
                        act[a] = false;
                    }
                    re[a] = nv;
                }
            }
            r.state = 2;
            r.hy = hy;
            r.hx = hx;
            r.dy = dy;
            r.dx = dx;
            r.masked = masked;
        }
        if (lane == 0) recs[s] = r;
    } else if (lane == 0) {
        recs[s].state = 0;
    }
    __syncthreads();
    // ---- 3. the env's snakes in order
    if (threadIdx.x != 0) return;
    int claimed[kMaxSnakes], nclaimed = 0;
    for (int i = 0; i < g.S; i++) {
        const Rec r = recs[i];
        const long long si = n * g.S + i;
        if (r.state == 0) {
            g.actions[si] = 0;
            continue;
        }
        if (r.state == 1) {
            g.actions[si] = 0;
            g.dirs[si * 2] = 0;
            g.dirs[si * 2 + 1] = 0;
            continue;
        }
        const int my[3] = {r.dy, -r.dx, r.dx}, mx[3] = {r.dx, r.dy, -r.dy};
        int best = 0, cell[3];
        float qbest = 0.f;
        for (int a = 0; a < 3; a++) {
            // |move| <= 128 and the head is inside the map: both fields stay positive
            cell[a] = (r.hy + my[a] + 256) * 1024 + (r.hx + mx[a] + 256);
            bool masked = (r.masked >> a & 1) != 0;
            for (int j = 0; j < nclaimed; j++) masked |= claimed[j] == cell[a];
            const float qa = masked ? -INFINITY : g.q[si * 3 + a];
            if (a == 0 || qa > qbest) {
                best = a;
                qbest = qa;
            }
        }
        g.actions[si] = (int8_t)best;
        g.dirs[si * 2] = (int8_t)my[best];
        g.dirs[si * 2 + 1] = (int8_t)mx[best];
        claimed[nclaimed++] = cell[best];
    }
}

int check_cfg(const snake_policy_cfg *c)
{
    if (!c) { set_error("snake_policy: cfg is NULL"); return SNAKE_E_CONFIG; }
    if (c->obs_c != 8) {
        set_error("snake_policy: obs_c must be 8 (frame_stack 1; got %d)", c->obs_c);
        return SNAKE_E_CONFIG;
    }
    if (c->obs_h < 1 || c->obs_h > kMaxSide || c->obs_w < 1 || c->obs_w > kMaxSide) {
        set_error("snake_policy: obs_h and obs_w must be in [1, %d] (got %d x %d)", kMaxSide, c->obs_h, c->obs_w);
        return SNAKE_E_CONFIG;
    }
    if (c->num_snakes < 1 || c->num_snakes > kMaxSnakes) {
        set_error("snake_policy: num_snakes must be in [1, %d] (got %d)", kMaxSnakes, c->num_snakes);
        return SNAKE_E_CONFIG;
    }
    if (c->fill_limit < 1 || c->fill_limit > kMaxLimit) {
        set_error("snake_policy: fill_limit must be in [1, %d] (got %d)", kMaxLimit, c->fill_limit);
        return SNAKE_E_CONFIG;
    }
    return SNAKE_OK;
}

}  // namespace policy
}  // namespace snake

using namespace snake;

extern "C" int snake_policy_plan(const snake_policy_cfg *cfg) { return policy::check_cfg(cfg); }

extern "C" int snake_safe_actions(const snake_policy_cfg *cfg, const uint8_t *obs, const float *q,
                                  const uint8_t *skip, int8_t *dirs, int8_t *actions, int64_t num_envs,
                                  void *stream)
{
    if (int rc = policy::check_cfg(cfg)) return rc;
    if (!q) { set_error("snake_safe_actions: NULL buffer"); return SNAKE_E_ARG; }     // (before obs's alignment)
    bool nothing;
    if (int rc = check_obs_call("snake_safe_actions", cfg, obs, dirs, actions, num_envs, &nothing)) return rc;
    if (nothing) return SNAKE_OK;
    policy::Args g;
    g.obs = obs;
    g.q = q;
    g.skip = skip;
    g.dirs = dirs;
    g.actions = actions;
    g.S = cfg->num_snakes;
    g.h = cfg->obs_h;
    g.w = cfg->obs_w;
    g.limit = cfg->fill_limit;
    g.cells = (long long)num_envs * g.S * g.h * g.w;
    g.nw = flag_words(g.h * g.w);
    g.cbits = 1;
    while ((1 << g.cbits) <= g.w) g.cbits++;
    const size_t lds = (size_t)g.S * policy::kFlags * g.nw * sizeof(uint64_t);   // at most 52 KB
    const hipStream_t s = (hipStream_t)stream;
    DeviceGuard dg(s);
    if (dg.dev < 0) return SNAKE_E_LAUNCH;
    hipLaunchKernelGGL(policy::k_safe_actions, dim3((unsigned)num_envs), dim3(64 * g.S), lds, s, g);
    return launch_status("k_safe_actions");
}
