// greedy_kernels.hip -- the rule-based fruit seeker of the reference's battle
// mode (train_dqn.py:774-856 GreedyEnemy.get_action) for every snake of a
// batch; semantics in include/snake_env.h (snake_greedy_actions).
//
// k_greedy<G>: a wave holds G snakes (consecutive in the flat index N*S, so
// they may belong to different envs), each on R = 64 / G lanes, lane l holding
// row l % R of snake G * wave + l / R.
//   G = 1: rows on 64 lanes, any h <= 64.
//   G = 4: four snakes per wave for h <= 16.
//
//  1. The wave's snakes are contiguous in memory: their G*h*w cells go through
//     the front end of obs_rows.h as one string of four flag bits per cell
//     (channel == 1 tests), and every lane cuts its row out of each string at
//     (l / R) * h*w + (l % R) * w: four w-bit row words (deadly, fruit, my
//     head, my body|tail).
//  2. Per snake, on its R lanes: the head (first row with a head bit), the
//     direction, the nearest fruit -- in a row the only candidates are the
//     highest fruit bit at or left of the head's column and the lowest one
//     right of it; a minimum over the lanes of (distance, y, x) picks the first
//     in row-major order among equals -- and the three moves' cells.
//     A reduction over a snake's lanes is its R bits of a __ballot, or log2(R)
//     xor-shuffle steps, which stay inside an aligned group of R lanes.
// No barrier and no pass over the snakes of an env: the waves of a workgroup
// are independent, four of them only to share a launch slot.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdint.h>

#include "snake_internal.h"
#include "snake_device.h"
#include "obs_rows.h"

namespace snake {
namespace greedy {

constexpr int kWaves = 4;          // waves per workgroup
constexpr int kPackRows = 16;      // G = 4: a snake's rows on 16 lanes
constexpr int kFlags = 4;
enum { F_DEADLY = 0, F_FRUIT = 1, F_HEAD = 2, F_BODY = 3 };
constexpr int kNw = flag_words(kMaxSide * kMaxSide);     // a wave has G*h*w <= 4096 cells

struct Args {
    const uint8_t *obs;
    const uint32_t *rnd;    // may be NULL
    const uint8_t *skip;    // may be NULL
    int8_t *dirs;
    int8_t *actions;
    long long cells;        // N * S * h * w: cells in obs
    long long snakes;       // N * S
    int h, w;
};

// the four flag bits of one cell: lo = channels 0-3, hi = channels 4-7
__device__ __forceinline__ uint32_t cell_flags(uint32_t lo, uint32_t hi)
{
    const uint32_t a = bytes_eq1(lo), b = bytes_eq1(hi);
    uint32_t f = 0;
    if ((a & 0x80800080u) | (b & 0x80800080u)) f |= 1u << F_DEADLY;   // channels 0, 2, 3, 4, 6, 7
    if (a & 0x00008000u) f |= 1u << F_FRUIT;
    if (b & 0x00008000u) f |= 1u << F_HEAD;
    if (b & 0x80800000u) f |= 1u << F_BODY;                            // channels 6, 7
    return f;
}

template <int G>
__global__ void __launch_bounds__(64 * kWaves) k_greedy(const Args g)
{
    constexpr int R = 64 / G;
    __shared__ uint64_t lin_all[kWaves][kFlags * kNw];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long first = ((long long)blockIdx.x * kWaves + wv) * G;   // the wave's first snake
    if (first >= g.snakes) return;
    const int grp = lane / R, r = lane % R, gbase = grp * R;
    const uint64_t gmask = R == 64 ? ~0ull : (1ull << R) - 1;
    const long long snake = first + grp;
    const bool valid = snake < g.snakes;
    const bool live = valid && !(g.skip != nullptr && g.skip[snake] != 0);
    if (__ballot(live) == 0) {          // every snake of the wave is skipped
        if (valid && r == 0) g.actions[snake] = 0;
        return;
    }
    const int h = g.h, w = g.w, hw = h * w;
    const int nsn = g.snakes - first < G ? (int)(g.snakes - first) : G;
    const int count = nsn * hw;         // the wave's cells
    uint64_t *lin = lin_all[wv];
    // ---- 1. the cells -> row words
    const int d = load_flag_strings<kFlags, 0>(g.obs, g.cells, first * hw, count, lin, kNw, lane, cell_flags).d;
    // the lane's row = bits [start, start + w) of each string
    const bool has_row = grp < nsn && r < h;
    const uint64_t wmask = w == 64 ? ~0ull : (1ull << w) - 1;
    const uint64_t rowmask = has_row ? wmask : 0;
    const int start = (has_row ? grp * hw + r * w : 0) + d;
    uint64_t m[kFlags];
#pragma unroll
    for (int k = 0; k < kFlags; k++) m[k] = cut_row(lin + k * kNw, start) & rowmask;
    // ---- 2. per snake. Every lane runs every ballot and shuffle: the branches
    // below are on values uniform over the wave or taken after the last exchange.
    auto any = [&](bool p) { return ((__ballot(p) >> gbase) & gmask) != 0; };
    // bit (y, x) of the map whose row is `word` on the snake's lane y; (y, x) is
    // tested against the bounds first
    auto at = [&](uint64_t word, int y, int x) {
        return y >= 0 && y < h && x >= 0 && x < w && r == y && ((word >> (x & 63)) & 1);
    };
    const uint64_t hrows = (__ballot(m[F_HEAD] != 0) >> gbase) & gmask;
    const bool go = live && hrows != 0;
    const int hy = hrows ? __builtin_ctzll(hrows) : 0;
    const int hx = __shfl(m[F_HEAD] ? __builtin_ctzll(m[F_HEAD]) : 0, gbase + hy);
    int dy = 0, dx = 0;
    if (go) {
        dy = g.dirs[snake * 2];
        dx = g.dirs[snake * 2 + 1];
    }
    const bool unknown = go && dy == SNAKE_DIR_UNKNOWN && dx == SNAKE_DIR_UNKNOWN;
    if (__ballot(unknown)) {
        const uint64_t bt = m[F_BODY];
        const bool up = any(at(bt, hy - 1, hx)), down = any(at(bt, hy + 1, hx));
        const bool left = any(at(bt, hy, hx - 1)), right = any(at(bt, hy, hx + 1));
        if (unknown) {      // direction = head - neighbour
            if (up) dy = 1, dx = 0;
            else if (down) dy = -1, dx = 0;
            else if (left) dy = 0, dx = 1;
            else if (right) dy = 0, dx = -1;
            else dy = -1, dx = 0;
        }
    }
    // the nearest fruit: key = distance << 12 | y << 6 | x (distance <= 126)
    uint32_t key = ~0u;
    {
        const uint64_t f = m[F_FRUIT];
        const uint64_t le = hx == 63 ? ~0ull : (2ull << hx) - 1;    // columns <= hx
        const uint64_t fl = f & le, fr = f & ~le;
        const int ady = r > hy ? r - hy : hy - r;
        if (fl) {
            const int x = 63 - __builtin_clzll(fl);
            key = (uint32_t)((ady + hx - x) << 12 | r << 6 | x);
        }
        if (fr) {
            const int x = __builtin_ctzll(fr);
            const uint32_t k2 = (uint32_t)((ady + x - hx) << 12 | r << 6 | x);
            key = k2 < key ? k2 : key;      // (left wins a tie: the smaller x)
        }
    }
#pragma unroll
    for (int s = 1; s < R; s <<= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)key, s);
        key = o < key ? o : key;
    }
    const bool fruit = key != ~0u;
    const int fy = (key >> 6) & 63, fx = key & 63;
    const int my[3] = {dy, -dx, dx}, mx[3] = {dx, dy, -dy};
    int best = INT_MIN, score[3];
    bool dead[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int y = hy + my[a], x = hx + mx[a];
        const bool in = y >= 0 && y < h && x >= 0 && x < w;
        dead[a] = any(at(m[F_DEADLY], y, x)) || !in;
        const int ay = y > fy ? y - fy : fy - y, ax = x > fx ? x - fx : fx - x;
        score[a] = fruit ? -(ay + ax) : 0;
        if (!dead[a] && score[a] > best) best = score[a];
    }
    if (r != 0 || !valid) return;
    if (!go) {
        g.actions[snake] = 0;
        return;
    }
    uint32_t tie = 0;
#pragma unroll
    for (int a = 0; a < 3; a++)
        if (!dead[a] && score[a] == best) tie |= 1u << a;
    int chosen = 0;
    if (tie) {
        const uint32_t u = g.rnd != nullptr ? g.rnd[snake] : 0;
        const int pick = (int)(((uint64_t)u * (uint32_t)__popc(tie)) >> 32);
        for (int i = 0; i < pick; i++) tie &= tie - 1;
        chosen = __builtin_ctz(tie);
    }
    g.actions[snake] = (int8_t)chosen;
    g.dirs[snake * 2] = (int8_t)(chosen == 0 ? my[0] : chosen == 1 ? my[1] : my[2]);
    g.dirs[snake * 2 + 1] = (int8_t)(chosen == 0 ? mx[0] : chosen == 1 ? mx[1] : mx[2]);
}

}  // namespace greedy
}  // namespace snake

using namespace snake;

namespace {

// rows_only: one snake per wave whatever the height (snake_debug_greedy_actions)
int greedy_launch(const snake_policy_cfg *cfg, const uint8_t *obs, const uint32_t *rnd, const uint8_t *skip,
                  int8_t *dirs, int8_t *actions, int64_t num_envs, void *stream, bool rows_only)
{
    bool nothing;
    if (int rc = check_obs_call("snake_greedy_actions", cfg, obs, dirs, actions, num_envs, &nothing)) return rc;
    // (after the num_envs range, where it used to come before it: a call wrong in both reports the range)
    if ((uintptr_t)rnd & 3) { set_error("snake_greedy_actions: rnd must be 4-byte aligned"); return SNAKE_E_ARG; }
    if (nothing) return SNAKE_OK;
    greedy::Args g;
    g.obs = obs;
    g.rnd = rnd;
    g.skip = skip;
    g.dirs = dirs;
    g.actions = actions;
    g.h = cfg->obs_h;
    g.w = cfg->obs_w;
    g.snakes = (long long)num_envs * cfg->num_snakes;
    g.cells = g.snakes * g.h * g.w;
    const bool packed = g.h <= greedy::kPackRows && !rows_only;
    const long long waves = packed ? (g.snakes + 3) / 4 : g.snakes;
    const dim3 grid((unsigned)((waves + greedy::kWaves - 1) / greedy::kWaves)), block(64 * greedy::kWaves);
    const hipStream_t s = (hipStream_t)stream;
    DeviceGuard dg(s);
    if (dg.dev < 0) return SNAKE_E_LAUNCH;
    if (packed) hipLaunchKernelGGL(greedy::k_greedy<4>, grid, block, 0, s, g);
    else hipLaunchKernelGGL(greedy::k_greedy<1>, grid, block, 0, s, g);
    return launch_status("k_greedy");
}

}  // namespace

extern "C" int snake_greedy_actions(const snake_policy_cfg *cfg, const uint8_t *obs, const uint32_t *rnd,
                                    const uint8_t *skip, int8_t *dirs, int8_t *actions, int64_t num_envs,
                                    void *stream)
{
    return greedy_launch(cfg, obs, rnd, skip, dirs, actions, num_envs, stream, false);
}

// Testing aid, not part of the C-ABI (like the snake_debug_* readers of
// snake_diag.h): snake_greedy_actions with the layout as an argument, rows_only
// != 0 = one snake per wave for any height. It keeps no state. The tests hold
// the two layouts against each other, scripts/greedy_bench.py times both.
extern "C" int snake_debug_greedy_actions(const snake_policy_cfg *cfg, const uint8_t *obs, const uint32_t *rnd,
                                          const uint8_t *skip, int8_t *dirs, int8_t *actions, int64_t num_envs,
                                          void *stream, int rows_only)
{
    return greedy_launch(cfg, obs, rnd, skip, dirs, actions, num_envs, stream, rows_only != 0);
}
