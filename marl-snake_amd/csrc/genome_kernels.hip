// genome_kernels.hip -- a population of NEAT decision heads, one genome per env
// (train_ga.py:224-257 eval_genomes: neat.nn.FeedForwardNetwork.activate on the
// frozen DQN's features, then np.argmax); semantics in include/snake_env.h
// (snake_genome_actions).
//
// k_genome_actions: one wave per tile. A tile is up to tile_rows feature rows
// that share one genome (snake_genome_tiles groups the rows by genome on the
// host), so everything that belongs to the genome -- node records, link sources
// and weights -- is read at wave-uniform addresses (scalar loads), and a lane
// owns one feature row.
//
//  1. The tile's feature rows are loaded row by row, lane j taking feature j
//     (coalesced), and written to LDS transposed, in[j][r] at a pitch of
//     tile_rows + 1 floats: the odd pitch puts the 32 lanes of a write on 32
//     banks, and the reads below (lane r reads in[j][r]) are consecutive.
//  2. Lane r walks the genome's nodes in evaluation order. A node's sum is the
//     contract's serial float64 sum: s = s + v * w, product rounded first (the
//     library is built with -ffp-contract=off), from +0.0, links in order; the
//     links are fetched eight at a time, only the adds form the chain. Node
//     values are indexed by the link's source slot, so they live in memory and
//     not in registers: val[node][lane] doubles in LDS for genomes of at most
//     lds_nodes nodes, else in the tile's slice of the global scratch (the
//     branch is per tile, wave-uniform). A lane reads only its own column.
//  3. The outputs are read back by their slots (-1: never evaluated, 0.0), the
//     first maximum is the action, and a set skip byte overrides it with 0.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include "snake_internal.h"
#include "snake_device.h"

namespace snake {
namespace genome {

constexpr int kMaxInputs = 1024;
constexpr int kMaxOutputs = 16;
constexpr int kMaxGenomes = 1 << 20;
constexpr int kLdsBudget = 64 * 1024;   // per wave: two tiles a CU at the limit, more for small genomes
constexpr int kLdsInputs = 40 * 1024;   // of which the staged features take at most this
constexpr int kChunk = 8;              // links fetched together (walk)
constexpr int kNumAct = 3;              // SNAKE_GENOME_RELU / _SIGMOID / _TANH

struct Args {
    snake_genome_prog p;
    const snake_genome_tile *tiles;
    const int32_t *rows;
    const float *features;
    const uint8_t *skip;    // may be NULL
    int8_t *actions;
    double *outputs;        // may be NULL
    double *scratch;        // [scratch tile][max_nodes][64]; NULL when no tile needs it
    int I, A, W;            // inputs, outputs, rows per tile
    int max_nodes;
};

__device__ __forceinline__ double activate(int act, double z)
{
    if (act == SNAKE_GENOME_RELU) return z > 0.0 ? z : 0.0;
    if (act == SNAKE_GENOME_SIGMOID) {
        z = fmax(-60.0, fmin(60.0, 5.0 * z));
        return 1.0 / (1.0 + exp(-z));
    }
    z = fmax(-60.0, fmin(60.0, 2.5 * z));
    return tanh(z);
}

// The nodes of one genome for the lane's row. val: the lane's column of the node
// values, val[k * vpitch] node k; in: the lane's column of the staged features.
__device__ __forceinline__ void walk(const Args &g, int n0, int n1, const float *in, int ipitch, double *val,
                                     int vpitch)
{
    const int I = g.I;
    for (int n = n0; n < n1; n++) {
        const int l0 = g.p.link_off[n], l1 = g.p.link_off[n + 1];
        double s = 0.0;
        int l = l0;
        // Eight links at a time: their sources, weights and values are fetched
        // together, and only the adds form the serial chain. Both places a
        // value can live are read (at a clamped index; val[0] may not be
        // written yet) and one is selected, so no branch separates the loads.
        for (; l + kChunk <= l1; l += kChunk) {
            double v[kChunk];
#pragma unroll
            for (int k = 0; k < kChunk; k++) {
                const int src = g.p.link_src[l + k];
                const float f = in[(src < I ? src : 0) * ipitch];
                const double d = val[(size_t)(src < I ? 0 : src - I) * vpitch];
                v[k] = (src < I ? (double)f : d) * g.p.link_w[l + k];
            }
#pragma unroll
            for (int k = 0; k < kChunk; k++) s = s + v[k];
        }
        for (; l < l1; l++) {
            const int src = g.p.link_src[l];
            const double v = src < I ? (double)in[src * ipitch] : val[(size_t)(src - I) * vpitch];
            const double t = v * g.p.link_w[l];
            s = s + t;
        }
        const double r = g.p.node_resp[n] * s;
        val[(size_t)(n - n0) * vpitch] = activate(g.p.node_act[n], g.p.node_bias[n] + r);
    }
}

// Steps 2 and 3 for the lane's row; in, val: the lane's columns as in walk().
__device__ __forceinline__ void finish(const Args &g, const snake_genome_tile &t, int n0, int n1, const float *in,
                                       int ipitch, double *val, int vpitch)
{
    const int I = g.I, lane = threadIdx.x;
    const long long row = g.rows[t.row_start + lane];
    // ---- 2. the genome
    walk(g, n0, n1, in, ipitch, val, vpitch);
    // ---- 3. outputs and the first maximum
    int best = 0;
    double vbest = 0.0;
    for (int a = 0; a < g.A; a++) {
        const int slot = g.p.out_slot[(long long)t.genome * g.A + a];
        const double v = slot < 0 ? 0.0 : slot < I ? (double)in[slot * ipitch] : val[(size_t)(slot - I) * vpitch];
        if (g.outputs) g.outputs[row * g.A + a] = v;
        if (a == 0 || v > vbest) {
            best = a;
            vbest = v;
        }
    }
    if (g.skip != nullptr && g.skip[row] != 0) best = 0;
    g.actions[row] = (int8_t)best;
}

__global__ void __launch_bounds__(64) k_genome_actions(const Args g)
{
    extern __shared__ double lds_val[];     // [lds nodes][W] doubles, then [I][W + 1] floats
    const int lane = threadIdx.x;
    const snake_genome_tile t = g.tiles[blockIdx.x];
    const int I = g.I, W = g.W, ipitch = W + 1;
    const int n0 = g.p.node_off[t.genome], n1 = g.p.node_off[t.genome + 1];
    const bool in_lds = t.scratch < 0;
    float *in_all = reinterpret_cast<float *>(lds_val + (size_t)(in_lds ? n1 - n0 : 0) * W);
    // ---- 1. the tile's features, transposed
    for (int r = 0; r < t.count; r++) {
        const float *row = g.features + (long long)g.rows[t.row_start + r] * I;
        for (int j = lane; j < I; j += 64) in_all[j * ipitch + r] = row[j];
    }
    __syncthreads();
    if (lane >= t.count) return;
    // (two calls: each sees the address space of its node values)
    if (in_lds) finish(g, t, n0, n1, in_all + lane, ipitch, lds_val + lane, W);
    else finish(g, t, n0, n1, in_all + lane, ipitch, g.scratch + (size_t)t.scratch * g.max_nodes * 64 + lane, 64);
}

int check_cfg(const snake_genome_cfg *c)
{
    if (!c) { set_error("snake_genome: cfg is NULL"); return SNAKE_E_CONFIG; }
    if (c->num_inputs < 1 || c->num_inputs > kMaxInputs) {
        set_error("snake_genome: num_inputs must be in [1, %d] (got %d)", kMaxInputs, c->num_inputs);
        return SNAKE_E_CONFIG;
    }
    if (c->num_outputs < 1 || c->num_outputs > kMaxOutputs) {
        set_error("snake_genome: num_outputs must be in [1, %d] (got %d)", kMaxOutputs, c->num_outputs);
        return SNAKE_E_CONFIG;
    }
    if (c->num_genomes < 1 || c->num_genomes > kMaxGenomes) {
        set_error("snake_genome: num_genomes must be in [1, %d] (got %d)", kMaxGenomes, c->num_genomes);
        return SNAKE_E_CONFIG;
    }
    // slots and offsets are int32
    if (c->num_nodes < 0 || c->num_nodes > (1ll << 30)) {
        set_error("snake_genome: num_nodes must be in [0, 2^30] (got %lld)", (long long)c->num_nodes);
        return SNAKE_E_CONFIG;
    }
    if (c->num_links < 0 || c->num_links > (1ll << 30)) {
        set_error("snake_genome: num_links must be in [0, 2^30] (got %lld)", (long long)c->num_links);
        return SNAKE_E_CONFIG;
    }
    if (c->max_nodes < 0 || c->max_nodes > c->num_nodes ||
        (int64_t)c->max_nodes * c->num_genomes < c->num_nodes) {
        set_error("snake_genome: max_nodes %d is not the largest genome of %d with %lld nodes in all", c->max_nodes,
                  c->num_genomes, (long long)c->num_nodes);
        return SNAKE_E_CONFIG;
    }
    return SNAKE_OK;
}

// rows per tile: the most of 64, 32, 16, 8 whose staged features fit kLdsInputs
// (1 024 inputs * 9 floats = 36 KB)
int tile_rows(int I)
{
    int W = 64;
    while (W > 8 && I * (W + 1) * 4 > kLdsInputs) W >>= 1;
    return W;
}

int layout_of(const snake_genome_cfg *c, int64_t rows, snake_genome_layout *out)
{
    if (int rc = check_cfg(c)) return rc;
    if (rows < 0 || rows > (1ll << 30)) {
        set_error("snake_genome: rows must be in [0, 2^30] (got %lld)", (long long)rows);
        return SNAKE_E_ARG;
    }
    const int W = tile_rows(c->num_inputs);
    const int in_bytes = (c->num_inputs * (W + 1) * 4 + 7) & ~7;
    snake_genome_layout o;
    o.tile_rows = W;
    o.lds_nodes = (kLdsBudget - in_bytes) / (W * 8);
    const int held = c->max_nodes < o.lds_nodes ? c->max_nodes : o.lds_nodes;
    o.lds_bytes = in_bytes + held * W * 8;
    // every genome ends in at most one tile that is not full
    const int64_t full = (rows + W - 1) / W + c->num_genomes;
    o.max_tiles = full < rows ? full : rows;
    o.scratch = c->max_nodes > o.lds_nodes ? o.max_tiles * c->max_nodes * 64 * 8 : 0;
    if (out) *out = o;
    return SNAKE_OK;
}

}  // namespace genome
}  // namespace snake

using namespace snake;

extern "C" int snake_genome_plan(const snake_genome_cfg *cfg, int64_t rows, snake_genome_layout *out)
{
    return genome::layout_of(cfg, rows, out);
}

extern "C" int snake_genome_check(const snake_genome_cfg *cfg, const snake_genome_prog *p)
{
    if (int rc = genome::check_cfg(cfg)) return rc;
    if (!p || !p->node_off || !p->out_slot || (cfg->num_nodes && (!p->node_act || !p->node_bias || !p->node_resp)) ||
        !p->link_off || (cfg->num_links && (!p->link_src || !p->link_w))) {
        set_error("snake_genome_check: NULL array");
        return SNAKE_E_ARG;
    }
    const int G = cfg->num_genomes, I = cfg->num_inputs, A = cfg->num_outputs;
    if (p->node_off[0] != 0 || p->node_off[G] != cfg->num_nodes) {
        set_error("snake_genome_check: node_off must run from 0 to num_nodes %lld (got %d .. %d)",
                  (long long)cfg->num_nodes, p->node_off[0], p->node_off[G]);
        return SNAKE_E_CONFIG;
    }
    if (p->link_off[0] != 0 || p->link_off[cfg->num_nodes] != cfg->num_links) {
        set_error("snake_genome_check: link_off must run from 0 to num_links %lld (got %d .. %d)",
                  (long long)cfg->num_links, p->link_off[0], p->link_off[cfg->num_nodes]);
        return SNAKE_E_CONFIG;
    }
    for (int64_t n = 0; n < cfg->num_nodes; n++) {      // (first: the loops below walk these ranges)
        if (p->link_off[n + 1] < p->link_off[n] || p->link_off[n + 1] > cfg->num_links) {
            set_error("snake_genome_check: link_off is not monotone at node %lld (%d then %d)", (long long)n,
                      p->link_off[n], p->link_off[n + 1]);
            return SNAKE_E_CONFIG;
        }
    }
    int largest = 0;
    for (int gi = 0; gi < G; gi++) {
        const int n0 = p->node_off[gi], n1 = p->node_off[gi + 1];
        if (n1 < n0 || n1 > cfg->num_nodes) {
            set_error("snake_genome_check: node_off is not monotone at genome %d (%d then %d)", gi, n0, n1);
            return SNAKE_E_CONFIG;
        }
        if (n1 - n0 > largest) largest = n1 - n0;
        for (int n = n0; n < n1; n++) {
            if (p->node_act[n] < 0 || p->node_act[n] >= genome::kNumAct) {
                set_error("snake_genome_check: node_act %d of genome %d node %d is not an activation id (0..%d)",
                          p->node_act[n], gi, n - n0, genome::kNumAct - 1);
                return SNAKE_E_CONFIG;
            }
            const int slot = I + (n - n0);
            for (int l = p->link_off[n]; l < p->link_off[n + 1]; l++) {
                if (p->link_src[l] < 0 || p->link_src[l] >= slot) {
                    set_error("snake_genome_check: link_src %d of genome %d node %d (slot %d) is not below its node's slot",
                              p->link_src[l], gi, n - n0, slot);
                    return SNAKE_E_CONFIG;
                }
            }
        }
        for (int a = 0; a < A; a++) {
            const int s = p->out_slot[(int64_t)gi * A + a];
            if (s < -1 || s >= I + (n1 - n0)) {
                set_error("snake_genome_check: out_slot %d of genome %d output %d is outside [-1, %d)", s, gi, a,
                          I + (n1 - n0));
                return SNAKE_E_CONFIG;
            }
        }
    }
    if (largest != cfg->max_nodes) {
        set_error("snake_genome_check: max_nodes is %d, the largest genome has %d nodes", cfg->max_nodes, largest);
        return SNAKE_E_CONFIG;
    }
    return SNAKE_OK;
}

extern "C" int64_t snake_genome_tiles(const snake_genome_cfg *cfg, const int32_t *node_off,
                                      const int32_t *genome_of_env, int64_t num_envs, int32_t num_snakes,
                                      int32_t *rows, snake_genome_tile *tiles, int64_t tile_cap)
{
    if (num_envs < 0 || num_envs > (1ll << 26) || num_snakes < 1 || num_snakes > kMaxSnakes) {
        set_error("snake_genome_tiles: num_envs must be in [0, 2^26] and num_snakes in [1, %d] (got %lld, %d)",
                  kMaxSnakes, (long long)num_envs, num_snakes);
        return SNAKE_E_ARG;
    }
    snake_genome_layout lay;
    if (int rc = genome::layout_of(cfg, num_envs * num_snakes, &lay)) return rc;
    if (!node_off || !genome_of_env || !rows) { set_error("snake_genome_tiles: NULL array"); return SNAKE_E_ARG; }
    const int G = cfg->num_genomes, W = lay.tile_rows;
    // counting sort of the envs by genome, stable; begin[g]: first env of genome g
    int64_t *begin = (int64_t *)calloc((size_t)G + 1, sizeof(int64_t));
    if (!begin) { set_error("snake_genome_tiles: out of memory"); return SNAKE_E_ARG; }
    int64_t rc = SNAKE_OK;
    for (int64_t e = 0; e < num_envs && rc == SNAKE_OK; e++) {
        if (genome_of_env[e] < 0 || genome_of_env[e] >= G) {
            set_error("snake_genome_tiles: genome_of_env[%lld] = %d is outside [0, %d)", (long long)e,
                      genome_of_env[e], G);
            rc = SNAKE_E_CONFIG;
        } else {
            begin[genome_of_env[e] + 1]++;
        }
    }
    int64_t nt = 0, ns = 0;
    if (rc == SNAKE_OK) {
        for (int gi = 0; gi < G; gi++) begin[gi + 1] += begin[gi];
        for (int64_t e = num_envs - 1; e >= 0; e--) {       // (backwards over counts turned into ends: stable)
            const int64_t at = --begin[genome_of_env[e] + 1];
            for (int s = 0; s < num_snakes; s++) rows[at * num_snakes + s] = (int32_t)(e * num_snakes + s);
        }
        // after the pass begin[g + 1] is genome g's first env
        for (int gi = 0; gi < G && rc == SNAKE_OK; gi++) {
            const int64_t r0 = begin[gi + 1] * num_snakes;
            const int64_t r1 = (gi + 1 < G ? begin[gi + 2] : num_envs) * num_snakes;
            const int nodes = node_off[gi + 1] - node_off[gi];
            if (nodes < 0 || nodes > cfg->max_nodes) {
                set_error("snake_genome_tiles: genome %d has %d nodes, max_nodes is %d", gi, nodes, cfg->max_nodes);
                rc = SNAKE_E_CONFIG;
                break;
            }
            for (int64_t r = r0; r < r1; r += W) {
                if (tiles) {
                    if (nt >= tile_cap) {
                        set_error("snake_genome_tiles: more than tile_cap = %lld tiles", (long long)tile_cap);
                        rc = SNAKE_E_ARG;
                        break;
                    }
                    snake_genome_tile &t = tiles[nt];
                    t.genome = gi;
                    t.count = (int32_t)(r1 - r < W ? r1 - r : W);
                    t.row_start = (int32_t)r;
                    t.scratch = nodes > lay.lds_nodes ? (int32_t)ns : -1;
                }
                if (nodes > lay.lds_nodes) ns++;
                nt++;
            }
        }
    }
    free(begin);
    return rc == SNAKE_OK ? nt : rc;
}

extern "C" int snake_genome_actions(const snake_genome_cfg *cfg, const snake_genome_prog *prog,
                                    const snake_genome_tile *tiles, const int32_t *rows, int64_t num_tiles,
                                    const float *features, const uint8_t *skip, int8_t *actions, double *outputs,
                                    void *scratch, int64_t num_rows, void *stream)
{
    snake_genome_layout lay;
    if (int rc = genome::layout_of(cfg, num_rows, &lay)) return rc;
    if (num_tiles < 0 || num_tiles > lay.max_tiles) {
        set_error("snake_genome_actions: num_tiles must be in [0, %lld] for %lld rows (got %lld)",
                  (long long)lay.max_tiles, (long long)num_rows, (long long)num_tiles);
        return SNAKE_E_ARG;
    }
    if (num_tiles == 0) return SNAKE_OK;
    if (!prog || !tiles || !rows || !features || !actions || !prog->node_off || !prog->link_off || !prog->out_slot) {
        set_error("snake_genome_actions: NULL buffer");
        return SNAKE_E_ARG;
    }
    if (lay.scratch > 0 && !scratch) {
        set_error("snake_genome_actions: a genome of %d nodes needs the scratch buffer (%lld bytes)", cfg->max_nodes,
                  (long long)lay.scratch);
        return SNAKE_E_ARG;
    }
    genome::Args g;
    g.p = *prog;
    g.tiles = tiles;
    g.rows = rows;
    g.features = features;
    g.skip = skip;
    g.actions = actions;
    g.outputs = outputs;
    g.scratch = lay.scratch > 0 ? (double *)scratch : nullptr;
    g.I = cfg->num_inputs;
    g.A = cfg->num_outputs;
    g.W = lay.tile_rows;
    g.max_nodes = cfg->max_nodes;
    const hipStream_t s = (hipStream_t)stream;
    DeviceGuard dg(s);
    if (dg.dev < 0) return SNAKE_E_LAUNCH;
    hipLaunchKernelGGL(genome::k_genome_actions, dim3((unsigned)num_tiles), dim3(64), (size_t)lay.lds_bytes, s, g);
    return launch_status("k_genome_actions");
}
