/*
 * snake_env.h -- C-ABI of the MI355X-native batched multi-snake environment.
 *
 * The drop-in boundary for the reference's hot path (tranthai189765/MARL-Snake,
 * marlenv/marlenv/envs/snake_env.py SnakeEnv.reset/step, reached through
 * marlenv/marlenv/wrappers.py make_snake). The reference is pure Python, so its
 * "FFI" for this path is the Python method surface; the product's Python host
 * layer (marl-snake_amd/marlenv) binds these entry points with ctypes
 * (marl-snake_amd/marlenv/_native.py) and re-exposes make_snake()/reset()/step().
 *
 * Conventions
 *   - plain C types only; every buffer pointer is DEVICE memory allocated and
 *     owned by the caller (PyTorch); the library allocates nothing on the device.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls
 *     are stream-ordered and asynchronous; not re-entrant per state.
 *   - every launch runs on the stream's device (NULL: the device current at the
 *     call), whatever device the calling thread has current; that device is
 *     current again on return.
 *   - return 0 on success, a negative SNAKE_E* code on a bad argument (message in
 *     snake_last_error()), never abort.
 *   - env i of a batch is a standalone reference SnakeEnv after
 *     np.random.seed(base_seed + env_offset + i).
 */
#ifndef SNAKE_ENV_H
#define SNAKE_ENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNAKE_ABI_VERSION 20

#define SNAKE_OK           0
#define SNAKE_E_CONFIG    -1   /* invalid snake_cfg (message says which field) */
#define SNAKE_E_ARG       -2   /* NULL / mis-sized buffer, num_envs out of range */
#define SNAKE_E_LAUNCH    -3   /* HIP launch error (message has hipGetErrorString) */

/* Environment configuration. Mirrors SnakeEnv.__init__ kwargs
 * (snake_env.py:58-129) and the gym ids of envs/__init__.py:3-16. */
typedef struct {
    int32_t height, width;      /* grid incl. walls, 3..255 */
    int32_t num_snakes;         /* S, 1..16 */
    int32_t snake_length;       /* initial length L >= 2 */
    int32_t vision_range;       /* 0 == None (full-map obs), else crop (2vr+1)^2 */
    int32_t frame_stack;        /* fs >= 1, obs channels = 8*fs */
    int32_t observer;           /* 0 = 'snake' (actions 0/1/2), 1 = 'human' (0..4) */
    int32_t num_fruits;         /* 1..64; default round(0.8*S) (:87-88) */
    double  rew_fruit, rew_kill, rew_lose, rew_win, rew_time;   /* reward_dict */
    double  max_episode_steps;  /* 1e4 by default (:56) */
    int32_t coop;               /* 1 = SnakeCoop-v1: episode ends when ANY snake dies */
    int32_t autoreset;          /* 1 = reset an env inside snake_step when all its dones
                                   are True and return the reset obs (vector-env semantics,
                                   wrappers.py:139-145); 0 = return the terminal obs;
                                   2 = reset every env after every step (gym 0.23.1's
                                   worker behind make_snake, wrappers.py:212) */
    int32_t spawn_ahead;        /* spawn-ahead threshold (snake_step): 0 = default (at most
                                   3 live snakes, 4 on small background batches of at most
                                   8192 spawn poses, every env under coop), -1 = off, k >= 1 =
                                   envs with at most k live snakes. Never changes results. */
    int32_t spawn_background;   /* 1 = the spawn-ahead attempts run in a background kernel on a
                                   stream of the library's (two per state) that outlives snake_step (see
                                   snake_sync, snake_release), 0 = automatic (on for boards of
                                   more than 8192 spawn poses, e.g. 40x40, and for batches of
                                   at most 8192 envs and 64 MiB of observations per step),
                                   -1 = off (inside the step). Needs spawn-ahead on and a draw record that fits LDS
                                   (at most 18 368 spawn poses). Never changes results. */
} snake_cfg;

/* Byte sizes of every caller-allocated buffer for num_envs envs (snake_plan). */
typedef struct {
    int64_t grid;       /* uint8  [N][fs][grid_stride]   grid ring (newest = env[2]) */
    int64_t snake;      /* int32  [N][S][4]              packed snake records: head/tail cells; heading,
                                                         alive, pending ring-word directions; ring head and
                                                         length; tail-direction queue (see k_logic) */
    int64_t body;       /* uint8  [N][S][ring_cap]       direction deques (rings), ring_cap >= 16 */
    int64_t env;        /* int32  [N][8]                 alive_snakes, episode_length, cur, mt_pos
                                                         (> 624: the key's twist is pending, position
                                                         624 + j = word j of the next key),
                                                         spawn-ahead status word (bits 0-1: 0 none,
                                                         1 partial, 2 ready, 3 being drawn by a background
                                                         job; bits 2-3: which of the env's four
                                                         records holds it (background spawn-ahead, one per
                                                         queue set); bits 4-31: the record's generation),
                                                         spawn failure (1: the last reset gave up, below);
                                                         words 6-7 unused */
    int64_t ctr;        /* uint16 [N][fs][S]             crop centre (r<<8|c) of each grid ring slot */
    int64_t stats;      /* snake_epi_stat [N][S]         running episode score/steps/fruits/kills */
    int64_t mt;         /* uint32 [N][624]               per-env MT19937 key */
    int64_t cand;       /* int16  [n_cand][L]            spawn-pose table (cell indices) */
    int64_t jscratch;   /* uint32 [min(N,2048)][round4(n_cand)+64] reset link tables, 0 when the
                                                         u16 draw record fits LDS (2*n_cand <= 36 KB)
                                                         and the board's auto-resets do not run beside
                                                         four-wave lean encodes (k_post_lean) */
    int64_t spawn;      /* uint32 [N][672]               spawn-ahead record: MT key, MT pos and the
                                                         S*L spawn cells (u16) of the env's next reset
                                                         ([4][N][672] with background spawn-ahead) */
    int64_t resetq;     /* int32  4 x ([3][64][cap] + [227*32]) sharded auto-reset and spawn-ahead
                                                         queues + the step's counters, one per 128-B
                                                         line; four sets, by step count mod 4; then the
                                                         fused step's flags and hand-off records
                                                         (zero-initialised) */
    int64_t obs;        /* uint8  [N][S][h][w][8*fs]     NHWC observations */
    int64_t rew;        /* double [N][S] */
    int64_t done;       /* uint8  [N][S] */
    int64_t ep_done;    /* uint8  [N]                    1 when the step ended the episode */
    int64_t rank;       /* int32  [N][S]                 info['rank'] where ep_done (elsewhere not written) */
    int64_t ep_stats;   /* double [N][4][S]              info episode_* where ep_done (elsewhere not written) */
    int64_t err;        /* int32  [N]                    1 = invalid action (reference KeyError: the
                                                         env is left unchanged, its rew/done are 0);
                                                         2 = its auto-reset gave up (below) */
    int64_t n_cand;     /* rows of the spawn-pose table */
    int32_t obs_h, obs_w, obs_c;
    int32_t grid_stride, ring_cap;
} snake_layout;

/* Running episode statistics of one snake (_reset_epi_stats, snake_env.py:
 * 385-389, 438-442): the score in float64 as the reference sums it; steps,
 * fruits and kills are the reference's integer-valued float64 sums held as
 * integers (fruits < 65536: a snake's length is bounded by the board; kills
 * <= num_snakes: every kill credit is a death in the episode). */
typedef struct {
    double   score;
    uint32_t steps;
    uint16_t fruits, kills;
} snake_epi_stat;

typedef struct {        /* device state buffers (layouts in snake_layout) */
    uint8_t  *grid;
    int32_t  *snake;
    uint8_t  *body;
    int32_t  *env;
    uint16_t *ctr;
    snake_epi_stat *stats;
    uint32_t *mt;
    const int16_t *cand;
    uint32_t *jscratch; /* may be NULL when layout.jscratch == 0 */
    uint32_t *spawn;
    int32_t  *resetq;   /* zero-initialised once by the caller */
} snake_state;

typedef struct {        /* device output buffers of one step/reset */
    uint8_t *obs;
    double  *rew;
    uint8_t *done;
    uint8_t *ep_done;
    int32_t *rank;
    double  *ep_stats;
    int32_t *err;
} snake_out;

/* Validate cfg and compute buffer sizes. Replaces SnakeEnv.__init__'s checks and
 * observation_space shape (snake_env.py:58-129). Also rejects boards on which S
 * random spawn poses are disjoint in fewer than 2e-4 of the draws (estimated by
 * sampling): the reference's _generate_snakes retries forever (:576-589), a reset
 * here gives up after 2^16 permutations -- sets env word 5 (and err = 2 for an
 * auto-reset) -- which the bound keeps below ~2e-6 per reset. */
int snake_plan(const snake_cfg *cfg, int64_t num_envs, snake_layout *out);

/* Which kernel variants snake_step takes for (cfg, num_envs): the launch plan's
 * path choices, so that a test can assert the path it means to cover. Host
 * only: needs no device and launches nothing. The per-step observation encode
 * is described; a reset (snake_reset, and an auto-reset inside the step)
 * always writes its observation with the direct encode. Without the all-done
 * auto-reset (cfg->autoreset 0 or 2) the step encodes in k_encode, one env per
 * wave, staged rows or direct only. */
typedef struct {
    int32_t encode;         /* per-step encode: 0 direct (one wave, no staging: more than 8 KB of
                               observation per snake), 1 staged rows (groups of whole snakes through
                               an LDS buffer of at most 8 KB), 2 table (one wave per 4 envs, k_post),
                               3 lean (four-wave workgroups, k_post_lean), 4 lean + table */
    int32_t enc_group;      /* staged rows: snakes per staged group (< num_snakes: several groups,
                               the last one possibly partial); 0 with the direct encode; what
                               k_encode would use where the step takes the table or lean encode */
    int32_t units;          /* 8-byte observation units per env: S * h * w * frame_stack (odd:
                               8-byte stores instead of 16-byte ones) */
    int32_t enc_per_wave;   /* envs per encode wave (lean: per workgroup) */
    int32_t enc_wpb;        /* table encode: independent encode waves per workgroup */
    int32_t desc_in_lds;    /* table encode: the unit descriptors are read from LDS (else registers) */
    int32_t fused;          /* the one-launch step (k_step) is eligible (snake_debug_set "fused") */
    int32_t background;     /* spawn-ahead attempts run in the background kernel (k_spawn) */
    int32_t link;           /* the reset workers' permutation record: 0 global link tables,
                               1 u16 draw record in LDS, 2 u32 link table in LDS */
    int32_t logic_lanes;    /* k_logic: lanes per env (4, 8 or 16) */
    int32_t logic_wpb;      /* k_logic: waves per workgroup (4 or 1) */
} snake_paths;

int snake_plan_paths(const snake_cfg *cfg, int64_t num_envs, snake_paths *out);

/* Host-side spawn-pose table = dfs_sweep_empty(make_grid(H, W), L) in reference
 * order (grid_util.py:73-115), as int16 cell indices r*W+c, n_cand x L. Static per
 * (H, W, L): computed once, uploaded once. Returns n_cand, or < 0. */
int64_t snake_build_candidates(const snake_cfg *cfg, int16_t *host_out, int64_t capacity);

/* Seed env i's MT19937 with base_seed + env_offset + i (np.random.seed,
 * snake_env.py:581 / grid_util.py:130 use the global legacy RandomState). */
int snake_seed(const snake_cfg *cfg, const snake_state *st, int64_t num_envs,
               uint32_t base_seed, int64_t env_offset, void *stream);

/* SnakeEnv.reset() (snake_env.py:131-159) for every env whose env_mask byte is
 * nonzero (env_mask == NULL: all envs); writes out->obs for those envs. With
 * spawn-ahead on (autoreset on all-done, cfg->spawn_ahead != -1) each reset env
 * also gets the spawn poses of its NEXT reset drawn into its spawn record (up to
 * 4 permutation attempts: status ready, else partial), see snake_step. */
int snake_reset(const snake_cfg *cfg, const snake_state *st, int64_t num_envs,
                const uint8_t *env_mask, const snake_out *out, void *stream);

/* SnakeEnv.step(actions) (snake_env.py:301-414) for all envs at once; actions is
 * int8 [N][S]. With cfg->autoreset an env whose dones are all True is reset in
 * the same call and its out->obs holds the reset observation. Launches, all on
 * `stream`: k_logic (the game rules of every env, queueing the auto-resets),
 * then k_post, whose first blocks are the reset workers and the rest the encodes
 * of every other env's observation (k_post_lean: four workers per workgroup, then
 * four-wave lean encodes, for boards with rings of 513-2048 dwords such as 40x40
 * with 4 frames). Background spawn-ahead adds k_spawn on the library's stream
 * for the state (snake_sync). Without autoreset: k_logic, k_encode; every-step
 * autoreset: k_logic, k_autoreset, k_encode.
 *
 * Spawn-ahead: a reset's spawn poses depend only on the env's MT19937 state, which
 * changes only at fruit respawns and resets. With autoreset, k_logic also queues
 * every env that is close to the end of its episode (at most 2 snakes alive, or
 * any env under coop) and has no ready record for its current MT state, and the
 * k_autoreset workers, after the step's resets, run one permutation attempt of
 * that env's NEXT reset into its spawn record (st->spawn). A later reset of the
 * env starts from the record (MT key, position, poses) when no draw has touched
 * the MT state since; a fruit respawn or a reset invalidates it. Results are
 * identical with or without it (it only moves draws off the step's critical
 * path); cfg->spawn_ahead = -1 disables it. A caller that
 * rewrites an env's MT key or position itself must zero that env's status word
 * (env word 4), after snake_sync. */
int snake_step(const snake_cfg *cfg, const snake_state *st, int64_t num_envs,
               const int8_t *actions, const snake_out *out, void *stream);

/* With background spawn-ahead (cfg->spawn_background) a spawn kernel of the
 * last snake_step may still be running when the call returns; it writes only
 * st->spawn and env word 4, and the next snake_step / snake_reset / snake_seed
 * order themselves after it. Before the caller reads or writes the state
 * buffers itself (snapshots, set_mt_state, freeing them), snake_sync makes
 * `stream` wait for it (a no-op without background work). */
int snake_sync(const snake_cfg *cfg, const snake_state *st, int64_t num_envs, void *stream);

/* Releases what the library keeps for this state (the background spawn-ahead
 * stream and events, created by its first snake_step): waits for its last
 * spawn kernel on the host, then destroys them. Call before freeing the state
 * buffers; a later snake_step on the same buffers creates them afresh. */
int snake_release(const snake_cfg *cfg, const snake_state *st, int64_t num_envs);

/* RGB image of every env's current grid: rgb_from_grid(grid, Cell, CellColors)
 * (grid_util.py:164-175), the frame of SnakeEnv.render('rgb_array') and of the
 * 'gif' frames via image_from_grid (snake_env.py:284-293). palette is HOST
 * memory, uint8 [6][16][3]: the colour of a cell of code v % 10 owned by snake
 * v / 10, i.e. CellColors[code][id % len] * 0.7 ** (id // len) truncated to
 * uint8 (snake.py:14-30), precomputed by the caller with the reference's own
 * arithmetic. rgb is device uint8 [N][H][W][3]. */
int snake_render_rgb(const snake_cfg *cfg, const snake_state *st, int64_t num_envs,
                     const uint8_t *palette, uint8_t *rgb, void *stream);

/* Profiling aid. While enabled, every kernel launch of snake_step / snake_reset
 * is bracketed by timing events on its own stream. snake_timing_read returns the
 * summed device time (ms) and the launch count of one kernel ("k_logic",
 * "k_post", "k_autoreset", "k_encode", "k_spawn", "k_reset") since its last read, and the number of
 * auto-resets run (kernel "resets": count only, every step); it waits for the
 * events. "resets_timed", "spawn_hits" and "spawn_jobs" count, while enabled,
 * the auto-resets, those that started from a ready spawn-ahead record and the
 * spawn-ahead attempts run; "spawn_void", "reset_partial", "respawn_slow",
 * "respawn_slow2", "gate_shut", "draw_wait" (resets that found a background job
 * drawing their record and waited) and "draw_timeout" (... and gave up waiting,
 * drawing from the env's own MT state) are further diagnostic counts. */
int snake_timing_enable(int on);
int snake_timing_read(const char *kernel, double *total_ms, int64_t *count);

/* Testing aid (no reference counterpart), process-wide, read at each
 * snake_step: "draw_wait_ticks" = how long (100 MHz ticks, default 200000 =
 * 2 ms) an auto-reset waits for a background spawn-ahead job drawing its record
 * before it voids the job and draws itself (0: never waits); "spawn_delay_ticks"
 * = fault injection: each background job sleeps that long (default 0) once it
 * has marked a record DRAWING, so resets meet jobs in flight; "fused" = 1 runs
 * the step as one launch (k_step) where the configuration allows it (one
 * frame, at most 4 snakes, table encode, in-step spawn-ahead; default 0);
 * "fuse_roles" = which of k_step's roles run (diagnostics; 7 = all). Results
 * are the same for any values of the first three. Returns SNAKE_E_ARG for an unknown name or a value out of
 * range. */
int snake_debug_set(const char *name, long long value);

/* ---- Fused consumer: the reference's DQN forward on the observation batch
 * (train_dqn.py:104-151 DQN.forward / forward_features, train_ga.py:60-100),
 * conv1 c->32, conv2 32->64, conv3 64->64 (3x3, pad 1, ReLU), NCHW flatten,
 * fc1 64hw->256, fc2 256->128 (ReLU), fc3 128->A, on the bf16 matrix cores with
 * fp32 accumulation. The five GEMMs conv1, conv2, conv3, fc1 and fc2 run on
 * v_mfma_f32_16x16x32_bf16: Y[m][n] = sum_k act(X)[m][k] * W[n][k] on bf16
 * operands, products exact, sums fp32. The rounding points are those of
 * snake_dqn32_forward_bf16 below; only the place differs (a value is rounded
 * as it is stored, not as it is staged):
 *   rounded      relu(Y + b) of conv1, conv2, conv3 and fc1, formed in fp32 and
 *                rounded to bf16, to nearest even, as it is stored (in LDS, or
 *                conv3's in act_scratch); the input byte becomes a bf16 value
 *                (exact); the weights are bf16 already, rounded to nearest even
 *                by the pack (snake_dqn_pack32)
 *   not rounded  the biases (fp32); the fp32 accumulators; relu(fc2 + b) =
 *                feat_out, fp32; fc3, in fp32 on those fp32 features and fp32
 *                weights
 *   input bytes  a byte is read at its value 0..255: the reference's /255
 *                branch does not exist here, the functions are for the env's
 *                0/1 observations
 * tests/test_dqn_round_gpu.py holds both functions to a float64 model of
 * exactly these points, bit for bit (tests/learner_model.py, the model of
 * snake_dqn32_forward_bf16 too; cases in tests/dqn_round_cases.py).
 * obs: uint8 [B][h][w][c] (the env's NHWC per-snake observations). h = w =
 * 2*vision_range+1 with vision_range in [1, 5], c = 8*frame_stack <= 32,
 * A <= 4. */
typedef struct {
    int32_t height, width, channels, num_actions;
    int32_t conv_waves;     /* waves per observation in the conv kernel: 1, 2, 4; 0 = default (4,
                             * or 2 when the row-tile count is odd; SNAKE_DQN_WAVES overrides 0);
                             * the map path (snake_dqn_map_*): 8, 16; 0 = default (16) */
} snake_dqn_cfg;

typedef struct {        /* sizes for snake_dqn_forward (element counts) */
    int64_t conv1_w;    /* bf16 B[32][k1]: k = tap*cpad + channel, tap = ky*3 + kx, zero padded */
    int64_t conv2_w;    /* bf16 B[64][288]: k = tap*32 + channel */
    int64_t conv3_w;    /* bf16 B[64][576]: k = tap*64 + channel; all three stored in MFMA
                         * fragment order: element (o, k) at
                         * ((o/16 * K/32 + k/32) * 4 + (k%32)/8) * 128 + (o%16) * 8 + k%8 */
    int64_t fc1_w;      /* bf16 [256][64*p16], k in conv3's MFMA fragment order:
                         * k = m*1024 + half*512 + quad*128 + c16*8 + j*4 + r holds
                         * channel (2*half + j)*16 + c16 at GEMM row i = m*16 + 4*quad + r,
                         * i.e. at observation position snake_dqn_rows()[i] (zero weights
                         * where that is -1) */
    int64_t fc2_w;      /* bf16 [128][256] */
    int64_t act_per_obs;/* bf16 scratch per observation: 64*p16 */
    int32_t cpad, p16, k1;   /* channels padded to a power of two >= 8; GEMM rows (16 per tile); 9*cpad to 32 */
    int32_t lds_conv;   /* LDS bytes per conv workgroup */
} snake_dqn_layout;

typedef struct {        /* device weights (layouts in snake_dqn_layout; biases and fc3 fp32) */
    const uint16_t *conv1_w, *conv2_w, *conv3_w, *fc1_w, *fc2_w;
    const float *conv1_b, *conv2_b, *conv3_b, *fc1_b, *fc2_b;
    const float *fc3_w;  /* [A][128] */
    const float *fc3_b;  /* [A] */
} snake_dqn_net;

int snake_dqn_plan(const snake_dqn_cfg *cfg, snake_dqn_layout *out);

/* The convolutions' GEMM row -> observation position map (p = y*w + x, -1 for a
 * padding row): rows[i] for i < p16. Rows are assigned so that the 16 rows of a
 * tile sit in distinct LDS banks (dqn_kernels.hip). Returns p16 (rows may be
 * NULL to query it), < 0 on error. */
int64_t snake_dqn_rows(const snake_dqn_cfg *cfg, int32_t *rows, int64_t n);

/* q_out: float [B][A]; feat_out (may be NULL): float [B][128] = forward_features;
 * act_scratch: bf16 [B][act_per_obs] device buffer. Two launches on `stream`, on
 * the stream's device. */
int snake_dqn_forward(const snake_dqn_cfg *cfg, const snake_dqn_net *net, const uint8_t *obs,
                      int64_t batch, uint16_t *act_scratch, float *q_out, float *feat_out,
                      void *stream);

/* The map path of the bf16 forward: the same network, layouts and roundings on
 * any h x w observation (rectangular included) with (h+2)*(w+2) <= 576, i.e. up
 * to 22x22 (train_dqn.py's 20x20 full map: 26 row tiles, p16 = 416), c in {8,
 * 16, 24, 32}, A <= 4. cfg->conv_waves: waves per workgroup of its convolution
 * kernel, 8 or 16; 0 = default (16). One workgroup runs one observation at a
 * time and loops over the row tiles, so h and w are runtime values. Same
 * structs and argument lists as the three functions above, whose window path
 * (3x3 .. 11x11) stays the faster one where it applies. What the plan rejects
 * is SNAKE_E_CONFIG; larger maps take fp32 mode below. The forward's two
 * launches run on `stream`, on the stream's device. */
int snake_dqn_map_plan(const snake_dqn_cfg *cfg, snake_dqn_layout *out);
int64_t snake_dqn_map_rows(const snake_dqn_cfg *cfg, int32_t *rows, int64_t n);
int snake_dqn_map_forward(const snake_dqn_cfg *cfg, const snake_dqn_net *net, const uint8_t *obs,
                          int64_t batch, uint16_t *act_scratch, float *q_out, float *feat_out,
                          void *stream);

/* fp32 mode of the DQN consumer (dqn32_kernels.hip): the same network in fp32
 * arithmetic (fp32 matrix cores: exact fp32 products, fp32 sums) on any observation size (e.g. train_dqn.py's 20x20 full map,
 * :29-33), cfg->channels a multiple of 8, conv_waves ignored. Weights fp32,
 * row-major [out][in]: conv w [cout][9*cin] with k = (ky*3 + kx)*cin + ci;
 * fc1 [256][h*w*64] with column p*64 + ch (the reference's NCHW flatten
 * column ch*h*w + p, permuted once); fc2 [128][256]; fc3 [A][128]. The uint8
 * input is divided by 255 when the batch holds a value > 1 (train_dqn.py:122). */
typedef struct {
    const float *conv1_w, *conv2_w, *conv3_w, *fc1_w, *fc2_w, *fc3_w;
    const float *conv1_b, *conv2_b, *conv3_b, *fc1_b, *fc2_b, *fc3_b;
} snake_dqn32_net;

/* Device scratch bytes snake_dqn32_forward needs for `batch` observations (< 0 on error). */
int64_t snake_dqn32_scratch(const snake_dqn_cfg *cfg, int64_t batch);

/* q_out: float [B][A]; feat_out (may be NULL): float [B][128]. Seven launches on
 * `stream`, on the stream's device. */
int snake_dqn32_forward(const snake_dqn_cfg *cfg, const snake_dqn32_net *net, const uint8_t *obs,
                        int64_t batch, void *scratch, float *q_out, float *feat_out, void *stream);

/* ---- The learner: train_dqn.py's Trainer.update_model (:228-257) on the
 * device, in fp32 (dqn_train_kernels.hip). No call below syncs with the host,
 * no kernel uses a floating-point atomic: every sum has a fixed order that
 * depends on the shapes alone, results are bitwise reproducible.
 *
 * snake_dqn32_backward: the gradients of sum(dq * Q) with respect to the twelve
 * parameters, for the batch a preceding snake_dqn32_forward ran.
 *   fwd_scratch    that forward's scratch (same cfg, obs, batch and weights): the
 *                  pre-activations Y1..Y5 and the x.max() > 1 flag; read only
 *   dq             float [B][A], any gradient with respect to the Q-values
 *   train_scratch  snake_dqn32_train_scratch(cfg, batch) bytes, 16-byte aligned:
 *                  dY5 [B][128] | dY4 [B][256] | dY3, dY2 [B*h*w][64] | dY1
 *                  [B*h*w][32] (gradients with respect to the pre-activations,
 *                  NHWC) | the weight-gradient partials | the bias partials
 *   grad           a snake_dqn32_net whose twelve pointers are WRITTEN (the
 *                  const is cast away): the weights' own layouts, i.e. conv
 *                  [cout][(ky*3 + kx)*cin + ci], fc1 [256][p*64 + ch]; every
 *                  element is overwritten, nothing accumulates across calls.
 *                  Weights and gradients 16-byte aligned.
 * A ReLU's mask is Y + bias > 0; conv1's weight gradient reads the uint8
 * observation as the forward did (divided by 255 when the flag is set).
 * Weight gradients dW[n][k] = sum_m dY[m][n] act(X)[m][k] and the convolutions'
 * and fc1/fc2's input gradients run on the fp32 matrix cores on every geometry
 * snake_dqn32_forward accepts (the conv input gradient in gather form); fc3 on
 * the vector ALUs. Split M: the M = B*h*w (fc: B) rows of a weight or bias
 * gradient are cut into chunks of max(2048, ceil(M/128) rounded up to 16) rows;
 * with more than one chunk each writes a partial and a second kernel adds the
 * partials in chunk order. batch in [0, 2^24]. Every launch on `stream`, on the
 * stream's device. */
int64_t snake_dqn32_train_scratch(const snake_dqn_cfg *cfg, int64_t batch);   /* bytes, < 0 on error */
int snake_dqn32_backward(const snake_dqn_cfg *cfg, const snake_dqn32_net *net, const uint8_t *obs,
                         int64_t batch, const void *fwd_scratch, const float *dq, void *train_scratch,
                         const snake_dqn32_net *grad, void *stream);

/* snake_dqn32_backward in bf16 mixed precision (dqn_train16_kernels.hip): the
 * same arguments, preconditions, return codes, scratch layout and split-M rule,
 * the same operand sources (the fp32 forward's scratch, the uint8 observation,
 * the fp32 weights, the fp32 dY buffers of train_scratch). The five weight
 * gradients and four input gradients of the matrix cores run on
 * v_mfma_f32_16x16x32_bf16: every element of a GEMM operand is rounded to bf16
 * when it is staged, products are exact and sums are fp32. bf16(v) is round to
 * nearest even on v's bit pattern (torch's .to(bfloat16)); a NaN keeps its sign
 * and top mantissa bits and gets the quiet bit. Exactly these are rounded:
 *   weight gradient  dW[n][k] = sum_m bf16(dY[m][n]) * bf16(act(X)[m][k]),
 *                    act(X) formed in fp32 first: relu(Y + b), or the byte, or
 *                    byte / 255 when the flag is set
 *   input gradient   dX[m][k] = (sum_r bf16(dY[..][r]) * bf16(W[r][k])) * mask
 * and these are not:
 *   the mask Y + bias > 0 (fp32, as above);
 *   dX as it is stored: the fp32 sum, unrounded (dY1..dY4 in train_scratch hold
 *   fp32 values; the next GEMM rounds them when it stages them);
 *   the bias gradients: db[n] = sum_m dY[m][n] over the unrounded fp32 dY, in a
 *   fixed order that depends on the shape alone;
 *   fc3 (weight, bias and input gradient, so dY5) and the sums of the split-M
 *   partials: the fp32 function's kernels, bit-equal to it.
 * No floating-point atomics; results are bitwise reproducible. Every launch on
 * `stream`, on the stream's device. */
int snake_dqn32_backward_bf16(const snake_dqn_cfg *cfg, const snake_dqn32_net *net, const uint8_t *obs,
                              int64_t batch, const void *fwd_scratch, const float *dq, void *train_scratch,
                              const snake_dqn32_net *grad, void *stream);

/* snake_dqn32_forward in bf16 mixed precision (dqn_fwd16_kernels.hip), the
 * learner's training forward: the same arguments, preconditions, return codes
 * and error texts as snake_dqn32_forward, on every geometry it accepts (no
 * dispatch by map width); batch == 0 returns SNAKE_OK. The weights are the fp32
 * masters, the activations are stored fp32.
 *   conv1, conv2, conv3, fc1 and fc2 run on v_mfma_f32_16x16x32_bf16:
 *     Y[m][n] = sum_k bf16(act(X)[m][k]) * bf16(W[n][k])
 *   act(X) is formed in fp32 first, exactly as the fp32 forward and the bf16
 *   weight gradient form it: the byte, or byte / 255 when the flag is set;
 *   relu(Y_prev + b_prev) otherwise (zero outside the map). bf16() is round to
 *   nearest even, the hardware's v_cvt_pk_bf16_f32, as in
 *   snake_dqn32_backward_bf16. Products are exact and sums are fp32.
 * Not rounded: Y as it is stored (the fp32 sum); the biases; the flag kernel;
 * fc3 (the fp32 forward's kernel on fp32 relu(Y5 + b) and fp32 weights);
 * feat_out = relu(Y5 + b) in fp32.
 * Scratch: snake_dqn32_forward_bf16_scratch(cfg, batch) bytes >=
 * snake_dqn32_scratch(cfg, batch). It begins with exactly snake_dqn32_forward's
 * layout -- the flag (16 bytes), then Y1..Y5, fp32 pre-activations without
 * bias, NHWC -- so snake_dqn32_backward and snake_dqn32_backward_bf16 take it
 * as fwd_scratch unchanged; fc1's split-K partials follow.
 * Split K: the K reduction steps of fc1 (K = 64 h w) and fc2 (K = 256) are cut
 * into chunks of max(1024, ceil(K / 16) rounded up to 64) steps; with more than
 * one chunk each writes a partial [chunk][B][N] and a second kernel adds the
 * partials in chunk order. The rule depends on K alone: a row's results do not
 * depend on the batch it is in. No floating-point atomics; every summation
 * order is a function of the shape alone, results are bitwise reproducible.
 * Every launch on `stream`, on the stream's device. */
int64_t snake_dqn32_forward_bf16_scratch(const snake_dqn_cfg *cfg, int64_t batch);   /* bytes, < 0 on error */
int snake_dqn32_forward_bf16(const snake_dqn_cfg *cfg, const snake_dqn32_net *net, const uint8_t *obs,
                             int64_t batch, void *scratch, float *q_out, float *feat_out, void *stream);

/* The TD loss (:243-250), one launch on `stream`, on the stream's device. Per
 * row b, in fp32 and in this order:
 *   target = reward[b] + ((1 - done[b]) * gamma) * max_a next_q[b][a]
 *   d      = q[b][action[b]] - target
 * loss_out (one float) = (sum_b smooth_l1(d)) / B with smooth_l1(d) = 0.5 d^2
 * for |d| < 1, else |d| - 0.5; dq [B][A] = clamp(d, -1, 1) / B at a = action[b],
 * 0 elsewhere. q, next_q float [B][A]; action int64 [B]; reward, done float
 * [B]. An action outside [0, A) is clamped into it and sets *err to 1 (err may
 * be NULL; the caller zeroes it). batch in [1, 2^24], num_actions in [1, 64]. */
int snake_dqn_td_loss(const float *q, const int64_t *action, const float *reward, const float *done,
                      const float *next_q, int64_t batch, int32_t num_actions, float gamma,
                      float *loss_out, float *dq, int32_t *err, void *stream);

/* clip_grad_norm_(params, max_norm) then optim.Adam.step() (torch defaults: no
 * amsgrad, no weight decay) over n elements; param, grad, exp_avg, exp_avg_sq
 * are flat float [n] device buffers (padding elements hold zero gradients and
 * stay unchanged). Three launches on `stream`, on the stream's device:
 *   norm  = sqrt(sum g^2)            two-stage, fixed order; also to *norm_out
 *   coef  = min(1, max_norm / (norm + 1e-6));  g' = g * coef  (grad is not written)
 *   m     = beta1 m + (1 - beta1) g';  v = beta2 v + ((1 - beta2) g') g'
 *   p     = p - step_size * (m / (sqrt(v) / sqrt(1 - beta2^step) + eps))
 * with step_size = lr / (1 - beta1^step); the two corrections are computed on
 * the host in double from the float arguments and rounded to float. step >= 1
 * is the count including this step. scratch: SNAKE_ADAM_SCRATCH_BYTES. */
#define SNAKE_ADAM_SCRATCH_BYTES 4112
int snake_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                    int64_t step, float lr, float beta1, float beta2, float eps, float max_norm,
                    void *scratch, float *norm_out, void *stream);

/* ---- The learner's weights in the bf16 forward's layouts (dqn_pack_kernels.hip):
 * a device-side conversion, so that a training loop acts (and forms its targets)
 * with snake_dqn_forward / snake_dqn_map_forward on the weights it is training.
 *   cfg, map_plan  the geometry and the plan whose layouts dst receives: 0 the
 *                  window plan (snake_dqn_plan), 1 the map plan
 *                  (snake_dqn_map_plan). Whatever that plan rejects is
 *                  SNAKE_E_CONFIG with the plan's message, before any launch.
 *   src            a net in the fp32 layouts above: conv [out][(ky*3 + kx)*cin +
 *                  ci], fc1 columns p*64 + ch, fc2 and fc3 row-major; read only
 *   dst            a snake_dqn_net whose twelve pointers are WRITTEN (the const
 *                  is cast away), sized by the plan's snake_dqn_layout: the conv
 *                  weights in MFMA fragment order, zero for channels in [C, cpad)
 *                  and for k in [9*cpad, k1); fc1 [256][64*p16] in conv3's
 *                  fragment order, zero in the GEMM rows whose rows[i] is -1 (or
 *                  anything else outside [0, h*w)); fc2 [128][256]; the five
 *                  biases, fc3_w and fc3_b copied as fp32. Every element of every
 *                  destination is written on every call: a packed net is a
 *                  snapshot of src, whatever the buffers held before.
 *   rows           p16 entries, the plan's own table (snake_dqn_rows /
 *                  snake_dqn_map_rows), in device memory
 * fp32 -> bf16 rounds to nearest even on the bit pattern, (u + 0x7fff + ((u >>
 * 16) & 1)) >> 16, as the forward rounds its activations; a NaN stays a NaN (its
 * bits are not pinned). src and dst must not overlap; the five weight tensors of
 * both are 16-byte aligned. One launch (k_dqn_pack) on `stream`, on the stream's
 * device; no atomics, no host sync.
 *
 * snake_dqn_pack32_host: the same conversion with every pointer a host pointer
 * (no alignment rule), as plain loops over the index mappings the kernel uses;
 * no device needed. */
int snake_dqn_pack32(const snake_dqn_cfg *cfg, int32_t map_plan, const snake_dqn32_net *src,
                     const snake_dqn_net *dst, const int32_t *rows, void *stream);
int snake_dqn_pack32_host(const snake_dqn_cfg *cfg, int32_t map_plan, const snake_dqn32_net *src,
                          const snake_dqn_net *dst, const int32_t *rows);

/* ---- Safe-action selection: the action rule of the reference's evaluator
 * (train_dqn.py:433-580 DQN_Evaluator.get_action, driven by the loop at
 * :625-646) for every env at once. Per env the snakes are taken in index order
 * with an empty set of claimed cells. A snake whose skip byte is nonzero gets
 * action 0 and keeps its direction. Otherwise its head is the first row-major
 * cell with channel 5 == 1 (none: action 0, direction (0,0)); an unknown
 * direction is read off the body cell behind the head (get_current_direction);
 * the moves are {0: (dy,dx), 1: (-dx,dy), 2: (dx,-dy)}; a move's Q-value is
 * masked to -inf when its target cell is outside the map, claimed by an earlier
 * snake of the env, deadly (channel 0, 2, 3, 4, 6 or 7 == 1), beside a cell
 * with channel 2 == 1, or opens into fewer reachable cells (flood fill, counted
 * up to fill_limit) than the snake is long; the action is the first argmax of
 * the masked values (all masked: 0), the direction becomes the chosen move and
 * head + move is claimed. Cells are in each snake's own observation
 * coordinates, as in the reference. NaN Q-values are outside the contract. */
typedef struct {
    int32_t obs_h, obs_w;   /* observation height and width, 1..64 */
    int32_t obs_c;          /* observation channels: 8 (frame_stack 1) */
    int32_t num_snakes;     /* S, 1..16 */
    int32_t fill_limit;     /* flood-fill cap, 1..4096; the reference's is 60 */
} snake_policy_cfg;

#define SNAKE_DIR_UNKNOWN (-128)   /* both bytes of a direction not known yet */

/* Validates cfg (host only, no device needed). */
int snake_policy_plan(const snake_policy_cfg *cfg);

/* obs: uint8 [N][S][h][w][8], 16-byte aligned; q: float [N][S][3]; skip: uint8
 * [N][S] or NULL (no snake skipped); dirs: int8 [N][S][2] (dy,dx), read and
 * updated in place; actions: int8 [N][S] out. One launch (k_safe_actions) on
 * `stream`, on the stream's device. */
int snake_safe_actions(const snake_policy_cfg *cfg, const uint8_t *obs, const float *q,
                       const uint8_t *skip, int8_t *dirs, int8_t *actions, int64_t num_envs,
                       void *stream);

/* ---- Greedy opponent: the rule-based fruit seeker of the reference's battle
 * mode (train_dqn.py:774-856 GreedyEnemy.get_action) for every snake at once,
 * each snake on its own observation alone (no claimed cells, no order among
 * the snakes). cfg is a snake_policy_cfg with the limits of snake_policy_plan;
 * fill_limit is validated but not used. A snake whose skip byte is nonzero
 * gets action 0 and keeps its direction. Otherwise its head is the first
 * row-major cell with channel 5 == 1; without one the action is 0 and the
 * direction stays as it is (unknown stays unknown). The target fruit is the
 * cell with channel 1 == 1 nearest to the head by |y-hy| + |x-hx|, the first
 * in row-major order among equals; there may be none. An unknown direction is
 * read off the head's neighbours in the order (-1,0), (1,0), (0,-1), (0,1):
 * the first one inside the map with channel 6 == 1 or channel 7 == 1 gives
 * direction = head - that cell; none gives (-1,0). (The evaluator's rule above
 * asks the neighbours in another order.) The moves are {0: (dy,dx), 1:
 * (-dx,dy), 2: (dx,-dy)}; a move is dead when its cell is outside the map or
 * has channel 0, 2, 3, 4, 6 or 7 == 1; a live move scores -(|y-fy| + |x-fx|)
 * from its cell to the target fruit, 0 without a fruit. All three dead: action
 * 0, the direction becomes move 0 (so a direction read off the body is
 * stored), rnd is not read. Otherwise, with best[] the n live moves of maximal
 * score in ascending order and u the snake's 32 random bits, the action is
 * best[((uint64_t)u * n) >> 32] and the direction becomes that move. The
 * reference draws with random.choice; here the random bits come in, so the
 * call is a pure function of its arguments.
 *
 * obs, skip, dirs, actions: as in snake_safe_actions; rnd: uint32 [N][S] or
 * NULL (all zero: the first best move). One launch (k_greedy) on `stream`, on
 * the stream's device. */
int snake_greedy_actions(const snake_policy_cfg *cfg, const uint8_t *obs, const uint32_t *rnd,
                         const uint8_t *skip, int8_t *dirs, int8_t *actions,
                         int64_t num_envs, void *stream);

/* ---- Graph observation: the ray-cast features of the reference's third env
 * id, SnakeGraph-v1 (graph_snake_env.py:47-103 GraphSnakeEnv._process_obs), for
 * every snake at once: 5 rays x obs_c values per snake, a pure function of the
 * observation tensor snake_step / snake_reset wrote and of the snake records
 * (st->snake, int32 [N][S][4]: word 0 = head row | head column << 8 | ..., word
 * 1 = direction (bits 0-1: 0 UP, 1 RIGHT, 2 DOWN, 3 LEFT) | alive << 8 | ...;
 * the other words are not read). Nothing that outlives snake_step writes
 * st->snake (the background spawn kernel writes st->spawn and env word 4 only),
 * so the call needs no snake_sync, only stream order after the step.
 *
 * A dead snake's 5 x obs_c values are zero. For a live snake, with n =
 * vision_range steps from the origin (vr, vr), the window's centre -- or, with
 * vision_range 0 (full-map observations), n = 5 steps from the snake's own head
 * cell -- and (dr, dc) the unit step of its direction ((-1,0), (0,1), (1,0),
 * (0,-1) for 0..3), ray k steps by
 *     0: F = (dr, dc)   1: L = (-dc, dr)   2: R = (dc, -dr)   3: F + L   4: F + R
 * and is, per channel, a float64 sum that starts at 0.0: for i = 0 .. n-1 in
 * order the cell origin + (i+1) * step is read; every channel whose byte is 1
 * adds w[i]; after that, if the cell's channel 0 is 1 (a wall in the oldest
 * frame of the stack) the ray ends -- the wall cell is counted. A cell outside
 * the observation ends the ray unread (the reference never gets there for a
 * live snake; the kernel reads nothing outside whatever the records hold).
 * w[i] = 1 / (i+1) for rays 0-2 and 1 / ((i+1) * sqrt(2.0)) for rays 3-4, as
 * the reference's arithmetic gives them: with a window its observation is
 * float64 and w[i] the float64 quotient; its full-map observation is float32
 * and w[i] = (double)(1.0f / (float)(i+1)), (double)(1.0f / (float)((i+1) *
 * sqrt(2.0))).
 *
 * source 0 ("own"): snake s reads observation s. source 1 ("reference"): the
 * reference indexes the observations with a counter of the LIVE snakes, so
 * live snake s reads observation k = the number of live snakes below s (with
 * the origin, for full maps, still s's own head): what GraphSnakeEnv returns,
 * live rows compacted, is this mode's live rows in index order. */
typedef struct {
    int32_t obs_h, obs_w;       /* observation height and width, 1..255; 2 * vision_range + 1 with a window */
    int32_t obs_c;              /* observation channels: 8 * frame_stack, 8..128 */
    int32_t num_snakes;         /* S, 1..16 */
    int32_t vision_range;       /* 0 == None (full-map observations), else 1..127 */
    int32_t source;             /* 0 own, 1 reference */
    int32_t out_f32;            /* 0: float64 out; 1: float out, the float64 result rounded once */
} snake_graph_cfg;

/* Validates cfg (host only, no device needed; SNAKE_E_CONFIG names the field). */
int snake_graph_plan(const snake_graph_cfg *cfg);

/* The weights of `steps` ray steps (1..127) as the kernel gets them: host_out
 * double [2][steps], row 0 rays 0-2, row 1 the diagonals; float32_quotient != 0
 * is the full-map arithmetic. Host only. */
int snake_graph_weights(int32_t steps, int32_t float32_quotient, double *host_out);

/* obs: uint8 [N][S][h][w][obs_c], 8-byte aligned; snake_records: int32
 * [N][S][4], 16-byte aligned; out: double (or float) [N][S][5][obs_c], 16-byte
 * aligned; num_envs in [0, 2^26] with num_envs * S * 5 * obs_c / 2 <= 2^31 (0:
 * no launch). One launch (k_graph_obs) on `stream`, on the stream's device;
 * reads obs and snake_records, writes every value of out. */
int snake_graph_obs(const snake_graph_cfg *cfg, const uint8_t *obs, const int32_t *snake_records,
                    void *out, int64_t num_envs, void *stream);

/* ---- Replay buffer: the reference trainer's deque of transitions
 * (train_dqn.py:89-100 ReplayBuffer, filled at :290-298, sampled at :228-240)
 * as rings in device memory, filled straight from one env step's tensors.
 *
 * Push. Snake (env, s) of the step is stored unless its skip byte is nonzero
 * (`if not dones[i]`, :291); the stored snakes are appended in (env, snake)
 * row-major order, which for one env is the reference's order. The stored
 * reward is (float)(r + p) with the sum in double: p = early_death_penalty when
 * the snake's done byte is nonzero, `step` is given and step[env] <
 * early_death_steps, else 0 (:292-295; the rounding is torch.tensor(...,
 * dtype=float32)'s at :238). done is stored as 0/1, the action as it is.
 * The rings have deque(maxlen=capacity) semantics: `count`, a device int64, is
 * the number of transitions ever stored and the only persistent counter; the
 * transition with sequence number q lives in slot q % capacity, size =
 * min(count, capacity), and logical index j in [0, size) -- the reference's
 * buffer[j], 0 the oldest -- is sequence number count - size + j. A call that
 * stores M > capacity transitions keeps the last `capacity` of them.
 * Observations are 0/1 bytes (the env's; any nonzero byte packs as 1) and are
 * stored bit-packed: the 8 channel bytes of one cell and frame, obs bytes
 * [8g, 8g + 8) of a snake's row, are byte g of its packed row (bit k = channel
 * k), h*w*obs_c/8 bytes per row at a 16-byte pitch.
 *
 * Gather. idx: int64 [B] logical indices, repeats allowed. An index is clamped
 * into [0, max(size, 1)): a caller's mistake cannot read outside the rings,
 * but an index outside [0, size) remains a contract violation. */
typedef struct {
    int32_t obs_h, obs_w;       /* observation height and width, 1..1024 */
    int32_t obs_c;              /* observation channels: 8 * frame_stack, 8..512 */
    int32_t num_snakes;         /* S, 1..16 */
    int64_t capacity;           /* transitions the rings hold, 1..2^40 */
    int32_t early_death_steps;  /* the reference's EARLY_DEATH_THRESHOLD (<= 0: never a penalty) */
    double  early_death_penalty;/* the reference's EARLY_DEATH_PENALTY */
} snake_replay_cfg;

typedef struct {        /* byte sizes of the caller's device buffers */
    int64_t state, next_state;  /* uint8 [capacity][pitch]: packed rows; zero them once */
    int64_t action;             /* int8 [capacity] */
    int64_t reward;             /* float [capacity] */
    int64_t done;               /* uint8 [capacity] */
    int64_t count;              /* one int64, zero = empty */
    int64_t scratch;            /* snake_replay_push's scratch for num_envs envs (contents need not survive a call) */
    int32_t packed_row, pitch;  /* h*w*obs_c/8, and that rounded up to 16 */
} snake_replay_layout;

typedef struct {        /* device buffers, sized by snake_replay_plan */
    uint8_t *state, *next_state;
    int8_t *action;
    float *reward;
    uint8_t *done;
    int64_t *count;
} snake_replay_rings;

#define SNAKE_REPLAY_U8_NHWC  0   /* states as uint8 [B][h][w][C]: the bytes that were pushed */
#define SNAKE_REPLAY_F32_NCHW 1   /* states as float [B][C][h][w], 0.0 / 1.0: x.permute(0,3,1,2).float() (:122) */

/* Validates cfg (host only, no device needed; SNAKE_E_CONFIG names the field)
 * and returns the buffer sizes for pushes of num_envs envs (0 .. 2^26). */
int snake_replay_plan(const snake_replay_cfg *cfg, int64_t num_envs, snake_replay_layout *out);

/* obs, next_obs: uint8 [N][S][h][w][C], 8-byte aligned; actions: int8 [N][S];
 * rewards: double [N][S]; done: uint8 [N][S]; skip: uint8 [N][S] or NULL (every
 * snake stored); step: int32 [N] or NULL (no penalty). Three launches on
 * `stream` (k_replay_count, k_replay_scan, k_replay_store) whose grids depend
 * on num_envs only; no host sync, the slots are assigned by a prefix count and
 * do not vary from run to run. */
int snake_replay_push(const snake_replay_cfg *cfg, const snake_replay_rings *rings, const uint8_t *obs,
                      const uint8_t *next_obs, const int8_t *actions, const double *rewards,
                      const uint8_t *done, const uint8_t *skip, const int32_t *step, int64_t num_envs,
                      void *scratch, void *stream);

/* idx: int64 [B]; state, next_state: 16-byte aligned, uint8 [B][h][w][C] or
 * float [B][C][h][w] by `format`; action: int64 [B]; reward, done: float [B]
 * (the dtypes of update_model's five tensors, :236-240). One launch
 * (k_replay_gather_u8 / k_replay_gather_f32) on `stream`. B * h*w*obs_c/8 must
 * be below 2^30. */
int snake_replay_gather(const snake_replay_cfg *cfg, const snake_replay_rings *rings, const int64_t *idx,
                        int64_t batch, int32_t format, void *state, void *next_state, int64_t *action,
                        float *reward, float *done, void *stream);

/* ---- Python's `random` on the device: the one generator the reference
 * trainer draws from -- random.random() < epsilon and random.randrange(A) per
 * live snake (train_dqn.py:163-165), random.sample(buffer, B) per update
 * (:96-97) -- so that a run seeded like random.seed(s) makes the reference's
 * choices, draws its minibatch indices and leaves its generator state.
 * (pyrandom_kernels.hip.)
 *
 * A stream is the 624 key words (uint32) and the position (int32, 0..624) of
 * random.Random.getstate()[1]. The caller owns n streams in two device arrays,
 * key [n][624] and pos [n]. With u32() the next tempered MT19937 word (a
 * position of 624 twists the key first), CPython defines
 *   getrandbits(k), 1 <= k <= 32   u32() >> (32 - k): the top bits;
 *   _randbelow(n), 1 <= n < 2^31   k = n.bit_length(); getrandbits(k) until the
 *                                  result is below n (a power of two n rejects
 *                                  half of its words);
 *   random()                       a = u32() >> 5, b = u32() >> 6, then
 *                                  (a * 67108864 + b) / 2^53, exact in a double.
 * Every rejection loop is bounded: after 256 words without a result -- a word
 * rejects with probability below 9/16, no real stream gets there -- the call
 * sets *err (device int32, zero it once; sticky: nothing ever clears it) and
 * finishes with values inside the range. A position outside [0, 624] sets *err
 * and is read as 624.
 *
 * Act. Env e uses stream e; its snakes are taken in slot order. A snake whose
 * skip byte is nonzero gets action 0 and consumes nothing (:281-285). Every
 * other snake draws u = random() -- both words, whatever epsilon is: the
 * reference evaluates random.random() < epsilon whenever it trains -- and if
 * u < epsilon (as doubles) its action is _randbelow(A), otherwise the first
 * maximal index of its row of q (NaN Q-values are outside the contract). A step
 * that crosses no key boundary reads the few words it consumes and writes the
 * position only; a stream whose position reaches 624 with a word to draw has
 * its key twisted in place.
 *
 * Sample. random.sample(range(n), B) from one stream, n = min(*count, capacity)
 * read on the device (count: a replay buffer's counter):
 *   setsize = 21, and for B > 5 also 4 ** ceil(log(3 B, 4)) (in integers: the
 *   smallest power of four >= 3 B; 4117 at B = 512, 16405 at B = 4096);
 *   n <= setsize: pool = [0, n); for i in 0..B-1: j = _randbelow(n - i),
 *                 idx[i] = pool[j], pool[j] = pool[n - i - 1];
 *   otherwise:    for i in 0..B-1: j = _randbelow(n) until j is not yet
 *                 selected, idx[i] = j.
 * The indices are logical (0 the oldest transition held), as snake_replay_gather
 * takes them. Work and memory are O(B): nothing depends on the capacity.
 * n < B is where Python raises: the call sets *err, draws nothing and writes
 * indices inside [0, max(n, 1)). */

/* Host only. SNAKE_E_CONFIG names the field: num_actions 1..127, batch 1..4096,
 * capacity 1..2^31-1. Returns random.sample's setsize for `batch` (>= 21). */
int snake_pyrandom_plan(int32_t num_actions, int64_t batch, int64_t capacity);

/* q: float [N * S][A]; skip: uint8 [N][S] or NULL; key, pos: the first N
 * streams; actions: int8 [N][S]. num_envs 0..2^26, num_snakes 1..16. One launch
 * (k_pyrandom_act) on `stream`. */
int snake_pyrandom_act(const float *q, const uint8_t *skip, double epsilon, uint32_t *key, int32_t *pos,
                       int8_t *actions, int32_t *err, int64_t num_envs, int32_t num_snakes, int32_t num_actions,
                       void *stream);

/* key, pos: the stream arrays, of which stream `stream_index` is used; count:
 * device int64; idx: int64 [batch]. One launch (k_pyrandom_sample, one wave) on
 * `stream`. */
int snake_pyrandom_sample(uint32_t *key, int32_t *pos, int64_t stream_index, const int64_t *count,
                          int64_t capacity, int64_t batch, int64_t *idx, int32_t *err, void *stream);

/* ---- Genome heads: a population of NEAT feed-forward networks, one genome
 * per env (train_ga.py:224-257 eval_genomes: every live snake's 128 features of
 * the frozen DQN go through the genome's neat.nn.FeedForwardNetwork, the action
 * is np.argmax of its outputs; train_dqn.py:725-772 HybridNEATEnemy is the same
 * head).
 *
 * A population is packed once into one flat program. Genome g owns the nodes
 * [node_off[g], node_off[g + 1]) in evaluation order (FeedForwardNetwork's
 * node_evals); node n owns the links [link_off[n], link_off[n + 1]) in order.
 * Values live in slots: slots 0 .. I-1 are the inputs, slot I + k is the
 * genome's k-th node, so a link's source slot is below its node's slot. Per
 * feature row the result is, in IEEE double with no fused multiply-add,
 *     s = +0.0;  for each link in order: s = s + value[src] * weight
 *     value[I + k] = act(bias + response * s)
 * with the inputs the float features widened to double (numpy 1.21, which the
 * reference pins: float32 scalar * Python float is float64), and act one of
 *     relu     z > 0.0 ? z : 0.0
 *     sigmoid  z = max(-60, min(60, 5 z));   1 / (1 + exp(-z))
 *     tanh     z = max(-60, min(60, 2.5 z)); tanh(z)
 * (neat-python's relu_, sigmoid_ and tanh_activation; the aggregation is sum).
 * Output a is the value of slot out_slot[g][a], or 0.0 where that is -1 (an
 * output key no node evaluates keeps activate()'s initial 0.0). The action is
 * the first maximum of the outputs; a row whose skip byte is nonzero gets
 * action 0 (train_ga.py:236; its outputs are still computed). relu-only
 * programs are exact; exp and tanh are the device library's. NaN or infinite
 * weights and features are outside the contract. */
#define SNAKE_GENOME_RELU    0
#define SNAKE_GENOME_SIGMOID 1
#define SNAKE_GENOME_TANH    2

typedef struct {
    int32_t num_inputs;     /* I, 1..1024 */
    int32_t num_outputs;    /* A, 1..16 */
    int32_t num_genomes;    /* G, 1..2^20 */
    int32_t max_nodes;      /* nodes of the largest genome */
    int64_t num_nodes;      /* nodes of all genomes, 0..2^30 */
    int64_t num_links;      /* links of all nodes, 0..2^30 */
} snake_genome_cfg;

typedef struct {        /* the packed program: host arrays for snake_genome_check, device arrays for the launch */
    const int32_t *node_off;    /* [G + 1], from 0 to num_nodes */
    const int32_t *node_act;    /* [num_nodes] SNAKE_GENOME_RELU / _SIGMOID / _TANH */
    const double *node_bias;    /* [num_nodes] */
    const double *node_resp;    /* [num_nodes] response */
    const int32_t *link_off;    /* [num_nodes + 1], from 0 to num_links */
    const int32_t *link_src;    /* [num_links] source slot */
    const double *link_w;       /* [num_links] */
    const int32_t *out_slot;    /* [G][A] slot of output a, -1: never evaluated */
} snake_genome_prog;

typedef struct {        /* up to tile_rows feature rows of one genome: the work of one wave */
    int32_t genome;
    int32_t count;          /* rows, 1..tile_rows */
    int32_t row_start;      /* the rows are rows[row_start .. row_start + count) */
    int32_t scratch;        /* index of the tile's slice of the scratch buffer, -1: node values in LDS */
} snake_genome_tile;

typedef struct {
    int64_t scratch;        /* bytes of snake_genome_actions' scratch (0: every genome's node values fit LDS) */
    int64_t max_tiles;      /* the most tiles snake_genome_tiles makes of that many rows */
    int32_t tile_rows;      /* rows per tile: 64, fewer where 64 rows of I features do not fit LDS */
    int32_t lds_nodes;      /* genomes of more nodes keep their node values in the scratch buffer */
    int32_t lds_bytes;      /* dynamic LDS of the launch */
} snake_genome_layout;

/* Validates cfg (host only, no device needed; SNAKE_E_CONFIG names the field)
 * and returns the sizes for launches over `rows` feature rows (0 .. 2^30). */
int snake_genome_plan(const snake_genome_cfg *cfg, int64_t rows, snake_genome_layout *out);

/* Checks a packed program in HOST memory against cfg (host only): SNAKE_E_CONFIG
 * names the field when node_off or link_off is not monotone from 0 to its total,
 * a node_act is not an activation id, a link_src is not below its node's slot,
 * an out_slot is outside [-1, I + the genome's nodes), or max_nodes is not the
 * largest genome's node count. The kernel trusts these indices: upload a
 * program only after this call has returned SNAKE_OK. */
int snake_genome_check(const snake_genome_cfg *cfg, const snake_genome_prog *host_prog);

/* Groups the N * S feature rows (row = env * S + snake) by genome (host only).
 * node_off: the program's, host; genome_of_env: int32 [N], any order, repeats
 * allowed; rows: int32 [N * S] out, the rows ordered by genome (envs of one
 * genome in index order); tiles: out, at most tile_cap of them, or NULL to count.
 * Returns the number of tiles (at most snake_genome_layout.max_tiles) or a
 * negative error. Upload both arrays as they are for snake_genome_actions. */
int64_t snake_genome_tiles(const snake_genome_cfg *cfg, const int32_t *node_off,
                           const int32_t *genome_of_env, int64_t num_envs, int32_t num_snakes,
                           int32_t *rows, snake_genome_tile *tiles, int64_t tile_cap);

/* prog: device arrays that passed snake_genome_check; tiles, rows: device copies
 * of snake_genome_tiles' output for the same cfg; features: float [num_rows][I];
 * skip: uint8 [num_rows] or NULL; actions: int8 [num_rows] out; outputs: double
 * [num_rows][A] out or NULL; scratch: snake_genome_layout.scratch bytes for
 * num_rows rows (may be NULL when that is 0; contents need not survive a call).
 * One launch (k_genome_actions) on `stream`, on the stream's device. */
int snake_genome_actions(const snake_genome_cfg *cfg, const snake_genome_prog *prog,
                         const snake_genome_tile *tiles, const int32_t *rows, int64_t num_tiles,
                         const float *features, const uint8_t *skip, int8_t *actions, double *outputs,
                         void *scratch, int64_t num_rows, void *stream);

/* Last error message of this thread ("" if none). */
const char *snake_last_error(void);

int snake_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SNAKE_ENV_H */
