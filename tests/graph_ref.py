"""The graph observation's rule (include/snake_env.h, snake_graph_obs) restated
in numpy: what the reference's GraphSnakeEnv._process_obs computes, with both
ways of choosing the observation a snake reads. Shared by test_graph_cpu.py,
test_graph_gpu.py and the fixture generator (tests/golden/gen/make_graph_golden.py),
which checks it against the reference call by call."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'graph_calls.npz')

DIRS = ((-1, 0), (0, 1), (1, 0), (0, -1))      # 0 UP, 1 RIGHT, 2 DOWN, 3 LEFT
FULL_MAP_STEPS = 5
# how a ray ended (graph_obs's third result)
NOT_CAST, WALL, FULL, CLIPPED = 0, 1, 2, 3
CONFIGS = ('b8', 'r9x12fs2', 'r8x10vr2fs2', 'b20vr5', 'b20vr5fs2', 'r7x11s1')


def ray_steps(d):
    """The five rays' steps for direction code d: forward, left, right, forward-left, forward-right."""
    dr, dc = DIRS[d]
    F, L, R = (dr, dc), (-dc, dr), (dc, -dr)
    return (F, L, R, (F[0] + L[0], F[1] + L[1]), (F[0] + R[0], F[1] + R[1]))


def weights(n, float32_quotient):
    """(2, n) float64: row 0 the axis rays' 1/(i+1), row 1 the diagonal rays'
    1/((i+1)*sqrt(2)). float32_quotient (the full-map observation, float32 in
    the reference): the quotient taken in float32, then widened."""
    i = np.arange(1, n + 1, dtype=np.float64)
    diag = i * math.sqrt(2.0)
    if float32_quotient:
        one = np.float32(1.0)
        return np.stack([(one / i.astype(np.float32)).astype(np.float64),
                         (one / diag.astype(np.float32)).astype(np.float64)])
    return np.stack([1.0 / i, 1.0 / diag])


def graph_obs(obs, heads, dirs, alive, vision_range, source='own'):
    """obs uint8 (N, S, h, w, C); heads (N, S, 2) row, column; dirs (N, S) codes;
    alive (N, S). Returns (float64 (N, S, 5, C) with zero rows for dead snakes,
    int8 (N, S, 5) how each ray ended)."""
    assert source in ('own', 'reference')
    obs = np.asarray(obs)
    N, S, h, w, C = obs.shape
    vr = int(vision_range or 0)
    n = vr if vr else FULL_MAP_STEPS
    wt = weights(n, vr == 0)
    alive = np.asarray(alive).reshape(N, S) != 0
    dirs = np.asarray(dirs).reshape(N, S).astype(np.int64) & 3
    heads = np.asarray(heads).reshape(N, S, 2).astype(np.int64)
    env = np.arange(N)[:, None]
    # the observation a snake reads: its own, or the one the reference's counter of live snakes points at
    slot = np.broadcast_to(np.arange(S), (N, S))
    if source == 'reference':
        slot = np.where(alive, np.cumsum(alive, axis=1) - 1, 0)
    r0 = np.full((N, S), vr) if vr else heads[..., 0]
    c0 = np.full((N, S), vr) if vr else heads[..., 1]
    steps = np.array([ray_steps(d) for d in range(4)])[dirs]      # (N, S, 5, 2)
    out = np.zeros((N, S, 5, C), np.float64)
    ended = np.zeros((N, S, 5), np.int8)
    for ray in range(5):
        going = alive.copy()
        acc = np.zeros((N, S, C), np.float64)
        for i in range(n):      # in ascending order: the sums are taken in the reference's order
            r, c = r0 + (i + 1) * steps[:, :, ray, 0], c0 + (i + 1) * steps[:, :, ray, 1]
            inside = (r >= 0) & (r < h) & (c >= 0) & (c < w)
            ended[:, :, ray][going & ~inside] = CLIPPED
            going &= inside
            cell = obs[env, slot, np.clip(r, 0, h - 1), np.clip(c, 0, w - 1)]        # (N, S, C)
            acc = acc + np.where(going[..., None] & (cell == 1), wt[int(ray >= 3), i], 0.0)
            wall = going & (cell[..., 0] == 1)
            ended[:, :, ray][wall] = WALL
            going &= ~wall
        ended[:, :, ray][going] = FULL
        out[:, :, ray] = acc
    return out, ended


def compact(rows, alive):
    """One env's (S, 5, C) rows -> what GraphSnakeEnv returns before its uint8
    cast: the live snakes' rows in index order, shape (0,) when there is none."""
    rows = np.asarray(rows)[np.asarray(alive).astype(bool)]
    return rows if len(rows) else np.zeros((0,), np.float64)


def load_calls():
    """{config: dict} of the recorded _process_obs calls: shape (S, h, w, C), vr,
    obs uint8 (R, S, h, w, C), heads (R, S, 2), dirs (R, S), alive (R, S), rows
    float64 (R, S, 5, C) (live rows first, zero padded), n_alive (R,), ret uint8
    (R, S, 5, C) (the env's return, padded alike)."""
    z = np.load(GOLDEN, allow_pickle=False)
    out = {}
    for name in CONFIGS:
        S, h, w, C, vr = (int(x) for x in z[name + '_shape'])
        R = len(z[name + '_n_alive'])
        obs = np.unpackbits(z[name + '_obs'], axis=1)[:, :S * h * w * C].reshape(R, S, h, w, C)
        out[name] = dict(S=S, h=h, w=w, C=C, vr=vr, obs=np.ascontiguousarray(obs),
                         **{k: z[name + '_' + k] for k in ('heads', 'dirs', 'alive', 'rows', 'n_alive', 'ret')})
    return out


def load_trajectories():
    """{config: dict(kwargs, seed, actions (T, S), shapes (T + resets, 3), obs
    list of uint8 arrays)}: one short reference GraphSnakeEnv rollout per
    configuration. Entry j of `events` is -1 for a reset() or the index of the
    step's action row; `obs[j]` is what that call returned."""
    z = np.load(GOLDEN, allow_pickle=False)
    out = {}
    for name in CONFIGS:
        kw = dict(zip(('height', 'width', 'num_snakes', 'snake_length', 'vision_range', 'frame_stack'),
                      (int(x) for x in z[name + '_tkw'])))
        kw['vision_range'] = kw['vision_range'] or None
        events, counts, flat = z[name + '_tevents'], z[name + '_tcount'], z[name + '_tobs']
        C = 8 * kw['frame_stack']
        obs, at = [], 0
        for cnt in counts:
            m = int(cnt) * 5 * C
            obs.append(flat[at:at + m].reshape(int(cnt), 5, C) if cnt else np.zeros((0,), np.uint8))
            at += m
        out[name] = dict(kwargs=kw, seed=int(z[name + '_tseed']), actions=z[name + '_tact'], events=events, obs=obs)
    return out
