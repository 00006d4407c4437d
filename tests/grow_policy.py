"""A deterministic host policy that grows snakes, the cases the long-snake tests
run with it, and the coverage those cases reach on the CPU oracle.

Random actions kill a snake within tens of steps at about 7 cells; the body
ring of k_logic / k_step (step_logic.h: whole tail queue up to 14 directions,
refills from 8-byte chunks, pending head bits, ring wrap, the 16-at-a-time death
erase, the dirty-chunk commit) only shows a wrong byte once a tail reaches it or
the snake dies long. This policy walks every snake towards the nearest fruit and
away from dead ends, so snakes pass 16, 34 and more cells before they die.

The rule (pure numpy on an oracle env's `grid` and `snakes()` table, rows
hr, hc, tr, tc, dir, alive, len; no randomness):
  dead snakes get action 0; alive snakes are processed in slot order;
  actions are tried in the order 0 keep, 1 left (dir + 3) & 3, 2 right
  (dir + 1) & 3; an action is a candidate if its target cell is EMPTY or FRUIT
  and no earlier slot claimed that cell this step; the candidate with the
  smallest key (target has no EMPTY / FRUIT 4-neighbour, Manhattan distance from
  the target to the nearest fruit -- 0 on a fruit cell and with no fruit at all
  --, action) is taken and claims its target; without a candidate: action 0.
"""
import numpy as np

EMPTY, WALL, FRUIT = 0, 1, 2
_DR = (-1, 0, 1, 0)   # 0 UP, 1 RIGHT, 2 DOWN, 3 LEFT
_DC = (0, 1, 0, -1)


def actions(grid, snakes):
    """(S,) actions in {0, 1, 2} for one env."""
    grid = np.asarray(grid)
    open_ = ((grid == EMPTY) | (grid == FRUIT)).tolist()
    fruits = np.argwhere(grid == FRUIT)
    fr, fc = fruits[:, 0], fruits[:, 1]
    claimed = set()
    out = np.zeros(len(snakes), np.int64)
    for k, (hr, hc, _, _, d, alive, _) in enumerate(np.asarray(snakes).tolist()):
        if not alive:
            continue
        best = None
        for a, nd in enumerate((d, (d + 3) & 3, (d + 1) & 3)):
            r, c = hr + _DR[nd], hc + _DC[nd]
            if not open_[r][c] or (r, c) in claimed:
                continue
            # (an open cell is interior: its four neighbours are on the board)
            dead_end = not (open_[r - 1][c] or open_[r + 1][c] or open_[r][c - 1] or open_[r][c + 1])
            dist = int((np.abs(fr - r) + np.abs(fc - c)).min()) if len(fr) else 0
            key = (dead_end, dist, a)
            if best is None or key < best[0]:
                best = (key, a, (r, c))
        if best is not None:
            out[k] = best[1]
            claimed.add(best[2])
    return out


def batch_actions(envs):
    """(len(envs), S) policy actions from the oracle envs' current states."""
    return np.stack([actions(e.grid, e.snakes()) for e in envs])


def ring_cap(kw):
    """The body ring's size in bytes (snake_plan): the interior cells rounded up
    to a power of two, at least 16."""
    n = (kw['height'] - 2) * (kw['width'] - 2)
    return max(16, 1 << (n - 1).bit_length())


def logic_lanes(S, N):
    """Lanes per env of k_logic (snake_capi.cpp plan_logic): 4 / 8 / 16 for
    S <= 4 / 8 / 16 (lanes_per_env), at least 8 up to 8192 envs."""
    lanes = 4 if S <= 4 else (8 if S <= 8 else 16)
    return max(lanes, 8) if N <= 8192 else lanes


SEED = 7   # env i of every case is seeded SEED + i

_A = dict(height=12, width=12, snake_length=3, num_fruits=10, vision_range=3)

# name -> (board kwargs, num_snakes, num_envs, steps); what each is for:
CASES = {
    # 8 lanes per env, background spawn kernel, one frame of 9 chunks committed
    # in place chunk by chunk, ring of 128 bytes
    'grow_12_s4': (_A, 4, 32, 400),
    # the same board through the fused step: the !ep_end store guards
    'fused_grow_12_s4': (dict(_A, spawn_background=-1), 4, 32, 400),
    # 4 lanes per env, 16 envs per wave; the policy drives sampled_envs() only
    'grow_12_s4_16384': (_A, 4, 16384, 300),
    # two frames: the whole-frame commit into the next ring slot
    'grow_16_s8_fs2': (dict(height=16, width=16, snake_length=3, num_fruits=24, vision_range=3, frame_stack=2),
                       8, 16, 400),
    # 16 lanes per env
    'grow_24_s16': (dict(height=24, width=24, snake_length=2, num_fruits=40, vision_range=3), 16, 16, 300),
    # a board that fills up: respawns with one, no or too few empty cells; ring of 64
    'grow_8_s2_full': (dict(height=8, width=8, snake_length=2, num_fruits=6), 2, 32, 400),
    # the 16-byte minimum ring: both death chunks are the same chunk, a wrap
    # every 16 steps, at most 15 directions
    'grow_6_s1_cap16': (dict(height=6, width=6, snake_length=2, num_fruits=2), 1, 32, 300),
    # one frame of 81 chunks: no in-place commit
    'grow_36_s4': (dict(height=36, width=36, snake_length=3, num_fruits=64, vision_range=4), 4, 16, 300),
    # W != H in the row / column arithmetic of the death walk
    'grow_rect_10x20_s3': (dict(height=10, width=20, snake_length=3, num_fruits=14, vision_range=3), 3, 32, 400),
}

_LONG = ('deaths_le17', 'deaths_18_33', 'deaths_ge34', 'grow16_off_group0', 'long_moves', 'multi_eat')
_FULL = ('full_fewer_fruits', 'full_same_fruits_grew')
# name -> the coverage counts that must be at least 1
REQUIRED = {
    'grow_12_s4': _LONG + ('eps_gt_cap',),
    'fused_grow_12_s4': _LONG + ('eps_gt_cap',),
    'grow_12_s4_16384': ('deaths_ge34', 'grow16_off_group0'),
    'grow_16_s8_fs2': _LONG,
    'grow_24_s16': _LONG,
    'grow_8_s2_full': _LONG + ('eps_gt_cap',) + _FULL,
    # (its ring holds at most 15 directions: no death past 16 cells)
    'grow_6_s1_cap16': ('eps_gt_cap',) + _FULL + ('deaths_ge12', 'grow16'),
    'grow_36_s4': _LONG,
    'grow_rect_10x20_s3': _LONG,
}


def sampled_envs(N):
    """The envs of a full-size batch that get oracle twins and policy actions."""
    return np.unique(np.concatenate([np.arange(8), np.linspace(0, N - 1, 40).astype(int),
                                     np.random.RandomState(0).randint(0, N, 16)]))


def oracle_kwargs(kw):
    """The board without the GPU scheduling knobs."""
    return {k: x for k, x in kw.items() if k not in ('spawn_ahead', 'spawn_background')}


def coverage(oracle, name):
    """Step the case's oracle envs under the policy, with the vector env's
    all-done reset, and count from the oracle alone what the rollout reaches."""
    kw, S, N, T = CASES[name]
    idx = sampled_envs(N) if N > 4096 else np.arange(N)
    envs = [oracle.OracleEnv(seed=SEED + int(i), num_snakes=S, **oracle_kwargs(kw)) for i in idx]
    for e in envs:
        e.reset()
    cap, per_wave = ring_cap(kw), 64 // logic_lanes(S, N)
    n = dict.fromkeys(_LONG + _FULL + ('eps_gt_cap', 'deaths_ge12', 'grow16', 'max_len'), 0)
    for _ in range(T):
        for i, e in zip(idx, envs):
            g0, t0 = e.grid, e.snakes()
            _, _, done, _ = e.step(actions(g0, t0))
            g1, t1 = e.grid, e.snakes()
            was, now = t0[:, 5] == 1, t1[:, 5] == 1
            l0, l1 = t0[:, 6], t1[:, 6]
            died = l0[was & ~now]
            n['deaths_le17'] += int((died <= 17).sum())
            n['deaths_18_33'] += int(((died >= 18) & (died <= 33)).sum())
            n['deaths_ge34'] += int((died >= 34).sum())
            n['deaths_ge12'] += int((died >= 12).sum())
            grew = was & now & (l1 == l0 + 1)
            g16 = int((grew & (l0 == 15)).sum())
            n['grow16'] += g16
            n['grow16_off_group0'] += g16 if int(i) % per_wave else 0
            n['long_moves'] += int((was & now & (l1 == l0) & (l0 >= 16)).sum())
            n['multi_eat'] += int(grew.sum() >= 2)
            n['max_len'] = max(n['max_len'], int(l1[now].max()) if now.any() else 0)
            if not (g1 == EMPTY).any():
                f0, f1 = int((g0 == FRUIT).sum()), int((g1 == FRUIT).sum())
                n['full_fewer_fruits'] += int(f1 < f0)
                n['full_same_fruits_grew'] += int(f1 == f0 and grew.any())
            if done.all():
                n['eps_gt_cap'] += int(e.episode_length > cap)
                e.reset()
    return n


# ------------------------------------------------- death at every ring phase
# One env per (L, t): a snake of L cells injected as a boustrophedon, its head
# at the start of an empty corridor along the top wall; it moves t steps
# straight and then turns left into the wall ('wall'), or turns right three
# times into its own body ('self'). An injected snake starts with ring head 0
# and a tail queue of one entry, so the head position mod 16, the pending
# head-bit count (t mod 4), head-word completion and one to five rounds of the
# death walk (L - 1 = 1 .. 64 directions) all vary over the batch, every tail
# move on the refill path.
RING_LENGTHS = (2, 3, 4, 5, 15, 16, 17, 18, 31, 32, 33, 34, 47, 48, 49, 50, 65)
RING_STRAIGHT = range(20)
RING_BOARD = dict(height=12, width=30, num_fruits=2,
                  reward_dict={'fruit': 10.0, 'kill': 3.0, 'lose': -0.5, 'win': 7.0, 'time': -0.001})


def ring_cases(kind):
    """[(L, t)] of the batch: every length for 'wall', L >= 16 for 'self'."""
    return [(L, t) for L in RING_LENGTHS if kind == 'wall' or L >= 16 for t in RING_STRAIGHT]


def ring_path(L, H, W):
    """L cells head first: head (1, 3) heading RIGHT, neck (1, 2), then (1, 1),
    (2, 1) and rows 3 .. H - 2 back and forth over the whole width. Row 1 right
    of the head and row 2 right of column 1 stay empty."""
    path = [(1, 3), (1, 2), (1, 1), (2, 1)]
    for r in range(3, H - 1):
        cols = range(1, W - 1) if r % 2 else range(W - 2, 0, -1)
        path += [(r, c) for c in cols]
    assert L <= len(path)
    return path[:L]


def ring_state(L, slot, S, H, W):
    """(grid, snakes, alive_snakes) for inject: the long snake in `slot`, dead
    snakes (on no cell of the grid) in the other slots, no fruit."""
    grid = np.zeros((H, W), np.int64)
    grid[0, :] = grid[-1, :] = grid[:, 0] = grid[:, -1] = WALL
    path = ring_path(L, H, W)
    for r, c in path[1:-1]:
        grid[r, c] = 4 + 10 * slot
    grid[path[-1]] = 5 + 10 * slot
    grid[path[0]] = 3 + 10 * slot
    snakes = [(path, True) if k == slot else ([(2, 2), (2, 3)], False) for k in range(S)]
    return grid, snakes, 1


def ring_action(kind, t, step):
    """The long snake's action at `step` (0-based): straight for t steps, then
    one left turn into the wall, or three right turns into the own body."""
    if kind == 'wall':
        return 1 if step == t else 0
    return 2 if t <= step < t + 3 else 0


def ring_death_step(kind, t):
    return t if kind == 'wall' else t + 2


# --------------------------------------------- a nearly full 16-byte ring
# One env per (L, start): a snake of 12 to 15 cells on the 16 interior cells of
# a 6x6 board walks round a closed tour, never eating, for three turns of its
# 16-byte ring. The policy never gets there (a snake that long on this board
# eats or dies): the tail refills come from chunks that also hold the head
# word, wrapped behind the head.
CYCLE_BOARD = dict(RING_BOARD, height=6, width=6)
CYCLE_LENGTHS = (12, 13, 14, 15)
CYCLE_STEPS = 48
_CYCLE = [(1, 1), (1, 2), (1, 3), (1, 4), (2, 4), (3, 4), (4, 4), (4, 3), (3, 3), (2, 3), (2, 2), (3, 2), (4, 2),
          (4, 1), (3, 1), (2, 1)]


def cycle_cases():
    return [(L, s) for L in CYCLE_LENGTHS for s in range(16)]


def cycle_state(L, start):
    """(grid, snakes, alive_snakes): head on tour cell `start`, body behind it."""
    path = [_CYCLE[(start - j) % 16] for j in range(L)]
    grid = np.zeros((6, 6), np.int64)
    grid[0, :] = grid[-1, :] = grid[:, 0] = grid[:, -1] = WALL
    for r, c in path[1:-1]:
        grid[r, c] = 4
    grid[path[-1]], grid[path[0]] = 5, 3
    return grid, [(path, True)], 1


def cycle_action(start, step):
    """The action that takes the head from tour cell start + step to the next."""
    a, b, c = (_CYCLE[(start + step + j) % 16] for j in (-1, 0, 1))
    dmap = {(-1, 0): 0, (0, 1): 1, (1, 0): 2, (0, -1): 3}
    d, nd = dmap[(b[0] - a[0], b[1] - a[1])], dmap[(c[0] - b[0], c[1] - b[1])]
    return {0: 0, 3: 1, 1: 2}[(nd - d) & 3]
