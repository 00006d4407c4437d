"""The safe-action kernel (snake_safe_actions, policy_kernels.hip) against the
numpy restatement (tests/policy_ref.py) on the same inputs copied to the host:
every case bit-exact (actions and directions are integers)."""
import numpy as np
import pytest

import policy_ref as R

pytestmark = pytest.mark.gpu

UNIT = ((-1, 0), (1, 0), (0, -1), (0, 1))


@pytest.fixture(scope='module')
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), 'needs the GPU'
    return torch


def run_kernel(torch, obs, q, skip, dirs, limit=60):
    """One SafeActions call on host arrays; returns (actions, dirs out) on the host."""
    from marlenv import SafeActions
    sa = SafeActions(obs.shape[1:], fill_limit=limit)
    d = torch.from_numpy(np.ascontiguousarray(dirs)).cuda()
    a = sa(torch.from_numpy(obs).cuda(), torch.from_numpy(q).cuda(),
           skip=None if skip is None else torch.from_numpy(skip).cuda(), dirs=d)
    assert a.dtype == torch.int8 and tuple(a.shape) == obs.shape[:2]
    return a.cpu().numpy(), d.cpu().numpy()


def check(torch, obs, q, skip, dirs, limit=60):
    act, dout, rule = R.safe_actions(obs, q, skip, dirs, limit)
    got_a, got_d = run_kernel(torch, obs, q, skip, dirs, limit)
    np.testing.assert_array_equal(got_a, act)
    np.testing.assert_array_equal(got_d, dout)
    return act, rule


@pytest.mark.parametrize('name', ['b10x14', 'b12', 'full20', 'vr5'])
def test_fixture_records(torch_gpu, name):
    """The reference's own calls, one record per env of a batch."""
    c = R.load_calls()[name]
    got_a, got_d = run_kernel(torch_gpu, c['obs'], c['q'], c['skip'], c['din'])
    np.testing.assert_array_equal(got_a, c['act'])
    np.testing.assert_array_equal(got_d, c['dout'])


def synthetic(rs, N, S, h, w):
    """Random observations with bytes from {0, 1, 2, 255} (only == 1 counts):
    per snake a blocked density from open to nearly closed maps, a body of 0 to
    ~40 cells, 0 to 3 heads (most snakes one; a third of them on the map's
    edge, where nothing says there is a wall) and 0 to 2 tails."""
    obs = np.zeros((N, S, h, w, 8), np.uint8)
    vals = np.array([1, 1, 1, 2, 255], np.uint8)

    def sprinkle(plane, p):
        m = rs.random_sample(plane.shape) < p
        plane[m] = vals[rs.randint(len(vals), size=int(m.sum()))]

    for n in range(N):
        for s in range(S):
            o = obs[n, s]
            block = rs.uniform(0.02, 0.6)
            sprinkle(o[:, :, 0], block * 0.7)
            sprinkle(o[:, :, 3], block * 0.3)
            sprinkle(o[:, :, 1], 0.08)
            sprinkle(o[:, :, 2], 0.02)
            sprinkle(o[:, :, 4], 0.01)
            sprinkle(o[:, :, 6], rs.randint(0, 41) / (h * w))
            sprinkle(o[:, :, 5], 0.01 * (rs.randint(3) == 0))          # decoys and extra heads
            for _ in range(rs.choice([0, 1, 1, 1, 1, 2, 3])):
                y, x = rs.randint(h), rs.randint(w)
                if rs.randint(3) == 0:
                    y, x = [(0, x), (h - 1, x), (y, 0), (y, w - 1)][rs.randint(4)]
                o[y, x, :] = 0
                o[y, x, 5] = 1
            for _ in range(rs.choice([0, 1, 1, 2])):
                o[rs.randint(h), rs.randint(w), 7] = vals[rs.randint(len(vals))]
    q = (rs.randint(-1, 2, size=(N, S, 3)) / 2).astype(np.float32)     # ties in most rows
    plain = rs.random_sample((N, S)) < 0.3
    q[plain] = rs.randn(int(plain.sum()), 3).astype(np.float32)
    skip = (rs.random_sample((N, S)) < 0.2).astype(np.uint8)
    choices = np.array(UNIT + ((0, 0), (R.UNKNOWN, R.UNKNOWN), (R.UNKNOWN, R.UNKNOWN)), np.int8)
    dirs = choices[rs.randint(len(choices), size=(N, S))]
    return obs, q, skip, dirs


@pytest.mark.parametrize('S,h,w', [(4, 20, 20), (4, 11, 11), (8, 40, 40), (3, 7, 13), (1, 3, 3), (16, 64, 64)])
def test_synthetic(torch_gpu, S, h, w):
    """37 envs (odd: with odd h*w the batch ends on a half 16-byte chunk);
    (16, 64, 64) puts rows on lanes 0 and 63 and columns on bits 0 and 63."""
    rs = np.random.RandomState(1000 * S + 10 * h + w)
    obs, q, skip, dirs = synthetic(rs, 37, S, h, w)
    act, rule = check(torch_gpu, obs, q, skip, dirs)
    if (S, h, w) == (4, 20, 20):
        # the inputs reach every rule, a snake without a head and all three moves masked
        for r in (R.OUTSIDE, R.OCCUPIED, R.DEADLY_CELL, R.NEAR_HEAD, R.FILL, R.SKIP, R.NOHEAD, R.NONE):
            assert (rule == r).any(), R.RULE_NAMES[r]
    # a small limit binds on open maps too
    check(torch_gpu, obs, q, None, dirs, limit=7)


def test_all_moves_masked_and_ties(torch_gpu):
    """A head walled in on three sides: every move masked gives action 0 whatever
    q says; an open map with equal Q-values gives the first move."""
    obs = np.zeros((2, 1, 5, 5, 8), np.uint8)
    obs[0, 0, :, :, 0] = 1
    obs[0, 0, 2, 2, 0] = 0
    obs[0, 0, 2, 2, 5] = 1
    obs[1, 0, 2, 2, 5] = 1
    q = np.array([[[0.0, 2.0, 1.0]], [[0.5, 0.5, 0.5]]], np.float32)
    dirs = np.array([[[0, 1]], [[1, 0]]], np.int8)
    act, _ = check(torch_gpu, obs, q, None, dirs)
    assert act.tolist() == [[0], [0]]


def corridor_case(L, C, fruit, h=20, w=20):
    """A snake of length L along the boustrophedon path of a map that is wall
    everywhere else, its head facing a free corridor of exactly C cells (the
    path's next C cells; with `fruit` the first of them holds one). The tail
    cell touches only the body, so freeing it adds nothing to the corridor."""
    path = [(r, c if r % 2 == 0 else w - 1 - c) for r in range(h) for c in range(w)]
    o = np.zeros((h, w, 8), np.uint8)
    o[:, :, 0] = 1
    for y, x in path[:L + C]:
        o[y, x, 0] = 0
    o[path[0][0], path[0][1], 7] = 1
    for y, x in path[1:L - 1]:
        o[y, x, 6] = 1
    hy, hx = path[L - 1]
    o[hy, hx, 5] = 1
    if fruit:
        o[path[L][0], path[L][1], 1] = 1
    d = (hy - path[L - 2][0], hx - path[L - 2][1])
    t = (path[L][0] - hy, path[L][1] - hx)
    moves = [d, (-d[1], d[0]), (d[1], -d[0])]
    q = np.zeros(3, np.float32)
    q[moves.index(t)] = 1.0                # the plain argmax walks into the corridor
    return o, q, np.array(d, np.int8)


def test_corridors_around_the_limit(torch_gpu):
    """Corridors of 59, 60 and 61 free cells against snakes of length 59, 60 and
    61 (the last longer than the limit: always masked), with and without a
    fruit on the first corridor cell: the fill masks exactly when
    min(60, C) < L + fruit."""
    cases = [(L, C, f) for L in (59, 60, 61) for C in (59, 60, 61) for f in (0, 1)]
    obs, q, dirs = (np.stack(v) for v in zip(*(corridor_case(*c) for c in cases)))
    obs, q, dirs = obs[:, None], q[:, None], dirs[:, None]
    act, rule = check(torch_gpu, np.ascontiguousarray(obs), q, None, dirs)
    for (L, C, f), r in zip(cases, rule[:, 0]):
        assert (r == R.FILL) == (min(60, C) < L + f), (L, C, f, R.RULE_NAMES[r])


@pytest.mark.parametrize('vision_range', [None, 5])
def test_end_to_end_rollout(torch_gpu, vision_range):
    """80 steps of a 32-env batch driven by the kernel's own actions: at every
    step they equal the restatement run on the GPU's observations, with the
    directions kept by SafeActions and forgotten where an episode ends."""
    torch = torch_gpu
    from marlenv import SafeActions, SnakeVecEnv
    N, S = 32, 4
    env = SnakeVecEnv(N, num_snakes=S, height=20, width=20, snake_length=5, vision_range=vision_range, seed=11)
    sa = SafeActions(env.obs_shape)
    obs = env.reset()
    rs = np.random.RandomState(5)
    dirs = np.full((N, S, 2), R.UNKNOWN, np.int8)
    skip = np.zeros((N, S), np.uint8)
    decided = set()
    for t in range(80):
        q = rs.randn(N, S, 3).astype(np.float32)
        a = sa(obs, torch.from_numpy(q).cuda().view(N * S, 3), skip=torch.from_numpy(skip).cuda())
        act, dirs, rule = R.safe_actions(obs.cpu().numpy(), q, skip, dirs)
        np.testing.assert_array_equal(a.cpu().numpy(), act, err_msg='step %d' % t)
        np.testing.assert_array_equal(sa.dirs.cpu().numpy(), dirs, err_msg='step %d' % t)
        decided |= set(np.unique(rule).tolist())
        obs, _, done, info = env.step(a)
        ended = info['episode_done']
        sa.forget(ended)
        dirs[ended.cpu().numpy()] = R.UNKNOWN
        skip = (done & ~ended[:, None]).cpu().numpy().astype(np.uint8)
    assert {R.NONE, R.DEADLY_CELL} <= decided
    env.close()


def test_evaluate(torch_gpu):
    """evaluate() with a small random fp32 DQN: the episode count is the sum of
    episode_done, the means are finite, and a second run from the same seeds
    returns the same numbers."""
    torch = torch_gpu
    from marlenv import DQNForward, SnakeVecEnv, evaluate
    h = w = 8
    g = torch.Generator().manual_seed(3)
    shapes = {'conv1.weight': (32, 8, 3, 3), 'conv1.bias': (32,), 'conv2.weight': (64, 32, 3, 3),
              'conv2.bias': (64,), 'conv3.weight': (64, 64, 3, 3), 'conv3.bias': (64,),
              'fc1.weight': (256, 64 * h * w), 'fc1.bias': (256,), 'fc2.weight': (128, 256),
              'fc2.bias': (128,), 'fc3.weight': (3, 128), 'fc3.bias': (3,)}
    state = {k: torch.randn(s, generator=g) * 0.05 for k, s in shapes.items()}
    net = DQNForward(state, h, w, 8, num_actions=3, precision='fp32')

    class Counting:                 # the env, counting the episodes its steps end
        def __init__(self, env):
            self.env, self.ended = env, 0

        def __getattr__(self, k):
            return getattr(self.env, k)

        def step(self, a):
            out = self.env.step(a)
            self.ended += int(out[3]['episode_done'].sum())
            return out

    def once():
        env = Counting(SnakeVecEnv(8, num_snakes=2, height=h, width=w, snake_length=3, seed=21,
                                   max_episode_steps=25))
        res = evaluate(env, net, 60)
        env.close()
        return res, env.ended

    (n, score, life), ended = once()
    assert n == ended and n >= 8            # (an episode lasts at most 25 of the 60 steps)
    assert np.isfinite(score) and np.isfinite(life) and 0 < life <= 25
    assert once() == ((n, score, life), ended)
