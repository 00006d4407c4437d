"""The replay buffer's kernels (snake_replay_push / snake_replay_gather,
replay_kernels.hip) and the Collector against the numpy-and-deque restatement
(tests/replay_ref.py) fed with the same inputs on the host. Every comparison is
bit-exact, and the rings are read back through sample(idx=arange(size))."""
import numpy as np
import pytest

import replay_ref as R

pytestmark = pytest.mark.gpu

NAMES = R.NAMES


@pytest.fixture(scope='module')
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), 'needs the GPU'
    return torch


def next_prime(n):
    while any(n % d == 0 for d in range(2, int(n ** 0.5) + 1)):
        n += 1
    return n


random_step, push_both = R.random_step, R.push_both


def assert_rows(got, want):
    names = ('state', 'action', 'reward', 'next_state', 'done')
    for name, g, w_ in zip(names, got, want):
        g = g.cpu().numpy()
        assert g.dtype == w_.dtype and g.shape == w_.shape, (name, g.dtype, g.shape, w_.dtype, w_.shape)
        assert g.tobytes() == w_.tobytes(), name


def assert_same(torch, buf, ref, formats=('uint8', 'float32')):
    """The whole ring, oldest first, in both formats."""
    size = len(ref)
    assert len(buf) == size and int(buf.count.item()) == ref.count
    if size == 0:
        return
    idx = torch.arange(size, device='cuda')
    for fmt in formats:
        assert_rows(buf.sample(idx=idx, format=fmt), ref.rows(format=fmt))


def new_pair(shape, capacity, early_death=(10, -1.0)):
    from marlenv import ReplayBuffer
    return ReplayBuffer(shape, capacity, early_death=early_death), R.RefReplay(capacity, early_death)


def test_fixture_stream(torch_gpu):
    """The reference's own training loop, pushed step by step (N = 1): the final
    rings are the reference's deque."""
    d = R.load_stream()
    S, h, w, c = d['obs'].shape[1:]
    buf, ref = new_pair((S, h, w, c), d['capacity'], d['early_death'])
    R.replay_stream(d, lambda *a: buf.push(*(torch_gpu.from_numpy(np.ascontiguousarray(v)).cuda() for v in a)))
    R.replay_stream(d, ref.push)
    assert_same(torch_gpu, buf, ref)
    want = (d['final_state'], d['final_action'], d['final_reward'], d['final_next_state'],
            d['final_done'].astype(np.float32))
    assert_rows(buf.sample(idx=torch_gpu.arange(d['capacity'], device='cuda')), want)
    fstate = buf.sample(idx=torch_gpu.arange(d['capacity'], device='cuda'), format='float32')[0].cpu().numpy()
    np.testing.assert_array_equal(fstate, d['final_state'].transpose(0, 3, 1, 2).astype(np.float32))


# The issue's five shapes -- the scan block of k_replay_count is 1 024 envs, so
# its 1 500 envs are raised to 3 500: three full blocks and a remainder -- and
# three more for the store kernel's other paths: a 400-byte packed row takes
# two passes of a full wave, a 256-byte row exactly one, a 3-byte row one lane.
SHAPES = [(1, 1, 3, 3, 8), (5, 3, 7, 5, 16), (3, 16, 4, 6, 8), (64, 4, 11, 11, 8), (3500, 4, 3, 3, 8),
          (3, 2, 20, 20, 8), (2, 3, 16, 16, 8), (7, 2, 1, 3, 8)]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_random_pushes(torch_gpu, shape):
    """Six pushes into a ring whose capacity, a prime above twice the snakes of
    a call, is coprime to every per-push count: it wraps at another offset each
    time."""
    N, S, h, w, C = shape
    rs = np.random.RandomState(sum(shape))
    capacity = next_prime(2 * N * S + 1)
    buf, ref = new_pair((S, h, w, C), capacity)
    for i in range(6):
        push_both(torch_gpu, buf, ref, random_step(rs, N, S, h, w, C, p_skip=0.0 if N * S == 1 else 0.3))
        if i in (0, 3):
            assert_same(torch_gpu, buf, ref, formats=('uint8',))
    assert ref.count > capacity                         # it wrapped
    assert_same(torch_gpu, buf, ref)


def test_one_call_stores_more_than_the_capacity(torch_gpu):
    rs = np.random.RandomState(5)
    buf, ref = new_pair((4, 3, 3, 8), 5)
    for _ in range(2):                                  # (from an empty and from a full ring)
        x = random_step(rs, 3, 4, 3, 3, 8)
        x['skip'] = None
        push_both(torch_gpu, buf, ref, x)
        assert len(ref) == 5
        assert_same(torch_gpu, buf, ref)
    action = buf.sample(idx=torch_gpu.arange(5, device='cuda'))[1].cpu().numpy()
    np.testing.assert_array_equal(action, x['actions'].reshape(-1)[7:])      # the last five


def test_every_snake_skipped(torch_gpu):
    rs = np.random.RandomState(6)
    buf, ref = new_pair((3, 4, 5, 8), 11)
    push_both(torch_gpu, buf, ref, random_step(rs, 2, 3, 4, 5, 8))
    x = random_step(rs, 2, 3, 4, 5, 8)
    x['skip'][:] = 1
    push_both(torch_gpu, buf, ref, x)
    assert_same(torch_gpu, buf, ref)
    empty, eref = new_pair((3, 4, 5, 8), 11)
    push_both(torch_gpu, empty, eref, x)
    assert len(empty) == 0 and int(empty.count.item()) == 0


def test_no_skip_and_no_step(torch_gpu):
    """skip=None stores every snake; step=None applies no penalty."""
    rs = np.random.RandomState(7)
    buf, ref = new_pair((3, 4, 5, 8), 50)
    x = random_step(rs, 4, 3, 4, 5, 8)
    x['done'][:] = 1
    x['skip'] = x['step'] = None
    push_both(torch_gpu, buf, ref, x)
    assert len(ref) == 12
    assert_same(torch_gpu, buf, ref)
    reward = buf.sample(idx=torch_gpu.arange(12, device='cuda'))[2].cpu().numpy()
    assert reward.tobytes() == x['rewards'].reshape(-1).astype(np.float32).tobytes()


def test_reward_sum_is_float64_and_the_threshold_is_strict(torch_gpu):
    """r = 1 + 2^-30 with penalty -1.0 stores 2^-30 (a float32 sum stores 0);
    step == early_death_steps gets no penalty, nor does a snake that lives."""
    buf, ref = new_pair((1, 3, 3, 8), 16, early_death=(10, -1.0))
    N = 4
    x = random_step(np.random.RandomState(8), N, 1, 3, 3, 8)
    x['skip'] = None
    x['rewards'][:] = 1.0 + 2.0 ** -30
    x['done'] = np.array([[1], [1], [1], [0]], np.uint8)
    x['step'] = np.array([9, 10, 0, 0], np.int32)
    push_both(torch_gpu, buf, ref, x)
    reward = buf.sample(idx=torch_gpu.arange(N, device='cuda'))[2].cpu().numpy()
    np.testing.assert_array_equal(reward, np.array([2.0 ** -30, 1.0, 2.0 ** -30, 1.0], np.float32))
    assert np.float32(np.float32(1.0 + 2.0 ** -30) + np.float32(-1.0)) == 0        # what a float32 sum gives
    assert_same(torch_gpu, buf, ref)


def test_gather_repeats_and_orders(torch_gpu):
    """Repeated indices, newest first, and a batch large enough for the gather's
    capped grid to go round several times (250 001 rows of 9 packed bytes)."""
    torch = torch_gpu
    rs = np.random.RandomState(9)
    buf, ref = new_pair((4, 3, 3, 8), 997)
    for _ in range(3):
        push_both(torch, buf, ref, random_step(rs, 150, 4, 3, 3, 8))
    size = len(ref)
    assert size == 997
    full = {fmt: ref.rows(format=fmt) for fmt in ('uint8', 'float32')}
    for idx in (np.arange(size)[::-1].copy(), np.array([3, 3, 0, size - 1, 3, size - 1]),
                rs.randint(0, size, size=250001)):
        for fmt in ('uint8', 'float32'):
            got = buf.sample(idx=torch.from_numpy(idx).cuda(), format=fmt)
            assert_rows(got, tuple(a[idx] for a in full[fmt]))
    assert_rows(buf.sample(idx=torch.tensor([5, 1, 5], device='cuda')), ref.rows([5, 1, 5]))


def test_many_envs(torch_gpu):
    """More than 1 024 scan blocks (k_replay_scan's threads then take two block
    totals each): 1 049 300 envs of one snake and one cell, every transition
    tagged by its action and reward."""
    torch = torch_gpu
    rs = np.random.RandomState(10)
    N = 1024 * 1024 + 724
    buf, ref = new_pair((1, 1, 1, 8), N, early_death=None)
    x = random_step(rs, N, 1, 1, 1, 8)
    x['actions'] = (np.arange(N) % 127).astype(np.int8).reshape(N, 1)
    x['rewards'] = np.arange(N, dtype=np.float64).reshape(N, 1)
    buf.push(**{k: torch.from_numpy(x[k]).cuda() for k in NAMES})
    kept = np.flatnonzero(x['skip'].reshape(-1) == 0)
    assert len(buf) == kept.size
    state, action, reward, nxt, done = (t.cpu().numpy() for t in buf.sample(idx=torch.arange(kept.size, device='cuda')))
    np.testing.assert_array_equal(reward, kept.astype(np.float32))
    np.testing.assert_array_equal(action, x['actions'].reshape(-1)[kept].astype(np.int64))
    np.testing.assert_array_equal(done, x['done'].reshape(-1)[kept].astype(np.float32))
    np.testing.assert_array_equal(state, x['obs'].reshape(N, 1, 1, 8)[kept])
    np.testing.assert_array_equal(nxt, x['next_obs'].reshape(N, 1, 1, 8)[kept])
    # the newest 3 000 against the restatement, which a deque of 3 000 fed with the last envs gives
    tail = R.RefReplay(3000)
    tail.push(*(None if x[k] is None else x[k][-6000:] for k in NAMES))
    idx = torch.arange(kept.size - 3000, kept.size, device='cuda')
    for fmt in ('uint8', 'float32'):
        assert_rows(buf.sample(idx=idx, format=fmt), tail.rows(format=fmt))


def test_pushes_and_sample_without_sync(torch_gpu):
    torch = torch_gpu
    steps = [random_step(np.random.RandomState(20 + i), 37, 4, 5, 5, 8) for i in range(6)]
    dev = [{k: torch.from_numpy(x[k]).cuda() for k in NAMES} for x in steps]
    idx = torch.arange(101, device='cuda')
    results = []
    for sync in (False, True):
        buf, _ = new_pair((4, 5, 5, 8), 101)
        torch.cuda.synchronize()
        for x in dev:
            buf.push(**x)
            if sync:
                torch.cuda.synchronize()
        results.append(buf.sample(idx=idx))
    torch.cuda.synchronize()
    for a, b in zip(*results):
        assert torch.equal(a, b)
    ref = R.RefReplay(101, (10, -1.0))
    for x in steps:
        ref.push(*(x[k] for k in NAMES))
    assert_rows(results[0], ref.rows())


def test_sample_without_replacement(torch_gpu):
    """B distinct indices inside [0, size): every transition is tagged by its
    reward (its index) and carries the index's bits in its observation."""
    torch = torch_gpu
    from marlenv import ReplayBuffer
    n, cap, B = 120, 200, 50
    buf = ReplayBuffer((1, 1, 2, 8), cap)
    tags = np.arange(n)
    obs = ((tags[:, None] >> np.arange(16)) & 1).astype(np.uint8).reshape(n, 1, 1, 2, 8)
    buf.push(torch.from_numpy(obs).cuda(), torch.from_numpy(1 - obs).cuda(),
             torch.from_numpy((tags % 3).astype(np.int8).reshape(n, 1)).cuda(),
             torch.from_numpy(tags.astype(np.float64).reshape(n, 1)).cuda(), torch.zeros((n, 1), dtype=torch.bool, device='cuda'))

    def draw(seed, **kw):
        g = torch.Generator(device='cuda').manual_seed(seed)
        state, action, reward, nxt, done = (t.cpu().numpy() for t in buf.sample(B, generator=g, **kw))
        tag = reward.astype(np.int64)
        assert tag.shape == (B,) and tag.min() >= 0 and tag.max() < n
        np.testing.assert_array_equal(action, tag % 3)
        np.testing.assert_array_equal(state.reshape(B, 16), (tag[:, None] >> np.arange(16)) & 1)
        np.testing.assert_array_equal(nxt, 1 - state)
        return tag

    a = draw(1)
    assert len(set(a.tolist())) == B                    # no repeats
    np.testing.assert_array_equal(draw(1), a)           # the same seed, the same batch
    assert set(draw(2).tolist()) != set(a.tolist())
    r = draw(3, replace=True)
    np.testing.assert_array_equal(draw(3, replace=True), r)
    f = buf.sample(B, format='float32', generator=torch.Generator(device='cuda').manual_seed(1))
    assert f[0].shape == (B, 8, 1, 2) and f[0].dtype == torch.float32
    np.testing.assert_array_equal(f[2].cpu().numpy().astype(np.int64), a)
    buf.clear()
    assert len(buf) == 0


def weighted_qnet(torch, h, w, c, seed):
    """Q-values that are exact in float32 and never tie: 3 * (an integer-weighted
    sum of the observation bytes) + the action's index."""
    g = torch.Generator().manual_seed(seed)
    weights = torch.randint(-8, 9, (3, h * w * c), generator=g).float().cuda()

    def qnet(obs):
        x = obs.reshape(obs.shape[0], 1, -1).float()
        return 3.0 * (x * weights[None]).sum(dim=2) + torch.arange(3, device=obs.device, dtype=torch.float32)

    return qnet


ENV = dict(num_snakes=3, height=10, width=10, vision_range=2, seed=3)


def test_collector_greedy(torch_gpu):
    """60 steps at epsilon 0 against a second env with the same seed, stepped by
    hand with the same rule and feeding the restatement: the buffers match,
    penalties and skipped snakes included."""
    torch = torch_gpu
    from marlenv import Collector, ReplayBuffer, SnakeVecEnv
    N, S = 8, 3
    env = SnakeVecEnv(N, **ENV)
    _, h, w, c = env.obs_shape
    qnet = weighted_qnet(torch, h, w, c, 0)
    buf = ReplayBuffer(env.obs_shape, 499, early_death=(10, -1.0))
    col = Collector(env, buf)
    col.run(qnet, 25)
    col.run(qnet, 35)                                   # (the state carries over)

    env2 = SnakeVecEnv(N, **ENV)
    ref = R.RefReplay(499, (10, -1.0))
    obs = env2.reset()
    mask = np.zeros((N, S), bool)
    counter = np.zeros(N, np.int32)
    penalties = 0
    for _ in range(60):
        q = qnet(obs.view(N * S, h, w, c)).cpu().numpy().reshape(N, S, 3)
        actions = np.where(mask, 0, q.argmax(axis=2)).astype(np.int8)
        next_obs, rewards, done, info = env2.step(torch.from_numpy(actions).cuda())
        ended = info['episode_done'].cpu().numpy()
        d = done.cpu().numpy()
        ref.push(obs.cpu().numpy(), next_obs.cpu().numpy(), actions, rewards.cpu().numpy(), d, mask, counter)
        penalties += int((d & ~mask & (counter[:, None] < 10)).sum())
        obs = next_obs
        mask = d & ~ended[:, None]
        counter = np.where(ended, 0, counter + 1).astype(np.int32)
    assert ref.count > 499 and penalties > 0 and ref.count < 60 * N * S      # it wrapped; penalties and skips occurred
    assert_same(torch, buf, ref)
    env.close()
    env2.close()


def test_collector_random(torch_gpu):
    """epsilon 1: every stored action is a uniform draw from {0, 1, 2}, so each
    share of at least 3 000 of them lies within 1/3 +- 0.05 (about six standard
    deviations); the same generator seed gives the same buffer. (The draws come
    from the device generator, which has no host restatement.)"""
    torch = torch_gpu
    from marlenv import Collector, ReplayBuffer, SnakeVecEnv

    def collect(seed):
        env = SnakeVecEnv(8, **ENV)
        _, h, w, c = env.obs_shape
        buf = ReplayBuffer(env.obs_shape, 4096, early_death=(10, -1.0))
        Collector(env, buf).run(weighted_qnet(torch, h, w, c, 0), 400, epsilon=1.0,
                                generator=torch.Generator(device='cuda').manual_seed(seed))
        size = len(buf)
        out = buf.sample(idx=torch.arange(size, device='cuda'))
        env.close()
        return size, out

    size, a = collect(11)
    assert size >= 3000
    share = np.bincount(a[1].cpu().numpy(), minlength=3) / size
    print('action shares', share, 'of', size)
    assert share.shape == (3,) and (np.abs(share - 1 / 3) <= 0.05).all(), share
    size2, b = collect(11)
    assert size2 == size
    for x, y in zip(a, b):
        assert torch.equal(x, y)
