"""The device `random` streams (snake_pyrandom_act / snake_pyrandom_sample,
pyrandom_kernels.hip) against the stdlib `random` module on the host: every
action, every minibatch index and every generator state afterwards is equal.
The loops of the reference trainer are restated in tests/pyrandom_ref.py."""
import random

import numpy as np
import pytest

import pyrandom_ref as PR
from guard_util import Arena

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), 'needs the GPU'
    return torch


def held_buffer(torch, capacity, count):
    """A ReplayBuffer of 3x3x8 observations whose device counter says `count`."""
    from marlenv import ReplayBuffer
    buf = ReplayBuffer((1, 3, 3, 8), capacity)
    buf._own_device()
    buf.count.fill_(count)
    return buf


def check_samples(torch, buf, n, B, rnds):
    """One sample(B) per generator of rnds, each from a stream of its own that
    starts in the generator's state: indices, states afterwards, err, and no
    write behind idx[B - 1]."""
    from marlenv import PyRandom
    rng = PyRandom.from_states([r.getstate() for r in rnds])
    arena = Arena([B * 8] * len(rnds))
    outs = [arena.take('idx%d' % i, B * 8, dtype=torch.int64) for i in range(len(rnds))]
    for i, out in enumerate(outs):
        assert rng.sample(buf.count, buf.capacity, B, stream=i, out=out) is out
    arena.check('snake_pyrandom_sample n=%d B=%d' % (n, B))
    for i, (rnd, out) in enumerate(zip(rnds, outs)):
        assert out.cpu().tolist() == rnd.sample(range(n), B), (n, B, i)
        assert rng.getstate(i) == rnd.getstate(), (n, B, i)
    assert int(rng.err.item()) == 0
    return rng


SAMPLE_CASES = [(n, B, n, n) for n, B in PR.SAMPLE_CASES] + [(10000, 512, 10000, 3 * 10000 + 7)]


@pytest.mark.parametrize('n,B,capacity,count', SAMPLE_CASES)
def test_sample_equals_random_sample(torch_gpu, n, B, capacity, count):
    """Every branch edge of random.sample, six seeds each; the last case is the
    wrapped ring (count = 3 * capacity + 7, n = capacity)."""
    torch = torch_gpu
    buf = held_buffer(torch, capacity, count)
    check_samples(torch, buf, n, B, [random.Random(s) for s in PR.SEEDS])
    # the public path: the batch is the gather of those indices
    from marlenv import PyRandom
    rnd = random.Random(11)
    got = buf.sample(B, rng=PyRandom(11))
    want = buf.sample(idx=torch.tensor(rnd.sample(range(n), B), device='cuda'))
    for g, w in zip(got, want):
        assert torch.equal(g, w)


@pytest.mark.parametrize('n', (5, 21, 22, 1000))
def test_sample_straddles_the_twist(torch_gpu, n):
    """B = 5 from streams pre-advanced by 617 .. 624 words: a draw begins before
    the key boundary and ends behind it, at each offset (624: the twist is the
    call's first act; 619 and below at n = 1000: it falls between two draws)."""
    torch = torch_gpu
    buf = held_buffer(torch, max(n, 5), n)
    check_samples(torch, buf, n, 5, [PR.advanced(2, words) for words in range(617, 625)])


def test_sample_more_than_held_sets_err(torch_gpu):
    """n < B: err becomes 1, the indices stay inside [0, max(n, 1)) and the
    stream does not move; err is sticky, and a later valid call draws the
    stdlib's indices for the state it started from."""
    torch = torch_gpu
    from marlenv import PyRandom
    rng = PyRandom([4])
    start = rng.getstate(0)
    for held in (0, 7, 31):
        buf = held_buffer(torch, 64, held)
        idx = rng.sample(buf.count, buf.capacity, 32)
        assert int(rng.err.item()) == 1
        idx = idx.cpu().numpy()
        assert idx.min() >= 0 and idx.max() < max(held, 1), held
    assert rng.getstate(0) == start
    rnd = random.Random()
    rnd.setstate(rng.getstate(0))
    buf = held_buffer(torch, 64, 40)
    assert rng.sample(buf.count, buf.capacity, 32).cpu().tolist() == rnd.sample(range(40), 32)
    assert rng.getstate(0) == rnd.getstate()
    assert int(rng.err.item()) == 1


def act_inputs(N, S, A, T, seed):
    """Q-values of small integers (exact ties, the maximum in every position)
    and random skip masks with one env all skipped."""
    rs = np.random.RandomState(seed)
    q = rs.randint(0, 4, size=(T, N * S, A)).astype(np.float32)
    skip = rs.rand(T, N, S) < 0.3
    if N > 1:
        skip[:, N // 2, :] = True
    else:
        skip[::4, 0, :] = True
    return q, skip


@pytest.mark.parametrize('epsilon', (0.0, 0.3, 1.0))
@pytest.mark.parametrize('A', (1, 3, 5))
@pytest.mark.parametrize('S', (1, 4, 16))
@pytest.mark.parametrize('N', (1, 65, 130))
def test_act_equals_the_reference_loop(torch_gpu, N, S, A, epsilon):
    """48 consecutive calls; stream e starts 37 e words into its generator, so
    the streams cross their key boundaries at different calls (at S = 16 each
    at least twice)."""
    torch = torch_gpu
    from marlenv import PyRandom
    T = 48
    q, skip = act_inputs(N, S, A, T, 1000 * N + 10 * S + A)
    rnds = [PR.advanced(100 + e, 37 * e) for e in range(N)]
    rng = PyRandom.from_states([r.getstate() for r in rnds])
    qd, sd = torch.from_numpy(q).cuda(), torch.from_numpy(skip).cuda()
    got = torch.stack([rng.act(qd[t], S, epsilon, skip=sd[t]) for t in range(T)]).cpu().numpy()
    assert got.dtype == np.int8 and got.shape == (T, N, S)
    want = np.array([[PR.select_actions(rnds[e], q[t, e * S:(e + 1) * S], skip[t, e], epsilon) for e in range(N)]
                     for t in range(T)])
    np.testing.assert_array_equal(got, want)
    for e in range(N):
        assert rng.getstate(e) == rnds[e].getstate(), e
    assert int(rng.err.item()) == 0
    if epsilon == 0.0 and N * S >= 65:
        assert set(np.unique(want)) == set(range(A))    # (the inputs: the maximum stood in every position)


def test_act_without_skip_uses_the_first_streams(torch_gpu):
    """skip=None stores an action for every snake; a PyRandom with more streams
    than envs leaves the others alone."""
    torch = torch_gpu
    from marlenv import PyRandom
    N, S, A = 3, 4, 3
    rnds = [random.Random(s) for s in range(5)]
    rng = PyRandom(list(range(5)))
    q = np.random.RandomState(0).randint(0, 3, size=(N * S, A)).astype(np.float32)
    got = rng.act(torch.from_numpy(q).cuda(), S, 0.5).cpu().numpy()
    want = [PR.select_actions(rnds[e], q[e * S:(e + 1) * S], np.zeros(S, bool), 0.5) for e in range(N)]
    np.testing.assert_array_equal(got, np.array(want))
    for e in range(5):
        assert rng.getstate(e) == rnds[e].getstate(), e


def test_trainer_interleaving(torch_gpu):
    """num_envs = 1 and one stream: 40 steps of act on recorded Q-values and
    done masks, each followed by sample(32) once 96 transitions are held in a
    ring of 100, against ONE random.Random driven by the restated loop of
    Trainer.train: every action, every index, the final state."""
    torch = torch_gpu
    from marlenv import PyRandom
    S, A, T, B, seed = 4, 3, 40, 32, 2024
    q, _ = act_inputs(1, S, A, T, 5)
    skip = np.random.RandomState(6).rand(T, 1, S) < 0.15
    skip[20] = True                     # a step in which nobody lives draws nothing
    rnd = random.Random(seed)
    want_actions, want_batches = PR.trainer_loop(rnd, q, skip[:, 0], 0.3, B, 96, 100)
    assert sum(b is not None for b in want_batches) >= 5

    rng = PyRandom(seed)
    buf = held_buffer(torch, 100, 0)
    qd, sd = torch.from_numpy(q).cuda(), torch.from_numpy(skip).cuda()
    held, actions, batches = 0, [], []
    for t in range(T):
        actions.append(rng.act(qd[t], S, 0.3, skip=sd[t]))
        live = int((~skip[t]).sum())
        buf.count += live
        held += live
        batches.append(rng.sample(buf.count, buf.capacity, B) if min(held, 100) >= 96 else None)
    assert [a.cpu().tolist()[0] for a in actions] == want_actions
    assert [b.cpu().tolist() if b is not None else None for b in batches] == want_batches
    assert rng.getstate(0) == rnd.getstate()
    assert int(rng.err.item()) == 0


def test_public_path_is_reproducible(torch_gpu):
    """Collector.run(..., rng=r) on 64 envs, then buf.sample(64, rng=r,
    stream=64) from a 65-stream PyRandom: the same seeds give byte-equal rings
    and batches, other seeds different ones."""
    torch = torch_gpu
    from marlenv import Collector, PyRandom, ReplayBuffer, SnakeVecEnv
    from test_replay_gpu import ENV, weighted_qnet

    def collect(first_seed):
        env = SnakeVecEnv(64, **ENV)
        _, h, w, c = env.obs_shape
        buf = ReplayBuffer(env.obs_shape, 4096, early_death=(10, -1.0))
        r = PyRandom(list(range(first_seed, first_seed + 65)))
        Collector(env, buf).run(weighted_qnet(torch, h, w, c, 0), 8, 0.3, rng=r)
        ring = buf.sample(idx=torch.arange(len(buf), device='cuda'))
        batch = buf.sample(64, rng=r, stream=64)
        env.close()
        assert int(r.err.item()) == 0
        return [t.cpu().numpy().tobytes() for t in ring + batch]

    a, b, c = collect(0), collect(0), collect(1000)
    assert a == b
    assert a[1] != c[1] and a[5:] != c[5:]      # the rings' actions, the batches
