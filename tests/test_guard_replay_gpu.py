"""snake_replay_push / snake_replay_gather called directly on buffers of exactly
snake_replay_plan's byte counts, inside a guard-band arena (tests/guard_util.py):
the rings at their 16-byte pitch with prime capacities, the count, the push
scratch planned for that N, and every gather output at its exact size in both
formats. After every push the guards are checked and the whole ring is read
back against the numpy-and-deque restatement (tests/replay_ref.py).

A read outside a buffer is invisible to this method."""
import ctypes

import numpy as np
import pytest

import replay_ref as R
from guard_util import Arena

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
RINGS = ('state', 'next_state', 'action', 'reward', 'done', 'count')
FORMATS = {'uint8': 0, 'float32': 1}        # SNAKE_REPLAY_U8_NHWC, SNAKE_REPLAY_F32_NCHW


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    from marlenv import _native
    _native.lib()


def next_prime(n):
    while any(n % d == 0 for d in range(2, int(n ** 0.5) + 1)):
        n += 1
    return n


class GuardedReplay:
    """The rings of one (S, h, w, C, capacity) and the scratch for pushes of N
    envs, zeroed (rings, count) or 0x5A (scratch), in one arena."""

    def __init__(self, N, shape, capacity, early_death=(10, -1.0)):
        from marlenv import _native
        self.nat, self.L = _native, _native.lib()
        S, h, w, c = shape
        self.N, self.shape, self.capacity = N, shape, capacity
        self.cfg = _native.ReplayCfg(h, w, c, S, capacity, int(early_death[0]), float(early_death[1]))
        self.lay = lay = _native.ReplayLayout()
        _native.check(self.L.snake_replay_plan(ctypes.byref(self.cfg), N, ctypes.byref(lay)), self.L)
        assert lay.packed_row == h * w * c // 8 and lay.pitch == (lay.packed_row + 15) // 16 * 16
        assert lay.state == lay.next_state == capacity * lay.pitch and lay.count == 8
        assert (lay.action, lay.reward, lay.done) == (capacity, 4 * capacity, capacity)
        sizes = [int(getattr(lay, k)) for k in RINGS] + [int(lay.scratch)]
        self.arena = ar = Arena(sizes)
        for k in RINGS:
            ar.take(k, getattr(lay, k), fill='zero')
        ar.take('scratch', lay.scratch)
        self.rings = _native.ReplayRings(*[ar.ptr(k) for k in RINGS])

    def push(self, obs, next_obs, actions, rewards, done, skip=None, step=None):
        """ReplayBuffer.push's signature (replay_ref.push_both), device tensors."""
        assert obs.shape[0] == self.N
        self.arena.refill('scratch')        # (its contents need not survive a call)
        args = [P(t.data_ptr()) if t is not None else None for t in (obs, next_obs, actions, rewards, done, skip, step)]
        self.nat.check(self.L.snake_replay_push(ctypes.byref(self.cfg), ctypes.byref(self.rings), *args, self.N,
                                                self.arena.ptr('scratch'), None), self.L)
        self.arena.check('push')

    def count(self):
        return int(self.arena.payload('count').view(torch.int64).item())

    def gather(self, idx, fmt):
        """The five tensors of logical indices idx, each at its exact size in an
        arena of its own; numpy arrays shaped as ReplayBuffer.sample's."""
        S, h, w, c = self.shape
        B = len(idx)
        nstate = B * h * w * c * (4 if fmt == 'float32' else 1)
        sizes = dict(state=nstate, next_state=nstate, action=8 * B, reward=4 * B, done=4 * B, idx=8 * B)
        ar = Arena(sizes.values())
        for k, n in sizes.items():
            ar.take(k, n)
        ar.payload('idx').copy_(torch.from_numpy(np.asarray(idx, np.int64).view(np.uint8)))
        self.nat.check(self.L.snake_replay_gather(
            ctypes.byref(self.cfg), ctypes.byref(self.rings), ar.ptr('idx'), B, FORMATS[fmt], ar.ptr('state'),
            ar.ptr('next_state'), ar.ptr('action'), ar.ptr('reward'), ar.ptr('done'), None), self.L)
        ar.check(f'gather B={B} {fmt}')
        self.arena.check(f'gather B={B} {fmt} (rings)')
        raw = {k: ar.payload(k).cpu().numpy() for k in sizes}
        assert (raw['idx'].view(np.int64) == idx).all()
        sdt, sshape = (np.float32, (B, c, h, w)) if fmt == 'float32' else (np.uint8, (B, h, w, c))
        return (raw['state'].view(sdt).reshape(sshape), raw['action'].view(np.int64), raw['reward'].view(np.float32),
                raw['next_state'].view(sdt).reshape(sshape), raw['done'].view(np.float32))


def assert_rows(got, want, where):
    for name, g, w_ in zip(('state', 'action', 'reward', 'next_state', 'done'), got, want):
        assert g.dtype == w_.dtype and g.shape == w_.shape, (where, name, g.dtype, g.shape, w_.dtype, w_.shape)
        assert g.tobytes() == w_.tobytes(), (where, name)       # an unwritten byte reads 0x5A


def assert_ring(buf, ref, formats, where):
    size = len(ref)
    assert buf.count() == ref.count, where
    if size:
        for fmt in formats:
            assert_rows(buf.gather(np.arange(size), fmt), ref.rows(format=fmt), f'{where} {fmt}')


# 3-byte rows; 70 bytes at pitch 80; a 256-byte row, exactly one pass of a wave; 400 bytes, two passes
SHAPES = [(1, 1, 3, 3, 8), (7, 2, 1, 3, 8), (5, 3, 7, 5, 16), (2, 3, 16, 16, 8), (3, 2, 20, 20, 8)]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_pushes_and_gathers(shape):
    """Six pushes into a ring of prime capacity above twice a call's snakes: it
    wraps at another slot each time. Then gathers of 1, 3 and 257 rows with
    repeats and newest-first order."""
    N, S, h, w, C = shape
    rs = np.random.RandomState(sum(shape))
    capacity = next_prime(2 * N * S + 1)
    buf, ref = GuardedReplay(N, (S, h, w, C), capacity), R.RefReplay(capacity, (10, -1.0))
    for i in range(6):
        R.push_both(torch, buf, ref, R.random_step(rs, N, S, h, w, C, p_skip=0.0 if N * S == 1 else 0.3))
        assert_ring(buf, ref, ('uint8',) if i < 5 else ('uint8', 'float32'), f'push {i}')
    assert ref.count > capacity                         # it wrapped
    size = len(ref)
    full = {fmt: ref.rows(format=fmt) for fmt in FORMATS}
    for idx in (np.array([size - 1]), np.array([3 % size, 3 % size, 0]), (size - 1 - np.arange(257)) % size,
                rs.randint(0, size, size=257)):
        for fmt in FORMATS:
            assert_rows(buf.gather(idx, fmt), tuple(a[idx] for a in full[fmt]), f'B={len(idx)} {fmt}')


def test_one_push_stores_more_than_the_capacity():
    """12 snakes into capacity 5, from an empty and from a full ring."""
    rs = np.random.RandomState(5)
    buf, ref = GuardedReplay(3, (4, 3, 3, 8), 5), R.RefReplay(5, (10, -1.0))
    for i in range(2):
        x = R.random_step(rs, 3, 4, 3, 3, 8)
        x['skip'] = None
        R.push_both(torch, buf, ref, x)
        assert len(ref) == 5 and ref.count == 12 * (i + 1)
        assert_ring(buf, ref, FORMATS, f'push {i}')
    np.testing.assert_array_equal(buf.gather(np.arange(5), 'uint8')[1], x['actions'].reshape(-1)[7:])
