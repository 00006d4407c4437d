"""Host checks of the device `random` streams (no GPU): the raw-word model the
kernels implement (tests/pyrandom_ref.py) against the stdlib, the integer
setsize rule, snake_pyrandom_plan's limits, and the argument checks of
ReplayBuffer.sample and PyRandom that come before any device work."""
import os
import random

import numpy as np
import pytest

import pyrandom_ref as PR


@pytest.fixture(scope='module')
def native():
    from marlenv import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _native


@pytest.mark.parametrize('seed', PR.SEEDS)
def test_model_draws_equal_stdlib(seed):
    """random(), randrange(n) and getrandbits(k) from raw words, interleaved:
    the values and the generator state afterwards."""
    a, b = random.Random(seed), random.Random(seed)
    u32 = PR.word_source(a)
    for i in range(700):
        n = (3, 1, 5, 127, 128, 2 ** 31 - 1)[i % 6]
        assert PR.random_double(u32) == b.random()
        assert PR.randbelow(u32, n) == b.randrange(n)
        k = 1 + i % 32
        assert PR.getrandbits(u32, k) == b.getrandbits(k)
    assert a.getstate() == b.getstate()


@pytest.mark.parametrize('n,k', PR.SAMPLE_CASES)
def test_model_sample_equals_stdlib(n, k):
    for seed in PR.SEEDS:
        a, b = random.Random(seed), random.Random(seed)
        assert PR.sample(PR.word_source(a), n, k) == b.sample(range(n), k), seed
        assert a.getstate() == b.getstate(), seed


def test_setsize_integer_rule(native):
    """The integer rule, the library's value and Lib/random.py's float formula
    agree for every batch the kernel takes."""
    from marlenv.pyrandom import setsize
    for k in range(1, 4097):
        want = PR.setsize_float(k)
        assert PR.setsize_int(k) == want, k
        assert setsize(k) == want, k
    assert PR.setsize_int(512) == 4117 and PR.setsize_int(4096) == 16405


def test_select_actions_is_the_reference_rule():
    """The restated loop draws two words per live snake, none for a skipped one,
    and _randbelow's words below epsilon."""
    q = np.array([[0, 2, 2], [1, 0, 0], [3, 3, 3]], np.float32)
    skip = np.array([False, True, False])
    a, b = random.Random(7), random.Random(7)
    assert PR.select_actions(a, q, skip, 0.0) == [1, 0, 0]
    for _ in range(4):
        b.getrandbits(32)
    assert a.getstate() == b.getstate()
    a, b = random.Random(7), random.Random(7)
    got = PR.select_actions(a, q, skip, 1.0)
    want = [(b.random(), b.randrange(3))[1], 0, (b.random(), b.randrange(3))[1]]
    assert got == want and a.getstate() == b.getstate()


def test_plan_limits(native):
    L = native.lib()

    def plan(A, B, cap):
        return native.check(L.snake_pyrandom_plan(A, B, cap), L)

    for A, B, cap in ((1, 1, 1), (127, 1, 1), (3, 4096, 4096), (3, 512, 2 ** 31 - 1)):
        assert plan(A, B, cap) == PR.setsize_int(B)
    for A, B, cap, field in ((0, 1, 1, 'num_actions'), (128, 1, 1, 'num_actions'), (-1, 1, 1, 'num_actions'),
                             (3, 0, 1, 'batch'), (3, 4097, 10000, 'batch'), (3, -5, 1, 'batch'),
                             (3, 32, 2 ** 31, 'capacity'), (3, 32, 2 ** 40, 'capacity'), (3, 32, 0, 'capacity')):
        with pytest.raises(ValueError, match=field):
            plan(A, B, cap)


def test_abi_version_is_unchanged(native):
    assert native.SNAKE_ABI_VERSION == 20 and native.lib().snake_abi_version() == 20
    for name in ('snake_pyrandom_plan', 'snake_pyrandom_act', 'snake_pyrandom_sample'):
        assert name in native.EXPORTS and hasattr(native.lib(), name)


def test_streams_are_seeded_by_the_stdlib(native):
    """Before the first use on a device the streams are the stdlib's states."""
    from marlenv import PyRandom
    r = PyRandom([3, 4])
    assert r.n == 2
    assert r.getstate(1) == random.Random(4).getstate()
    assert PyRandom(9).getstate(0) == random.Random(9).getstate()
    rnd = PR.advanced(5, 700)
    s = PyRandom.from_states([rnd.getstate()])
    assert s.n == 1 and s.getstate(0) == rnd.getstate()
    with pytest.raises(ValueError):
        PyRandom.from_states([(2, (0,) * 625, None)])
    with pytest.raises(ValueError):
        PyRandom([])
    with pytest.raises(IndexError):
        r.getstate(2)


def test_sample_argument_checks(native):
    """rng excludes replace=True and idx, and its limits are the plan's: all
    ValueErrors before any device work (this machine needs no GPU for them)."""
    import torch
    from marlenv import PyRandom, ReplayBuffer
    buf = ReplayBuffer((1, 3, 3, 8), 10000)
    r = PyRandom(0)
    with pytest.raises(ValueError, match='replace'):
        buf.sample(32, rng=r, replace=True)
    with pytest.raises(ValueError, match='idx'):
        buf.sample(idx=torch.zeros(4, dtype=torch.int64), rng=r)
    with pytest.raises(ValueError, match='batch'):
        buf.sample(4097, rng=r)
    with pytest.raises(TypeError):
        buf.sample(32, rng=random.Random(0))
    with pytest.raises(ValueError, match='capacity'):
        ReplayBuffer((1, 1, 1, 8), 2 ** 31).sample(32, rng=r)
    assert buf.count is None and r.key is None      # nothing was allocated
