"""CPU checks of the replay buffer (no GPU needed): the numpy-and-deque
restatement (tests/replay_ref.py) reproduces the reference's own deque
(tests/golden/replay_stream.npz), the host-side plan call returns the documented
sizes and rejects bad configs, and ReplayBuffer refuses wrong inputs before any
device work."""
import ctypes
import os

import numpy as np
import pytest

import replay_ref as R


@pytest.fixture(scope='module')
def native():
    from marlenv import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _native


@pytest.fixture(scope='module')
def stream():
    return R.load_stream()


def test_restatement_reproduces_the_reference(stream):
    d = stream
    ref = R.RefReplay(d['capacity'], d['early_death'])
    R.replay_stream(d, ref.push)
    assert len(ref) == d['capacity'] == 97 and ref.count > 4 * 97        # the ring wrapped several times
    state, action, reward, nxt, done = ref.rows()
    np.testing.assert_array_equal(state, d['final_state'])
    np.testing.assert_array_equal(nxt, d['final_next_state'])
    np.testing.assert_array_equal(action, d['final_action'])
    assert reward.dtype == np.float32 and reward.tobytes() == d['final_reward'].tobytes()
    np.testing.assert_array_equal(done, d['final_done'].astype(np.float32))


def test_fixture_covers_the_rules(stream):
    d = stream
    assert d['action'].shape == (300, 3) and d['obs'].shape == (300, 3, 10, 10, 8)
    assert d['early_death'] == (10, -1.0)
    stored = d['mask'] == 0
    assert stored.sum() >= 300 and (~stored).sum() >= 100                # stored and skipped snakes
    died = stored & (d['done'] == 1)
    early = died & (d['step'][:, None] < 10)
    assert early.sum() >= 20 and (died & ~early).sum() >= 5              # with and without the penalty
    assert (d['step'] == 0).sum() >= 10 and d['step'].max() == 39        # many episodes, some cut at the cap
    assert len(set(d['reward'].reshape(-1).tolist())) >= 4               # float64 rewards that float32 rounds


def test_restatement_formats_and_order():
    rs = np.random.RandomState(0)
    ref = R.RefReplay(5)
    obs = rs.randint(0, 2, size=(2, 6, 3, 4, 8)).astype(np.uint8)
    nxt = rs.randint(0, 2, size=(2, 6, 3, 4, 8)).astype(np.uint8)
    act = np.arange(12, dtype=np.int8).reshape(2, 6)
    ref.push(obs, nxt, act, np.zeros((2, 6)), np.zeros((2, 6), np.uint8))
    state, action, _, _, _ = ref.rows()
    np.testing.assert_array_equal(action, np.arange(7, 12))              # the last five, in (env, snake) order
    np.testing.assert_array_equal(state, obs.reshape(12, 3, 4, 8)[7:])
    f = ref.rows([4, 0, 4], 'float32')[0]
    assert f.shape == (3, 8, 3, 4) and f.dtype == np.float32
    np.testing.assert_array_equal(f[1], obs[1, 1].transpose(2, 0, 1))


def plan(native, h, w, c, S, capacity, N=0):
    cfg = native.ReplayCfg(h, w, c, S, capacity, 10, -1.0)
    lay = native.ReplayLayout()
    rc = native.lib().snake_replay_plan(ctypes.byref(cfg), N, ctypes.byref(lay))
    return rc, native.lib().snake_last_error().decode(), lay


def test_abi_version(native):
    assert native.SNAKE_ABI_VERSION == 20
    assert native.lib().snake_abi_version() == 20


def test_plan_sizes(native):
    rc, _, lay = plan(native, 11, 11, 8, 4, 1 << 20, 65536)
    assert rc == 0
    assert (lay.packed_row, lay.pitch) == (121, 128)                     # one byte per cell, rows at a 16-byte pitch
    assert lay.state == lay.next_state == (1 << 20) * 128
    assert (lay.action, lay.reward, lay.done, lay.count) == (1 << 20, 4 << 20, 1 << 20, 8)
    # the header (four int64), one int32 per 1 024-env block, one int32 per env
    assert lay.scratch == 32 + 64 * 4 + 65536 * 4
    rc, _, lay = plan(native, 20, 20, 16, 4, 1000, 1500)
    assert rc == 0 and (lay.packed_row, lay.pitch) == (800, 800) and lay.state == 800000
    assert lay.scratch == 32 + 4 * 4 + 1500 * 4                          # (two blocks, padded to four words)
    rc, _, lay = plan(native, 3, 3, 8, 1, 1, 1)
    assert rc == 0 and (lay.packed_row, lay.pitch) == (9, 16) and lay.scratch == 32 + 16 + 16
    assert plan(native, 1, 1, 8, 16, 1)[0] == 0


@pytest.mark.parametrize('args,msg', [
    ((11, 11, 12, 4, 100), 'obs_c'), ((11, 11, 0, 4, 100), 'obs_c'), ((11, 11, 8, 0, 100), 'num_snakes'),
    ((11, 11, 8, 17, 100), 'num_snakes'), ((11, 11, 8, 4, 0), 'capacity'), ((11, 11, 8, 4, -5), 'capacity'),
    ((0, 11, 8, 4, 100), 'obs_h'), ((11, 0, 8, 4, 100), 'obs_w'),
])
def test_plan_rejects(native, args, msg):
    rc, err, _ = plan(native, *args)
    assert rc == -1
    assert msg in err
    with pytest.raises(ValueError):
        native.check(rc)


def test_constructor_rejects_a_config_before_any_device_work(native):
    """No GPU here: the constructor raises from the host-side plan check."""
    from marlenv import ReplayBuffer
    for shape, cap, msg in (((4, 11, 11, 12), 100, 'obs_c'), ((17, 11, 11, 8), 100, 'num_snakes'),
                            ((4, 11, 11, 8), 0, 'capacity'), ((11, 11, 8), 100, 'obs_shape')):
        with pytest.raises(ValueError, match=msg):
            ReplayBuffer(shape, cap)
    ReplayBuffer((4, 11, 11, 8), 1 << 20, early_death=(10, -1.0))


def test_push_rejects_inputs_before_any_device_work(native):
    """Wrong dtypes raise TypeError, wrong shapes and host tensors ValueError:
    every check comes before the first allocation on a device."""
    import torch
    from marlenv import ReplayBuffer
    buf = ReplayBuffer((3, 5, 5, 8), 10)
    N, S = 2, 3

    def inputs():
        return dict(obs=torch.zeros((N, S, 5, 5, 8), dtype=torch.uint8),
                    next_obs=torch.zeros((N, S, 5, 5, 8), dtype=torch.uint8),
                    actions=torch.zeros((N, S), dtype=torch.int8), rewards=torch.zeros((N, S), dtype=torch.float64),
                    done=torch.zeros((N, S), dtype=torch.bool), skip=torch.zeros((N, S), dtype=torch.bool),
                    step=torch.zeros(N, dtype=torch.int32))

    wrong_type = dict(obs=torch.zeros((N, S, 5, 5, 8)), next_obs=torch.zeros((N, S, 5, 5, 8), dtype=torch.int8),
                      actions=torch.zeros((N, S), dtype=torch.int64), rewards=torch.zeros((N, S)),
                      done=torch.zeros((N, S)), skip=torch.zeros((N, S), dtype=torch.int32),
                      step=torch.zeros(N, dtype=torch.int64), )
    for k, v in wrong_type.items():
        with pytest.raises(TypeError, match=k):
            buf.push(**dict(inputs(), **{k: v}))
    with pytest.raises(TypeError, match='obs'):
        buf.push(**dict(inputs(), obs=np.zeros((N, S, 5, 5, 8), np.uint8)))
    with pytest.raises(TypeError, match='contiguous'):
        buf.push(**dict(inputs(), obs=torch.zeros((N, S, 5, 8, 5), dtype=torch.uint8).transpose(3, 4)))
    wrong_shape = dict(obs=torch.zeros((N, S, 5, 6, 8), dtype=torch.uint8),
                       next_obs=torch.zeros((N + 1, S, 5, 5, 8), dtype=torch.uint8),
                       actions=torch.zeros((N * S,), dtype=torch.int8),
                       rewards=torch.zeros((N, S + 1), dtype=torch.float64),
                       done=torch.zeros((S, N), dtype=torch.bool), skip=torch.zeros((N, 1), dtype=torch.bool),
                       step=torch.zeros((N, S), dtype=torch.int32))
    for k, v in wrong_shape.items():
        with pytest.raises(ValueError):
            buf.push(**dict(inputs(), **{k: v}))
    with pytest.raises(ValueError, match='GPU'):        # host tensors of the right types and shapes
        buf.push(**inputs())
    assert buf.count is None and len(buf) == 0          # nothing was allocated
    with pytest.raises(ValueError, match='format'):
        buf.sample(4, format='float16')
    with pytest.raises(ValueError, match='batch_size'):
        buf.sample()
    with pytest.raises(TypeError, match='idx'):
        buf.sample(idx=torch.zeros(4, dtype=torch.int32))
