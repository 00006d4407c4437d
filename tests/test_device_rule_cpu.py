"""The package's one device rule and its one tensor check (marlenv/_device.py),
on the host: what each kind of mismatch raises, and that an object which takes
its device from the first tensor it sees refuses host tensors before it binds
or allocates anything."""
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from dqn_probe import probe_net  # noqa: E402

N, S = 3, 2
OBS_SHAPE = (S, 5, 5, 8)


@pytest.fixture(scope='module')
def native():
    from marlenv import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _native


def _obs():
    return torch.zeros((N,) + OBS_SHAPE, dtype=torch.uint8)


# (kind, the argument, the class it raises)
MISMATCHES = (
    ('not a tensor', np.zeros((4, 5, 8), np.uint8), TypeError),
    ('wrong dtype', torch.zeros((4, 5, 8), dtype=torch.int8), TypeError),
    ('not contiguous', torch.zeros((4, 8, 5), dtype=torch.uint8).transpose(1, 2), TypeError),
    ('wrong shape', torch.zeros((4, 5, 9), dtype=torch.uint8), ValueError),
    ('wrong rank', torch.zeros((4, 5), dtype=torch.uint8), ValueError),
)


@pytest.mark.parametrize('kind,t,cls', MISMATCHES, ids=[m[0] for m in MISMATCHES])
def test_check_tensor_raises_per_kind_of_mismatch(kind, t, cls):
    from marlenv._device import check_tensor
    with pytest.raises(cls, match='frames') as e:
        check_tensor('Owner.method', 'frames', t, 'uint8', (None, 5, 8), contiguous=True)
    if cls is TypeError:
        assert 'uint8' in str(e.value) and 'Owner.method' in str(e.value)
    else:
        assert 'frames shape %s is not' % (tuple(t.shape),) in str(e.value)


def test_check_tensor_accepts():
    """An open batch dimension takes any size, zero included; several dtypes;
    contiguity only where it is asked for."""
    from marlenv._device import check_tensor
    for B in (0, 1, 7):
        check_tensor('who', 'frames', torch.zeros((B, 5, 8), dtype=torch.uint8), 'uint8', (None, 5, 8), contiguous=True)
    check_tensor('who', 'done', torch.zeros((2, 3), dtype=torch.bool), ('bool', 'uint8'), (2, 3))
    check_tensor('who', 'done', torch.zeros((2, 3), dtype=torch.uint8), ('bool', 'uint8'), (2, 3))
    check_tensor('who', 'frames', torch.zeros((4, 8, 5), dtype=torch.uint8).transpose(1, 2), 'uint8', (4, 5, 8))
    check_tensor('who', 'anything', torch.zeros((9, 1), dtype=torch.float32), 'float32')      # no shape asked
    with pytest.raises(ValueError, match='done shape'):
        check_tensor('who', 'done', torch.zeros((3, 2), dtype=torch.bool), ('bool', 'uint8'), (2, 3))
    with pytest.raises(TypeError, match='bool or uint8'):
        check_tensor('who', 'done', torch.zeros((2, 3), dtype=torch.int8), ('bool', 'uint8'), (2, 3))


def test_check_on_names_the_argument_and_both_devices():
    from marlenv._device import check_on
    t = torch.zeros(3)
    check_on('reward', t, torch.device('cpu'), 'Owner')
    with pytest.raises(ValueError, match='reward is on cpu, this Owner on cuda:1') as e:
        check_on('reward', t, torch.device('cuda', 1), 'Owner')
    assert 'no CPU fallback' in str(e.value)


def test_default_device_without_a_gpu_names_the_owner(monkeypatch):
    from marlenv._device import default_device
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    for device in (None, 'cuda', 'cuda:1'):
        with pytest.raises(RuntimeError, match=r'Owner needs a HIP device \(MI355X\); there is no CPU fallback'):
            default_device(device, 'Owner')


def test_constructors_without_a_gpu_raise_the_rule(native, monkeypatch):
    """The three that allocate at construction, and the two lazy binders when
    they must allocate before they saw a tensor."""
    from marlenv import DQNForward, DQNLearner, PyRandom, ReplayBuffer, SnakeVecEnv
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    state = probe_net(5, 5, 8, 3, 0)
    with pytest.raises(RuntimeError, match='SnakeVecEnv needs a HIP device'):
        SnakeVecEnv(4, num_snakes=2)
    with pytest.raises(RuntimeError, match='DQNLearner needs a HIP device'):
        DQNLearner(state, 5, 5, 8)
    for precision in ('bf16', 'fp32'):
        with pytest.raises(RuntimeError, match='DQNForward needs a HIP device'):
            DQNForward(state, 5, 5, 8, precision=precision)
    buf = ReplayBuffer(OBS_SHAPE, 16)
    with pytest.raises(RuntimeError, match='ReplayBuffer needs a HIP device'):
        buf.size()
    with pytest.raises(RuntimeError, match='ReplayBuffer needs a HIP device'):
        buf.sample(4, rng=PyRandom(0))
    assert buf.count is None and buf.device is None


def test_a_bad_config_is_rejected_before_the_device_is_asked(native, monkeypatch):
    """With a GPU present, resolving 'the current device' initialises it: the
    constructors reject what the host can reject first."""
    from marlenv import DQNForward, DQNLearner, SnakeVecEnv

    def asked():
        raise AssertionError('the current device was asked before the rejection')

    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'current_device', asked)
    state = probe_net(5, 5, 8, 3, 0)
    for device in (None, 'cuda'):
        with pytest.raises(ValueError):
            SnakeVecEnv(4, num_snakes=2, height=2, device=device)
        with pytest.raises(ValueError, match='num_actions'):
            DQNLearner(state, 5, 5, 8, 65, device=device)
        with pytest.raises(ValueError):
            DQNForward(state, 23, 23, 8, device=device)     # no bf16 plan takes 23x23


def test_dqn_forward_keeps_the_host_pack(native):
    from marlenv import DQNForward
    fwd = DQNForward(probe_net(5, 5, 8, 3, 0), 5, 5, 8, 3, device='cpu')
    assert fwd.device == torch.device('cpu') and fwd.plan == 'window'
    assert all(t.device.type == 'cpu' for t in fwd.tensors.values())


def _safe(native):
    from marlenv import SafeActions
    p = SafeActions(OBS_SHAPE)
    return p, lambda: p(_obs(), torch.zeros((N, S, 3))), lambda: p.dirs


def _greedy(native):
    from marlenv import GreedyActions
    p = GreedyActions(OBS_SHAPE)
    return p, lambda: p(_obs()), lambda: p.dirs


def _genome(native):
    from marlenv.neat_head import GenomeHeads
    p = GenomeHeads.from_linear(np.ones((3, 4)), np.zeros(3), num_envs=N)
    return p, lambda: p(torch.zeros((N * S, 4))), lambda: p._dev_prog


def _replay(native):
    from marlenv import ReplayBuffer
    p = ReplayBuffer(OBS_SHAPE, 16)
    call = lambda: p.push(_obs(), _obs(), torch.zeros((N, S), dtype=torch.int8),      # noqa: E731
                          torch.zeros((N, S), dtype=torch.float64), torch.zeros((N, S), dtype=torch.bool))
    return p, call, lambda: p.count


def _pyrandom_act(native):
    from marlenv import PyRandom
    p = PyRandom(range(N))
    return p, lambda: p.act(torch.zeros((N * S, 3)), S, 0.5, skip=torch.zeros((N, S), dtype=torch.bool)), lambda: p.key


def _pyrandom_sample(native):
    from marlenv import PyRandom
    p = PyRandom(range(N))
    return p, lambda: p.sample(torch.full((1,), 9, dtype=torch.int64), 16, 4), lambda: p.key


@pytest.mark.parametrize('make', [_safe, _greedy, _genome, _replay, _pyrandom_act, _pyrandom_sample],
                         ids=lambda f: f.__name__.strip('_'))
def test_lazy_binders_refuse_host_tensors_before_binding(native, make):
    """Built without a device and called with well-formed host tensors: a
    ValueError, no device bound and nothing allocated -- twice, so the first
    refusal left no state behind."""
    obj, call, allocated = make(native)
    assert obj.device is None
    for _ in range(2):
        with pytest.raises(ValueError, match='no CPU fallback'):
            call()
        assert obj.device is None and allocated() is None
