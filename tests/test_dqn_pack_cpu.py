"""CPU checks of the pack (no GPU needed): snake_dqn_pack32_host -- the host
twin that shares the kernel's index mappings and rounding -- against the torch
packing of tests/dqn_pack_ref.py run on the CPU, bit for bit, on real-valued nets
with the crafted rounding cases of tests/dqn_pack_cases.py; the same for a
DQNForward built from a state dict, which packs through the twin; what the
plans reject; the exports."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dqn_pack_cases as PC


@pytest.fixture(scope='module')
def native():
    from marlenv import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _native


def host_pack(state, plan, h, w, c, A):
    """DQNForward.empty on the CPU, its buffers 0xFF-filled, packed by the host twin."""
    from marlenv.dqn import DQNForward
    fwd = DQNForward.empty(h, w, c, num_actions=A, device='cpu', plan=plan)
    assert fwd.plan == plan
    PC.fill_ff(fwd)
    keep, net32 = PC.kernel_net(state, h, w)
    fwd.pack32(net32)
    return fwd, keep


@pytest.mark.parametrize('plan,h,w,c,A', PC.CASES, ids=PC.IDS)
def test_host_pack_equals_the_torch_packing(native, plan, h, w, c, A):
    state, want = PC.case(plan, h, w, c, A)
    fwd, _ = host_pack(state, plan, h, w, c, A)
    PC.assert_equal_bits(PC.packed_bits(fwd), want, PC.IDS[PC.CASES.index((plan, h, w, c, A))])


def test_crafted_values_round_as_stated():
    """The crafted list does hold a tie of each parity, both neighbours of a tie,
    and values that overflow and underflow: torch's own rounding of it."""
    got = torch.from_numpy(PC.CRAFTED.copy()).to(torch.bfloat16).view(torch.int16).numpy().astype(np.int64) & 0xffff
    want = [0x0000, 0x8000, 0x3f80, 0x3f82, 0x3f80, 0x3f81, 0x0001, 0x0080, 0x7f80, 0xff80, 0x7f80,
            0xff80, 0xbf80, 0xbf82, 0x8001, 0x3f81]
    assert [int(v) for v in got] == want


def test_padding_is_written_as_zero(native):
    """11x11x24 pads the channels to 32 and has 7 padding rows in 128: those
    elements are +0 after a pack over 0xFF bytes, and nowhere does 0xFFFF stay."""
    state, _ = PC.case('window', 11, 11, 24, 3)
    fwd, _ = host_pack(state, 'window', 11, 11, 24, 3)
    lay = fwd.layout
    assert (lay.cpad, lay.k1, lay.p16) == (32, 288, 128)
    for k in PC.BF16:
        assert not bool((fwd.tensors[k] == -1).any()), k
    # conv1 element (o, k): ((o/16 * K/32 + k/32) * 4 + (k%32)/8) * 128 + (o%16) * 8 + k%8
    w1 = fwd.tensors['conv1_w']
    for o, tap, ci in ((0, 0, 24), (17, 8, 31), (31, 4, 27)):
        k = tap * 32 + ci
        assert int(w1[((o // 16 * 9 + k // 32) * 4 + (k % 32) // 8) * 128 + (o % 16) * 8 + k % 8]) == 0
    rows = fwd._rows.tolist()
    assert rows.count(-1) == 7 and sorted(r for r in rows if r >= 0) == list(range(121))
    fc1 = fwd.tensors['fc1_w'].view(256, 8, 2, 4, 16, 2, 4)      # n, m, half, quad, c16, j, r
    for i, p in enumerate(rows):
        if p < 0:
            assert not bool(fc1[:, i // 16, :, (i % 16) // 4, :, :, i % 4].any()), i


def test_nan_packs_to_nan(native):
    state = PC.real_state(3, 3, 8, 3, crafted=False)
    # the smallest signalling NaN (the plain rounding formula would make it inf),
    # the default quiet NaN, and the two all-ones patterns (which would wrap to zero)
    nans = torch.from_numpy(np.array([0x7f800001, 0x7fc00000, 0xffffffff, 0x7fffffff], np.uint32).view(np.float32))
    for name in ('conv1.weight', 'conv2.weight', 'conv3.weight', 'fc1.weight', 'fc2.weight'):
        state[name].view(-1)[:4] = nans
        assert bool(state[name].view(-1)[:4].isnan().all())
    fwd, _ = host_pack(state, 'window', 3, 3, 8, 3)
    for k in PC.BF16:
        got = fwd.tensors[k].view(torch.bfloat16).float()
        assert int(got.isnan().sum()) == 4, k
        assert not bool(got.isinf().any()), k


def test_every_call_overwrites_everything(native):
    """A second net packed into the same buffers leaves nothing of the first."""
    from marlenv.dqn import DQNForward
    h, w, c, A = 4, 6, 8, 3
    fwd = DQNForward.empty(h, w, c, num_actions=A, device='cpu', plan='map')
    first = PC.real_state(h, w, c, A, seed=1)
    second, want = PC.case('map', h, w, c, A)
    for state in (first, second):
        keep, net32 = PC.kernel_net(state, h, w)
        fwd.pack32(net32)
    PC.assert_equal_bits(PC.packed_bits(fwd), want)


def padding_is_zero(fwd):
    """What 11x11x24 must show: channels padded to 32, 7 padding rows in 128,
    all of them +0, and 0xFFFF nowhere."""
    lay = fwd.layout
    assert (lay.cpad, lay.k1, lay.p16) == (32, 288, 128)
    for k in PC.BF16:
        assert not bool((fwd.tensors[k] == -1).any()), k
    # conv1 element (o, k): ((o/16 * K/32 + k/32) * 4 + (k%32)/8) * 128 + (o%16) * 8 + k%8
    w1 = fwd.tensors['conv1_w']
    for o, tap, ci in ((0, 0, 24), (17, 8, 31), (31, 4, 27)):
        k = tap * 32 + ci
        assert int(w1[((o // 16 * 9 + k // 32) * 4 + (k % 32) // 8) * 128 + (o % 16) * 8 + k % 8]) == 0
    rows = fwd._rows.tolist()
    assert rows.count(-1) == 7 and sorted(r for r in rows if r >= 0) == list(range(121))
    fc1 = fwd.tensors['fc1_w'].view(256, 8, 2, 4, 16, 2, 4)      # n, m, half, quad, c16, j, r
    for i, p in enumerate(rows):
        if p < 0:
            assert not bool(fc1[:, i // 16, :, (i % 16) // 4, :, :, i % 4].any()), i


@pytest.mark.parametrize('plan,h,w,c,A', PC.CASES, ids=PC.IDS)
def test_constructor_equals_the_torch_packing(native, plan, h, w, c, A):
    """A DQNForward built from a state dict packs through the host twin into
    buffers that are not zero-initialised: every bit is the model's."""
    from marlenv.dqn import DQNForward
    state, want = PC.case(plan, h, w, c, A)
    fwd = DQNForward(state, h, w, c, num_actions=A, device='cpu', plan=plan)
    assert fwd.plan == plan and fwd.precision == 'bf16' and fwd._source is None
    PC.assert_equal_bits(PC.packed_bits(fwd), want, PC.IDS[PC.CASES.index((plan, h, w, c, A))])
    if (plan, h, w, c) == ('window', 11, 11, 24):
        padding_is_zero(fwd)


def test_fp32_mode_holds_the_kernel_layout(native):
    from marlenv.dqn import DQNForward
    from marlenv.learner import FIELDS, NAMES, to_kernel
    h, w, c, A = 3, 4, 8, 3
    state = PC.real_state(h, w, c, A)
    fwd = DQNForward(state, h, w, c, num_actions=A, precision='fp32', device='cpu')
    assert fwd.plan is None and tuple(fwd.tensors) == FIELDS
    for field, name in zip(FIELDS, NAMES):
        t = fwd.tensors[field]
        assert t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0, field
        assert torch.equal(PC.bits(t), PC.bits(to_kernel(name, state[name], h * w))), field
        assert getattr(fwd.net, field) == t.data_ptr(), field
    with pytest.raises(ValueError):
        fwd.pack32(fwd.net)


def test_constructor_packs_nan_to_nan(native):
    """The NaN patterns of test_nan_packs_to_nan in a state dict: each bf16
    tensor holds exactly four NaN and no infinity. Which quiet NaN a NaN becomes
    is the pack's choice (bf16_rne in dqn_pack_kernels.hip) since the
    constructor packs through it; it was torch's before. Their bits are not
    pinned."""
    from marlenv.dqn import DQNForward
    state = PC.real_state(3, 3, 8, 3, crafted=False)
    nans = torch.from_numpy(np.array([0x7f800001, 0x7fc00000, 0xffffffff, 0x7fffffff], np.uint32).view(np.float32))
    for name in ('conv1.weight', 'conv2.weight', 'conv3.weight', 'fc1.weight', 'fc2.weight'):
        state[name].view(-1)[:4] = nans
        assert bool(state[name].view(-1)[:4].isnan().all())
    fwd = DQNForward(state, 3, 3, 8, num_actions=3, device='cpu', plan='window')
    for k in PC.BF16:
        got = fwd.tensors[k].view(torch.bfloat16).float()
        assert int(got.isnan().sum()) == 4, k
        assert not bool(got.isinf().any()), k


def test_pack32_on_a_state_built_forward(native):
    """Every bf16 forward has the row table: pack32 replaces the weights of one
    built from a state dict."""
    from marlenv.dqn import DQNForward
    h, w, c, A = 4, 6, 8, 3
    fwd = DQNForward(PC.real_state(h, w, c, A, seed=1), h, w, c, num_actions=A, device='cpu', plan='map')
    second, want = PC.case('map', h, w, c, A)
    keep, net32 = PC.kernel_net(second, h, w)
    fwd.pack32(net32)
    PC.assert_equal_bits(PC.packed_bits(fwd), want)


@pytest.mark.parametrize('fn', ['snake_dqn_pack32', 'snake_dqn_pack32_host'])
@pytest.mark.parametrize('map_plan,geo,msg', [
    (0, (4, 6, 8, 3), 'vision_range'), (0, (13, 13, 8, 3), 'vision_range'), (0, (5, 5, 12, 3), 'channels'),
    (0, (5, 5, 8, 5), 'num_actions'), (0, (5, 5, 8, 3, 8), 'conv_waves'),
    (1, (40, 40, 8, 3), 'bordered'), (1, (20, 20, 64, 3), 'channels'), (1, (20, 20, 8, 5), 'num_actions'),
    (1, (20, 20, 8, 3, 4), 'conv_waves'),
])
def test_rejected_geometry_is_a_config_error(native, fn, map_plan, geo, msg):
    rc, err = PC.null_call(native, fn, PC.cfg_of(*geo), map_plan)
    assert rc == -1 and msg in err, (rc, err)
    with pytest.raises(ValueError):
        native.check(rc)


@pytest.mark.parametrize('fn', ['snake_dqn_pack32', 'snake_dqn_pack32_host'])
def test_null_arguments_are_refused(native, fn):
    rc, err = PC.null_call(native, fn, PC.cfg_of(5, 5, 8, 3), 0)       # an accepted cfg, NULL pointers
    assert rc == -2 and 'NULL' in err
    rc, err = PC.null_call(native, fn, PC.cfg_of(5, 5, 8, 3), 2)
    assert rc == -2 and 'map_plan' in err


def test_empty_and_learner_reject_before_any_device_work(native):
    """No bf16 plan takes 40x40, five actions or 64 channels: ValueError with the
    plan's message (this machine need not have a GPU: nothing touches one)."""
    from marlenv import DQNLearner
    from marlenv.dqn import DQNForward
    for geo, msg in (((40, 40, 8, 3), 'bordered'), ((5, 5, 8, 5), 'num_actions'), ((5, 5, 64, 3), 'channels')):
        h, w, c, A = geo
        with pytest.raises(ValueError, match=msg):
            DQNForward.empty(h, w, c, num_actions=A)
        with pytest.raises(ValueError, match=msg):
            DQNLearner({}, h, w, c, A, target_precision='bf16')
    with pytest.raises(ValueError, match='target_precision'):
        DQNLearner({}, 5, 5, 8, 3, target_precision='fp16')
    with pytest.raises(ValueError, match='plan'):
        DQNForward.empty(5, 5, 8, plan='tile')


def test_exports(native):
    L = native.lib()
    for n in ('snake_dqn_pack32', 'snake_dqn_pack32_host'):
        assert n in native.EXPORTS and hasattr(L, n)
    assert native.SNAKE_ABI_VERSION == 20 and L.snake_abi_version() == 20
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include',
                               'snake_env.h')).read()
    assert '#define SNAKE_ABI_VERSION 20' in header
    from marlenv.dqn import DQNForward
    assert callable(DQNForward.empty) and callable(DQNForward.pack32) and callable(DQNForward.sync)
