"""Nets, geometries and the ground truth of the pack tests (no GPU needed here),
so that tests/test_dqn_pack_cpu.py checks the host twin against exactly what
tests/test_dqn_pack_gpu.py holds the kernel to.

The integer probe nets of tests/dqn_probe.py are exactly representable in bf16
and cannot see the rounding, so the nets here are real-valued: seeded normal
weights scaled by 1/sqrt(fan_in), and in every tensor the first 16 entries are
the crafted values below -- signed zeros, exact ties with an even and with an
odd kept bit, one fp32 ulp either side of a tie, denormals, FLT_MIN, the
infinities and FLT_MAX (which rounds to inf). No NaN: the comparisons are on
bits, and a NaN's bits are not pinned.

The ground truth is the torch packing of tests/dqn_pack_ref.py (what
DQNForward.__init__ did before the library packed everything through
snake_dqn_pack32), run on the CPU."""
import ctypes
import functools

import numpy as np
import torch

# (plan, h, w, c)
GEOMETRIES = (
    ('window', 3, 3, 8),        # one row tile
    ('window', 5, 5, 16),
    ('window', 11, 11, 24),     # 121 positions in 128 rows, cpad 32 > C, k1 = 288
    ('window', 11, 11, 32),
    ('map', 1, 7, 8),
    ('map', 4, 6, 8),
    ('map', 12, 10, 24),
    ('map', 20, 20, 8),         # p16 = 416
)
ACTIONS = (3, 4)
CASES = tuple(g + (a,) for g in GEOMETRIES for a in ACTIONS)
IDS = ['%s-%dx%dx%d-A%d' % c for c in CASES]

BF16 = ('conv1_w', 'conv2_w', 'conv3_w', 'fc1_w', 'fc2_w')
FP32 = ('conv1_b', 'conv2_b', 'conv3_b', 'fc1_b', 'fc2_b', 'fc3_w', 'fc3_b')

_TIE_EVEN = 1.0 + 2.0 ** -8             # between 1 and 1 + 2^-7, kept bit 0: rounds down
_TIE_ODD = 1.0 + 3 * 2.0 ** -8          # between 1 + 2^-7 and 1 + 2^-6, kept bit 1: rounds up
_F = np.float32
CRAFTED = np.array([
    0.0, -0.0, _TIE_EVEN, _TIE_ODD,
    np.nextafter(_F(_TIE_EVEN), _F(0)), np.nextafter(_F(_TIE_EVEN), _F(2)),
    1e-40, np.finfo(np.float32).tiny, np.inf, -np.inf, np.finfo(np.float32).max,
    -np.finfo(np.float32).max, -_TIE_EVEN, -_TIE_ODD, -1e-40, np.nextafter(_F(_TIE_ODD), _F(0)),
], dtype=np.float32)
assert CRAFTED.size == 16 and not np.isnan(CRAFTED).any()


def shapes(h, w, c, A):
    return {'conv1.weight': (32, c, 3, 3), 'conv1.bias': (32,), 'conv2.weight': (64, 32, 3, 3), 'conv2.bias': (64,),
            'conv3.weight': (64, 64, 3, 3), 'conv3.bias': (64,), 'fc1.weight': (256, 64 * h * w), 'fc1.bias': (256,),
            'fc2.weight': (128, 256), 'fc2.bias': (128,), 'fc3.weight': (A, 128), 'fc3.bias': (A,)}


def real_state(h, w, c, A, seed=0, crafted=True):
    """A state dict of the reference's names: normal draws scaled by
    1/sqrt(fan_in) of the layer, the crafted values first."""
    torch.manual_seed(1000 * seed + 97 * h + 13 * w + c + A)
    sh = shapes(h, w, c, A)
    state = {}
    for name, shape in sh.items():
        wshape = sh[name.split('.')[0] + '.weight']
        fan_in = int(np.prod(wshape[1:]))
        t = torch.randn(shape) / fan_in ** 0.5
        if crafted:
            n = min(16, t.numel())
            t.view(-1)[:n] = torch.from_numpy(CRAFTED[:n].copy())
        state[name] = t
    return state


def bits(t):
    """A tensor's bit pattern: bf16 words stay int16, float32 is viewed as int32."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def truth(state, plan, h, w, c, A):
    """The bits of the torch packing (tests/dqn_pack_ref.py), run on the CPU."""
    import dqn_pack_ref
    return {k: bits(v) for k, v in dqn_pack_ref.torch_pack(state, plan, h, w, c, A).items()}


@functools.lru_cache(maxsize=None)
def case(plan, h, w, c, A):
    """(state, ground truth), shared between the tests of a session; nobody
    writes to its tensors."""
    state = real_state(h, w, c, A)
    return state, truth(state, plan, h, w, c, A)


def kernel_net(state, h, w, device='cpu'):
    """The state dict in the fp32 kernels' layouts: (tensors that own the
    memory, the Dqn32Net of their addresses)."""
    from marlenv._native import Dqn32Net
    from marlenv.learner import FIELDS, NAMES, to_kernel
    keep = [to_kernel(n, state[n].to(device=device, dtype=torch.float32), h * w).contiguous() for n in NAMES]
    assert len(FIELDS) == len(keep)
    return keep, Dqn32Net(*(t.data_ptr() for t in keep))


def fill_ff(fwd):
    """Every byte of a forward's weight buffers becomes 0xFF, so an element the
    pack leaves unwritten shows (0xFFFF is a bf16 NaN, 0xFFFFFFFF an fp32 NaN)."""
    for t in fwd.tensors.values():
        t.view(torch.uint8).fill_(255)


def packed_bits(fwd):
    return {k: bits(v) for k, v in fwd.tensors.items()}


def assert_equal_bits(got, want, what=''):
    assert set(got) == set(want)
    for k in BF16 + FP32:
        assert got[k].numel() == want[k].numel(), (what, k)
        same = torch.equal(got[k].view(-1), want[k].view(-1))
        if not same:
            bad = (got[k].view(-1) != want[k].view(-1)).nonzero().view(-1)
            i = int(bad[0])
            raise AssertionError('%s %s: %d of %d elements differ, first at %d: got %#x, want %#x' % (
                what, k, bad.numel(), got[k].numel(), i, int(got[k].view(-1)[i]) & 0xffffffff,
                int(want[k].view(-1)[i]) & 0xffffffff))


def cfg_of(h, w, c, A, waves=0):
    from marlenv._native import DqnCfg
    return DqnCfg(h, w, c, A, waves)


def null_call(native, fn, cfg, map_plan):
    """rc and message of a pack call whose cfg is checked before any pointer."""
    from marlenv._native import Dqn32Net, DqnNet
    L = native.lib()
    args = [ctypes.byref(cfg), map_plan, ctypes.byref(Dqn32Net()), ctypes.byref(DqnNet()), None]
    if fn == 'snake_dqn_pack32':
        args.append(None)
    return getattr(L, fn)(*args), L.snake_last_error().decode()
