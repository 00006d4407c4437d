"""The DQN entry points on buffers of exactly the planned size, inside a
guard-band arena (tests/guard_util.py): every scratch at the byte count its plan
function returns for that batch, every output at its exact size, 0x5A-filled.

  snake_dqn32_forward / _forward_bf16     snake_dqn32_scratch / _forward_bf16_scratch
  snake_dqn32_backward / _backward_bf16   snake_dqn32_train_scratch; the gradient net's flat
                                          buffer with 0x5A in the pad floats between its tensors
  snake_dqn_td_loss, snake_adam_step      SNAKE_ADAM_SCRATCH_BYTES
  snake_dqn_pack32                        the twelve destinations at the plan layout's sizes
  snake_dqn_forward / _map_forward        2 * B * act_per_obs bytes

After the guards pass the results are compared as the exact tests compare them
(integer probes: torch.equal with float64; TD loss and Adam: the derived
bounds of tests/learner_cases.py; the pack: the torch packing, bit for bit), so
an output byte nothing wrote shows as 0x5A. The probes' preconditions are
proven on the CPU (tests/test_dqn_probe_cpu.py, test_dqn_map_cpu.py,
test_learner_cpu.py, test_learner_fwd16_cpu.py).

A read outside a buffer is invisible to this method."""
import ctypes

import numpy as np
import pytest
import torch

import dqn_pack_cases as PC
import dqn_probe as P
import learner_cases as LC
import learner_fwd16_cases as FC
from guard_util import FILL_BYTE, Arena, untouched

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
VP = ctypes.c_void_p


@pytest.fixture(scope='module', autouse=True)
def native():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    from marlenv import _native
    _native.lib()
    return _native


def key_id(k):
    return '%dx%dx%d-A%d-s%d-B%d' % tuple(k)


def same(got, want, what):
    got = got.double().cpu()
    assert got.shape == want.shape, what
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError('%s: %d of %d differ, first at %s: got %r, want %r' % (
            what, bad.size(0), want.numel(), i, float(got[i]), float(want[i])))


# ---- the fp32 layout's forwards and backwards ----------------------------------------
FORWARDS = {'fp32': ('snake_dqn32_forward', 'snake_dqn32_scratch'),
            'bf16': ('snake_dqn32_forward_bf16', 'snake_dqn32_forward_bf16_scratch')}
BACKWARDS = {'fp32': 'snake_dqn32_backward', 'bf16': 'snake_dqn32_backward_bf16'}


def planned(L, fn, cfg, B):
    n = int(getattr(L, fn)(ctypes.byref(cfg), B))
    assert n > 0, L.snake_last_error().decode()
    return n


class Forward32:
    """One forward of a probe's first B rows: scratch, q and (optionally) feat
    taken at their exact sizes; guards checked, results compared."""

    def __init__(self, native, mode, key, B, with_feat):
        from marlenv.dqn_weights import Net32
        h, w, c, A = key[:4]
        self.L = L = native.lib()
        fn, scratch_fn = FORWARDS[mode]
        p = P.probe(*key)
        self.cfg = cfg = native.DqnCfg(h, w, c, A, 0)
        self.net = Net32(h * w, c, A, DEV).load(p.state)
        self.obs = p.obs[:B].contiguous().to(DEV)
        need = planned(L, scratch_fn, cfg, B)
        sizes = dict(scratch=need, q=4 * B * A)
        if with_feat:
            sizes['feat'] = 4 * B * 128
        self.arena = ar = Arena(sizes.values())
        ar.take('scratch', need)
        q = ar.take('q', sizes['q'], torch.float32, (B, A))
        feat = ar.take('feat', sizes['feat'], torch.float32, (B, 128)) if with_feat else None
        what = '%s forward %s B=%d feat=%s' % (mode, key_id(key), B, with_feat)
        native.check(getattr(L, fn)(ctypes.byref(cfg), ctypes.byref(self.net.struct), VP(self.obs.data_ptr()), B,
                                    ar.ptr('scratch'), ar.ptr('q'), ar.ptr('feat') if with_feat else None, None), L)
        ar.check(what)
        same(q, p.q[:B], what + ' q')
        if with_feat:
            same(feat, p.feat[:B], what + ' features')


# (h, w, c, A, seed, probe B) and the batch prefixes run
FWD_KEYS = [((4, 33, 8, 3, 0, 65), 65), ((2, 34, 8, 3, 0, 65), 65), ((5, 5, 8, 3, 1, 129), 1),
            ((5, 5, 8, 3, 1, 129), 127), ((5, 5, 8, 3, 1, 129), 129), ((5, 5, 8, 5, 0, 70), 70),
            ((1, 1, 8, 3, 0, 70), 70), ((5, 5, 64, 3, 0, 70), 70)]
# fc1's split K at the full map; a chunk above the 1 024 floor with a ragged
# end (16 chunks, the last of 256 steps); three chunks, the last of 64 steps
FWD16_KEYS = FWD_KEYS + [((20, 20, 8, 3, 0, 5), 5)] + [(k, k[5]) for k in FC.SPLIT_K_KEYS]


def run_id(r):
    return key_id(r[0][:5] + (r[1],))


@pytest.mark.parametrize('with_feat', [False, True], ids=['q-only', 'with-feat'])
@pytest.mark.parametrize('run', FWD_KEYS, ids=run_id)
def test_fp32_forward(native, run, with_feat):
    Forward32(native, 'fp32', run[0], run[1], with_feat)


@pytest.mark.parametrize('with_feat', [False, True], ids=['q-only', 'with-feat'])
@pytest.mark.parametrize('run', FWD16_KEYS, ids=run_id)
def test_bf16_forward(native, run, with_feat):
    assert FC.fc1_chunks((17, 17, 8, 3, 0, 5)) == (16, 256) and FC.fc1_chunks((3, 11, 8, 3, 0, 37)) == (3, 64)
    Forward32(native, 'bf16', run[0], run[1], with_feat)


BWD_KEYS = [((5, 5, 8, 3, 1, 129), 1), ((5, 5, 8, 3, 1, 129), 127), ((5, 5, 8, 3, 1, 129), 129),
            ((4, 33, 8, 3, 0, 65), 65),         # five split-M chunks, the last one ragged
            ((5, 5, 24, 5, 0, 70), 70),         # fc3_b of 5 floats, 11 pad floats behind it
            ((2, 34, 8, 3, 0, 65), 65), ((20, 20, 8, 3, 0, 5), 5), ((17, 17, 8, 3, 0, 5), 5)]


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
@pytest.mark.parametrize('run', BWD_KEYS, ids=run_id)
def test_backward(native, run, mode):
    """After the forward of the same precision; every tensor of the gradient net
    equals the autograd reference and every pad float keeps its 0x5A bytes."""
    from marlenv.dqn_weights import Net32
    key, B = run
    h, w, c, A = key[:4]
    case = LC.backward_case(key, B)
    fwd = Forward32(native, mode, key, B, False)
    L = fwd.L
    need = planned(L, 'snake_dqn32_train_scratch', fwd.cfg, B)
    numel = Net32.size(h * w, c, A)
    ar = Arena([need, 4 * numel, 4 * B * A])
    ar.take('train_scratch', need)
    flat = ar.take('grad', 4 * numel, torch.float32)
    dq = ar.take('dq', 4 * B * A, torch.float32, (B, A))
    dq.copy_(case.dq)
    gnet = Net32(h * w, c, A, flat=flat)
    pad = torch.ones(numel, dtype=torch.bool)
    for off, size, _ in Net32.spans(h * w, c, A)[0]:
        pad[off:off + size] = False
    assert int(pad.sum()) == 16 - A               # behind fc3_b, the only tensor that is no multiple of 16 floats
    fwd_scratch = fwd.arena.payload('scratch').clone()
    what = '%s backward %s B=%d' % (mode, key_id(key), B)
    native.check(getattr(L, BACKWARDS[mode])(
        ctypes.byref(fwd.cfg), ctypes.byref(fwd.net.struct), VP(fwd.obs.data_ptr()), B, fwd.arena.ptr('scratch'),
        ar.ptr('dq'), ar.ptr('train_scratch'), ctypes.byref(gnet.struct), None), L)
    ar.check(what)
    fwd.arena.check(what + ' (the forward\'s buffers)')
    assert torch.equal(fwd.arena.payload('scratch'), fwd_scratch), 'fwd_scratch is read only'
    assert torch.equal(dq.cpu(), case.dq), 'dq is read only'
    pads = flat.cpu().view(torch.uint8).view(numel, 4)[pad]
    changed = (pads != FILL_BYTE).any(1)
    assert not bool(changed.any()), '%s: %d pad floats of the gradient buffer were written, the first at float %d' % (
        what, int(changed.sum()), int(pad.nonzero().view(-1)[changed.nonzero().view(-1)[0]]))
    got = gnet.unpack()
    wrong = [n for n in LC.PARAMS if not torch.equal(got[n].double().cpu(), case.grads[n])]
    assert not wrong, '%s: %s differ from the float64 reference' % (what, wrong)


# ---- TD loss -----------------------------------------------------------------------------------
def td_inputs(B, A):
    g = P._gen(B, A, 9001)
    return (torch.randn((B, A), generator=g) * 2, torch.randint(0, A, (B,), generator=g),
            torch.randn(B, generator=g), (torch.rand(B, generator=g) < 0.3).float(), torch.randn((B, A), generator=g) * 2)


@pytest.mark.parametrize('B,A', [(1, 3), (70, 3), (257, 5), (513, 1)])
def test_td_loss(native, B, A):
    L = native.lib()
    inputs = td_inputs(B, A)
    gamma = 0.99
    loss64, dq64, _ = LC.td_ref64(*inputs, gamma)
    loss_bound, dq_bound = LC.td_bounds(*inputs, gamma)
    q, action, reward, done, next_q = (t.contiguous().to(DEV) for t in inputs)
    ar = Arena([4 * B * A, 4, 4])
    dq = ar.take('dq', 4 * B * A, torch.float32, (B, A))
    loss = ar.take('loss', 4, torch.float32)
    err = ar.take('err', 4, torch.int32, fill='zero')          # (the caller zeroes it)
    native.check(L.snake_dqn_td_loss(VP(q.data_ptr()), VP(action.data_ptr()), VP(reward.data_ptr()),
                                     VP(done.data_ptr()), VP(next_q.data_ptr()), B, A, gamma, ar.ptr('loss'),
                                     ar.ptr('dq'), ar.ptr('err'), None), L)
    ar.check('td_loss B=%d A=%d' % (B, A))
    assert not bool(untouched(dq).view(B * A, 4).all(1).any()), 'a dq element was not written'
    err_dq = (dq.cpu().double() - dq64).abs()
    print('loss err %.3g (bound %.3g), dq err %.3g (bound %.3g)' % (
        abs(float(loss) - float(loss64)), loss_bound, float(err_dq.max()), float(dq_bound.max())))
    assert bool((err_dq <= dq_bound).all())
    assert abs(float(loss) - float(loss64)) <= loss_bound
    assert int(err.item()) == 0


# ---- clip + Adam -------------------------------------------------------------------------------
HYPER = dict(lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=10.0)


@pytest.mark.parametrize('n', [1, 5, 4099, 5003])
def test_adam_step(native, n):
    """param, m, v and the (read-only) gradient at exactly 4 n bytes, the scratch
    at SNAKE_ADAM_SCRATCH_BYTES, the norm at 4; against float64 within the bound
    tests/learner_cases.py derives (as tests/test_learner_gpu.py)."""
    L = native.lib()
    step = 2
    g = P._gen(n, 9002)
    grad, p = torch.randn(n, generator=g), torch.randn(n, generator=g)
    m, v = torch.randn(n, generator=g), torch.randn(n, generator=g) ** 2
    p64, m64, v64, norm64, S = LC.adam_ref64(p, grad, m, v, step, **HYPER)
    assert native.ADAM_SCRATCH_BYTES == 4112
    ar = Arena([4 * n] * 4 + [native.ADAM_SCRATCH_BYTES, 4])
    dev = {}
    for name, t in (('param', p), ('grad', grad), ('m', m), ('v', v)):
        dev[name] = ar.take(name, 4 * n, torch.float32)
        dev[name].copy_(t)
    ar.take('scratch', native.ADAM_SCRATCH_BYTES)
    norm = ar.take('norm', 4, torch.float32)
    native.check(L.snake_adam_step(ar.ptr('param'), ar.ptr('grad'), ar.ptr('m'), ar.ptr('v'), n, step, HYPER['lr'],
                                   HYPER['beta1'], HYPER['beta2'], HYPER['eps'], HYPER['max_norm'],
                                   ar.ptr('scratch'), ar.ptr('norm'), None), L)
    ar.check('adam n=%d' % n)
    assert torch.equal(dev['grad'].cpu(), grad), 'the gradient is not written'
    e_n, K = LC.adam_bounds(n)
    got = dev['param'].cpu()
    half_ulp = torch.from_numpy(np.spacing(np.maximum(got.abs().numpy(), p64.abs().float().numpy()))).double() / 2
    err = (got.double() - p64).abs()
    bound = half_ulp + K * LC.U * S
    print('norm rel err %.3g (bound %.3g); worst p err / bound %.3f' % (
        abs(float(norm) - norm64) / norm64, e_n + LC.U, float((err / bound.clamp(min=1e-300)).max())))
    assert abs(float(norm) - norm64) <= (e_n + LC.U) * norm64
    assert bool((err <= bound).all())
    e_g = e_n + 3 * LC.U
    b1 = float(np.float32(HYPER['beta1']))
    coef = min(1.0, 10.0 / (norm64 + 1e-6))
    am = (b1 * m.double()).abs() + ((1 - b1) * coef * grad.double()).abs()
    assert bool(((dev['m'].cpu().double() - m64).abs() <= (e_g + 3 * LC.U) * LC.SLACK * am).all())
    assert bool(((dev['v'].cpu().double() - v64).abs() <= (2 * e_g + 4 * LC.U) * LC.SLACK * v64).all())


# ---- the pack and the bf16 forwards --------------------------------------------------------------
def guarded_forward(plan, h, w, c, A):
    """A DQNForward.empty whose twelve weight buffers are arena payloads of the
    plan layout's sizes (0x5A-filled); returns (forward, arena)."""
    from marlenv.dqn import NET_FIELDS, DQNForward
    fwd = DQNForward.empty(h, w, c, num_actions=A, device=DEV, plan=plan)
    assert fwd.plan == plan
    lay = fwd.layout
    elems = {k: int(getattr(lay, k)) for k in PC.BF16}
    elems.update(conv1_b=32, conv2_b=64, conv3_b=64, fc1_b=256, fc2_b=128, fc3_w=A * 128, fc3_b=A)
    nbytes = {k: n * (2 if k in PC.BF16 else 4) for k, n in elems.items()}
    ar = Arena(nbytes.values())
    for k in NET_FIELDS:
        t = ar.take(k, nbytes[k], torch.int16 if k in PC.BF16 else torch.float32)
        assert t.numel() == fwd.tensors[k].numel() and t.dtype == fwd.tensors[k].dtype, k
        fwd.tensors[k] = t.view(fwd.tensors[k].shape)
    fwd.net = type(fwd.net)(*(fwd.tensors[k].data_ptr() for k in NET_FIELDS))
    return fwd, ar


PACK_CASES = [('window', 3, 3, 8, 3), ('window', 11, 11, 24, 4), ('map', 1, 7, 8, 3), ('map', 12, 10, 8, 3),
              ('map', 20, 20, 8, 3)]


@pytest.mark.parametrize('plan,h,w,c,A', PACK_CASES, ids=['%s-%dx%dx%d-A%d' % c for c in PACK_CASES])
def test_pack32(plan, h, w, c, A):
    """Every element of every destination is written on every call: none keeps
    its prefill, all equal the torch packing."""
    state, want = PC.case(plan, h, w, c, A)
    fwd, ar = guarded_forward(plan, h, w, c, A)
    keep, net32 = PC.kernel_net(state, h, w, DEV)
    for call in ('first call', 'second call'):
        fwd.pack32(net32)
        ar.check('pack32 %s %dx%dx%d %s' % (plan, h, w, c, call))
        PC.assert_equal_bits(PC.packed_bits(fwd), want, call)


BF16_FWD = [('window', (11, 11, 8, 3, 0, 513)), ('map', (20, 20, 8, 3, 0, 257))]


@pytest.mark.parametrize('B', [1, 33, 257])
@pytest.mark.parametrize('plan,key', BF16_FWD, ids=['window-11x11x8', 'map-20x20x8'])
def test_bf16_plan_forwards(native, plan, key, B):
    """snake_dqn_forward / snake_dqn_map_forward with act_scratch of exactly
    2 * B * act_per_obs bytes, feat_out NULL and given."""
    from marlenv.dqn import DQNForward
    h, w, c, A = key[:4]
    p = P.probe(*key)
    net = DQNForward({k: v.to(DEV) for k, v in p.state.items()}, h, w, c, A, device=DEV, plan=plan)
    assert net.plan == plan
    obs = p.obs[:B].contiguous().to(DEV)
    need = 2 * B * int(net.layout.act_per_obs)
    for with_feat in (False, True):
        ar = Arena([need, 4 * B * A, 4 * B * 128])
        ar.take('act_scratch', need)
        q = ar.take('q', 4 * B * A, torch.float32, (B, A))
        feat = ar.take('feat', 4 * B * 128, torch.float32, (B, 128))
        what = '%s forward B=%d feat=%s' % (plan, B, with_feat)
        native.check(net._forward_fn(ctypes.byref(net.cfg), ctypes.byref(net.net), VP(obs.data_ptr()), B,
                                     ar.ptr('act_scratch'), ar.ptr('q'), ar.ptr('feat') if with_feat else None, None),
                     net._L)
        ar.check(what)
        same(q, p.q[:B], what + ' q')
        if with_feat:
            same(feat, p.feat[:B], what + ' features')
        else:
            assert bool(untouched(feat).all()), 'feat written though feat_out is NULL'
