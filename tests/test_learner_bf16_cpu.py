"""CPU checks of the bf16 backward's tests (no GPU needed): what
tests/test_learner_bf16_gpu.py's comparisons rest on.

Existing probes: bf16 holds every staged GEMM operand exactly, so the model of
tests/learner_model.py equals the autograd reference. Rounding cases (dq x 29):
all integers, every sum of absolute terms below 2^24, rounding does change
operands and results. Real-valued case: no unit sits close enough to its ReLU
threshold for the fp32 forward to mask it differently. And the new entry point
is exported and validates its arguments like the fp32 one, before any launch."""
import ctypes

import pytest
import torch

import dqn_probe as P
import learner16_cases as L16
import learner_cases as LC
import learner_model as M
from learner_gpu_util import key_ids, native, run_ids  # noqa: F401 (native is a fixture)

ALL_RUNS = LC.gpu_backward_runs()
RUN_IDS, KEY_IDS = run_ids(ALL_RUNS), key_ids(L16.ROUNDING_KEYS)


@pytest.mark.parametrize('key,B', ALL_RUNS, ids=RUN_IDS)
def test_existing_probes_stage_only_bf16_values(key, B):
    case = LC.backward_case(key, B)
    grads, staged, bound = M.backward_model(case.state, case.obs, case.dq)
    assert set(staged) == {'x', 'c1', 'c2', 'c3', 'h1', 'w:conv2', 'w:conv3', 'w:fc1', 'w:fc2',
                           'dY1', 'dY2', 'dY3', 'dY4', 'dY5'}
    top = {n: float(v.abs().max()) for n, v in staged.items()}
    print(top)
    for name, v in staged.items():
        assert torch.equal(v, v.round()) and top[name] < 256, name      # integers below 2^8: exact in bf16
        assert torch.equal(M.bf16(v), v), name
    for name in LC.PARAMS:
        assert torch.equal(grads[name], case.grads[name]), name
    assert bound < LC.SUM_LIMIT


def test_the_unrounded_model_is_the_autograd_reference():
    """backward_model with no rounding is ref_grads, also where rounding matters."""
    for key in L16.ROUNDING_KEYS[:2]:
        case, dq, _ = L16.rounding_case(key)
        grads = M.backward_model(case.state, case.obs, dq, M.exact)[0]
        ref = LC.ref_grads(case.state, case.obs, dq)
        for name in LC.PARAMS:
            assert torch.equal(grads[name], ref[name]), (key, name)


@pytest.mark.parametrize('key', L16.ROUNDING_KEYS, ids=KEY_IDS)
def test_rounding_cases_are_exact_and_do_round(key):
    case, dq, model = L16.rounding_case(key)
    grads, staged, bound = M.backward_model(case.state, case.obs, dq)
    for name in LC.PARAMS:
        assert torch.equal(grads[name], model[name])
        assert torch.equal(model[name], model[name].round()), name
    for name, v in staged.items():
        assert torch.equal(v, v.round()), name
    # the chain's own sums, on the operands as it stages them
    print('max sum |terms| %.4g of 2^24 = %.4g' % (bound, LC.SUM_LIMIT))
    assert bound < LC.SUM_LIMIT
    assert max(float(g.abs().max()) for g in model.values()) <= bound
    # rounding changes the dY buffers: of the float64 reference's chain (29 x the probe's) ...
    _, exact_staged, _ = M.backward_model(case.state, case.obs, dq, M.exact)
    changed = {i: int((M.bf16(exact_staged['dY%d' % i]) != exact_staged['dY%d' % i]).sum()) for i in range(1, 6)}
    # ... and of the model's chain. There dY3 is an exception by construction: the
    # probe's fc1 has one +-1 weight per column, so every dY3 entry is a copy of a
    # ROUNDED dY4 entry and is a bf16 value already.
    own = {i: int((M.bf16(staged['dY%d' % i]) != staged['dY%d' % i]).sum()) for i in range(1, 6)}
    print('unrepresentable entries: reference chain %s, model chain %s' % (changed, own))
    for i in L16.ROUNDED_DY[key]:
        assert changed[i] > 0, i
        assert own[i] > 0 or i == 3, i
    if key == (5, 5, 8, 3, 0, 70):
        assert [changed[i] for i in range(1, 6)] == [10527, 5760, 1199, 329, 5]
    if key == (5, 5, 24, 5, 0, 70):
        assert [changed[i] for i in range(1, 6)] == [10744, 8549, 2181, 660, 69]
    # weights stay below 2^8: only dY is rounded here
    for name in ('x', 'c1', 'c2', 'c3', 'h1', 'w:conv2', 'w:conv3', 'w:fc1', 'w:fc2'):
        assert torch.equal(M.bf16(staged[name]), staged[name]), name
    # and the result is not 29 x the unrounded one
    for name in ('conv1.weight', 'conv2.weight', 'conv3.weight', 'fc1.weight'):
        assert not torch.equal(model[name], L16.ROUNDING_SCALE * case.grads[name]), name
    # what the header leaves unrounded
    for name in ('fc3.weight', 'fc3.bias', 'fc2.bias'):
        assert torch.equal(model[name], L16.ROUNDING_SCALE * case.grads[name]), name


def test_the_29x_bound_of_the_4x33_case_is_too_large():
    """Why (4, 33, 8, 3, 0, 65) is no rounding case."""
    case = LC.backward_case((4, 33, 8, 3, 0, 65))
    assert LC.term_bound(case.state, case.obs, case.dq) * L16.ROUNDING_SCALE > LC.SUM_LIMIT


@pytest.mark.parametrize('scaled', [False, True], ids=['bytes-0-1', 'bytes-0-255'])
def test_real_case_masks_are_stable(scaled):
    state, obs, dq = L16.real_case(scaled=scaled)
    assert tuple(obs.shape) == (6, 3, 4, 8) and tuple(dq.shape) == (6, 3)
    assert int(obs.max()) == (255 if scaled else 1)
    margin = M.margin(state, obs, M.exact)
    print('min |Y + b| / max |Y + b| = %.3g' % margin)
    assert margin >= L16.MASK_MARGIN
    model, ref = L16.ref_grads_bf16(state, obs, dq), LC.ref_grads(state, obs, dq)
    exact = M.backward_model(state, obs, dq, M.exact)[0]
    for name in LC.PARAMS:
        assert model[name].shape == ref[name].shape
        scale = float(ref[name].abs().max())
        assert float((exact[name] - ref[name]).abs().max()) <= 1e-12 * scale, name
        if name in ('fc3.weight', 'fc3.bias', 'fc2.bias'):                # nothing rounded on their path
            assert torch.equal(model[name], exact[name]), name
        else:
            assert not torch.equal(model[name], exact[name]), name
        rel = float((model[name] - ref[name]).norm() / ref[name].norm())
        print('%-13s |model - g64| / |g64| = %.3g' % (name, rel))
        assert rel < 2e-2, name                                       # a few bf16 roundings (2^-9 each)


def test_real_seed_is_the_first_stable_one():
    assert L16.first_stable_seed(M.exact) == L16.REAL_SEED


# ---- exports and validation ------------------------------------------------------
def test_exports(native):
    L = native.lib()
    assert 'snake_dqn32_backward_bf16' in native.EXPORTS and hasattr(L, 'snake_dqn32_backward_bf16')
    assert native.SNAKE_ABI_VERSION == 20 and L.snake_abi_version() == 20
    assert L.snake_dqn32_backward_bf16.argtypes == L.snake_dqn32_backward.argtypes


def call(native, fn, cfg=(5, 5, 8, 3), batch=1, net=0x1000, grad=0x2000, obs=0x100, fwd=0x3000, dq=0x100,
         ts=0x4000, bad_w=None, bad_g=None):
    """Both functions validate before any launch, so host-only calls with
    made-up addresses reach every check (none is dereferenced)."""
    L = native.lib()
    c = native.DqnCfg(*cfg, 0)
    wts = [net + 64 * i for i in range(12)]
    gds = [grad + 64 * i for i in range(12)]
    if bad_w is not None:
        wts[3] = bad_w
    if bad_g is not None:
        gds[7] = bad_g
    n, g = native.Dqn32Net(*wts), native.Dqn32Net(*gds)
    p = ctypes.c_void_p
    rc = getattr(L, fn)(ctypes.byref(c), ctypes.byref(n) if net else None, p(obs), batch, p(fwd), p(dq), p(ts),
                        ctypes.byref(g) if grad else None, None)
    return rc, L.snake_last_error().decode()


BAD_ARGS = [
    (dict(obs=0), 'NULL buffer'), (dict(fwd=0), 'NULL buffer'), (dict(dq=0), 'NULL buffer'),
    (dict(ts=0), 'NULL buffer'), (dict(net=0), 'NULL buffer'), (dict(grad=0), 'NULL buffer'),
    (dict(bad_w=0), 'NULL weight'), (dict(bad_g=0), 'NULL weight'),
    (dict(bad_w=0x1004), '16-byte'), (dict(bad_g=0x2008), '16-byte'),
    (dict(fwd=0x3004), 'scratch'), (dict(ts=0x4008), 'scratch'),
    (dict(cfg=(5, 5, 12, 3)), 'channels'), (dict(cfg=(0, 5, 8, 3)), 'observation'),
    (dict(cfg=(5, 5, 8, 65)), 'num_actions'), (dict(batch=-1), 'batch'),
    (dict(cfg=(255, 255, 8, 3), batch=1 << 20), 'batch'),
]


@pytest.mark.parametrize('kw,msg', BAD_ARGS, ids=[m + '-' + '-'.join(k) for k, m in BAD_ARGS])
def test_bf16_backward_rejects_what_the_fp32_one_rejects(native, kw, msg):
    rc32, err32 = call(native, 'snake_dqn32_backward', **kw)
    rc16, err16 = call(native, 'snake_dqn32_backward_bf16', **kw)
    assert rc32 < 0 and rc16 == rc32
    assert msg in err16 and msg in err32
    assert err16.replace('snake_dqn32_backward_bf16', 'snake_dqn32_backward') == err32


def test_bf16_backward_of_an_empty_batch_launches_nothing(native):
    assert call(native, 'snake_dqn32_backward_bf16', batch=0)[0] == 0
    assert call(native, 'snake_dqn32_backward', batch=0)[0] == 0


def test_learner_rejects_a_precision_before_any_device_work(native):
    from marlenv import DQNLearner
    state = P.probe_net(5, 5, 8, 3, 0)
    for bad in ('fp16', 'BF16', None, 16):
        with pytest.raises(ValueError, match='backward_precision'):
            DQNLearner(state, 5, 5, 8, 3, backward_precision=bad)
    if not torch.cuda.is_available():
        for ok in ('fp32', 'bf16'):
            with pytest.raises(RuntimeError, match='HIP device'):       # accepted: the next check is the device
                DQNLearner(state, 5, 5, 8, 3, backward_precision=ok)
