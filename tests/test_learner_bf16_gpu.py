"""GPU checks of the bf16 backward (DQNLearner(backward_precision='bf16');
dqn_train16_kernels.hip, snake_dqn32_backward_bf16).

On the integer probes of tests/learner_cases.py bf16 holds every staged operand
exactly, so the result must EQUAL the float64 autograd reference, as the fp32
backward's does. On the rounding cases (dq x 29) it must EQUAL the float64 model
of tests/learner_model.py, which rounds exactly where include/snake_env.h says
the kernel rounds (tests/test_learner_bf16_cpu.py proves both preconditions).
On real values it stays within a tolerance the model sets. update() in bf16 mode
is bit-equal to its stages, reproducible, and checkpoints move between modes."""
import pytest
import torch

import dqn_probe as P
import learner16_cases as L16
import learner_cases as LC
from learner_gpu_util import (DEV, check_checkpoints_move, check_update_equals_its_stages, key_ids, make_learner,
                              run_ids)

pytestmark = pytest.mark.gpu


def run_backward(state, key, obs, dq, precision='bf16'):
    learner = make_learner(state, key, backward_precision=precision)
    assert learner.backward_precision == precision
    obs = obs.to(DEV)
    q = learner(obs)
    learner.backward(obs, dq.to(DEV))
    return q.cpu(), {k: v.cpu() for k, v in learner.grads().items()}


def mismatches(got, ref):
    wrong = {}
    for name in LC.PARAMS:
        assert got[name].shape == ref[name].shape and got[name].dtype == torch.float32
        if not torch.equal(got[name].double(), ref[name]):
            diff = (got[name].double() - ref[name]).abs()
            wrong[name] = (int((diff != 0).sum()), float(diff.max()))
    return wrong


def localise(key, B, scale=1.0):
    """Which single layer's backward is wrong: every other layer identity-like."""
    h, w, c, A, seed, _ = key
    bad = []
    for layer in P.LAYERS:
        state = P.probe_net(h, w, c, A, seed, identity=tuple(n for n in P.LAYERS if n != layer))
        obs = P.probe_obs(key[5], h, w, c, seed)[:B].contiguous()
        dq = (LC.probe_dq(key)[:B] * scale).contiguous()
        ref = L16.ref_grads_bf16(state, obs, dq)
        _, got = run_backward(state, key, obs, dq)
        wrong = [n for n in LC.PARAMS if not torch.equal(got[n].double(), ref[n])]
        if wrong:
            bad.append('%s alone: %s' % (layer, wrong))
    return '; '.join(bad) or 'no single layer reproduces it'


RUNS = LC.gpu_backward_runs()


@pytest.mark.parametrize('key,B', RUNS, ids=run_ids(RUNS))
def test_bf16_backward_equals_float64_reference(key, B):
    case = LC.backward_case(key, B)
    q, got = run_backward(case.state, key, case.obs, case.dq)
    assert torch.equal(q.double(), P.probe(*key).q[:B])
    wrong = mismatches(got, case.grads)
    assert not wrong, '%s; %s' % (wrong, localise(key, B))


@pytest.mark.parametrize('key', L16.ROUNDING_KEYS, ids=key_ids(L16.ROUNDING_KEYS))
def test_bf16_backward_equals_the_rounding_model(key):
    case, dq, model = L16.rounding_case(key)
    _, got = run_backward(case.state, key, case.obs, dq)
    wrong = mismatches(got, model)
    assert not wrong, '%s; %s' % (wrong, localise(key, key[5], L16.ROUNDING_SCALE))
    # the fp32 backward on the same inputs is 29 x the probe's gradients: the bf16 kernels did run
    _, got32 = run_backward(case.state, key, case.obs, dq, 'fp32')
    for name in LC.PARAMS:
        assert torch.equal(got32[name].double(), L16.ROUNDING_SCALE * case.grads[name]), name
    for name in ('conv1.weight', 'conv2.weight', 'conv3.weight', 'fc1.weight'):
        assert not torch.equal(got[name], got32[name]), name
    for name in ('fc3.weight', 'fc3.bias', 'fc2.bias'):
        assert torch.equal(got[name], got32[name]), name


@pytest.mark.parametrize('scaled', [False, True], ids=['bytes-0-1', 'bytes-0-255'])
def test_bf16_backward_real_values_within_the_model_tolerance(scaled):
    """Per parameter tensor |got - g64| <= 1.5 |model - g64| + 1e-5 |g64| (2-norms):
    g64 the float64 autograd reference, model the float64 bf16 model. The kernel
    differs from the model only by fp32 accumulation order (2^-24 per addition
    against 2^-9 per rounded operand) and by rare ties at a rounding boundary,
    hence 1.5; 1e-5 is the fp32 backward's own tolerance, for the tensors the
    model does not round at all (fc3). The masks are the model's: the CPU file
    asserts every unit is 2e-5 of its layer's scale away from its threshold."""
    state, obs, dq = L16.real_case(scaled=scaled)
    g64, model = LC.ref_grads(state, obs, dq), L16.ref_grads_bf16(state, obs, dq)
    key = L16.REAL_GEOM
    _, got = run_backward(state, key, obs, dq)
    _, got32 = run_backward(state, key, obs, dq, 'fp32')
    failed = []
    for name in LC.PARAMS:
        err = float((got[name].double() - g64[name]).norm())
        model_err = float((model[name] - g64[name]).norm())
        ref_norm = float(g64[name].norm())
        err32 = float((got32[name].double() - g64[name]).norm())
        print('%-13s |got - g64| %.4g  |model - g64| %.4g  |g64| %.4g  (fp32 mode: %.4g)' % (
            name, err, model_err, ref_norm, err32))
        if not err <= 1.5 * model_err + 1e-5 * ref_norm:
            failed.append(name)
    assert not failed
    assert not torch.equal(got['conv2.weight'], got32['conv2.weight'])


# ---- composition, determinism, checkpoints -----------------------------------------
def test_bf16_update_equals_its_stages_and_is_reproducible():
    check_update_equals_its_stages(dict(backward_precision='bf16'))


def test_checkpoints_move_between_the_modes():
    check_checkpoints_move('backward_precision')


def test_default_mode_is_the_fp32_backward():
    key = (5, 5, 8, 3, 0, 70)
    case = LC.backward_case(key)
    obs, dq = case.obs.to(DEV), case.dq.to(DEV)
    state, _ = LC.descent_batch()                                      # real-valued weights on the probe's batch
    grads = []
    for kw in ({}, dict(backward_precision='fp32'), dict(backward_precision='bf16')):
        learner = make_learner(state, key, **kw)
        learner(obs)
        learner.backward(obs, dq)
        grads.append(learner.grads())
    assert make_learner(state, key).backward_precision == 'fp32'
    for name in LC.PARAMS:
        assert torch.equal(grads[0][name], grads[1][name]), name
    assert not torch.equal(grads[0]['conv2.weight'], grads[2]['conv2.weight'])
