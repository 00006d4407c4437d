"""GPU checks of the bf16 mixed-precision forward (DQNLearner(forward_precision=
'bf16'), target_precision='mixed'; dqn_fwd16_kernels.hip,
snake_dqn32_forward_bf16).

On the integer probes of tests/learner_cases.py bf16 holds every staged operand
exactly, so Y1..Y5, the features and Q must EQUAL dqn_probe.ref64 and the
gradients of either backward the autograd reference. On the rounding cases
(conv1 x 61) everything must EQUAL the float64 model of
tests/learner_model.py, which rounds exactly where include/snake_env.h
says the kernel rounds (tests/test_learner_fwd16_cpu.py proves the
preconditions). On real values it stays within a tolerance the model sets. Rows
do not depend on their batch; update() is bit-equal to its stages, reproducible,
and checkpoints move between the modes."""
import pytest
import torch

import dqn_probe as P
import learner16_cases as L16
import learner_cases as LC
import learner_fwd16_cases as FC
import learner_model as M
from learner_gpu_util import (DEV, KEY5, check_checkpoints_move, check_update_equals_its_stages, key_ids,
                              make_learner, run_ids)

pytestmark = pytest.mark.gpu

ALL16 = dict(forward_precision='bf16', backward_precision='bf16', target_precision='mixed')


class Run:
    """One forward (Y1..Y5, features, Q) and both backwards of it, on the CPU."""

    def __init__(self, state, key, obs, dq=None, forward='bf16'):
        obs = obs.to(DEV)
        self.grads = {}
        for mode in ('fp32', 'bf16') if dq is not None else ('fp32',):
            learner = make_learner(state, key, forward_precision=forward, backward_precision=mode)
            assert learner.forward_precision == forward
            feat = learner.forward_features(obs)
            y_feat = learner.pre_activations()
            q = learner(obs)
            self.Y = {k: v.cpu() for k, v in learner.pre_activations().items()}
            assert all(torch.equal(self.Y[n], y_feat[n].cpu()) for n in FC.YS)
            self.feat, self.q = feat.cpu(), q.cpu()
            if dq is not None:
                learner.backward(obs, dq.to(DEV))
                self.grads[mode] = {k: v.cpu() for k, v in learner.grads().items()}


def wrong_tensors(run, Y, feat, q, grads=None):
    """The names of what differs from the float64 expectation, forward first, in layer order."""
    B, (h, w) = run.q.shape[0], tuple(run.Y['Y1'].shape[1:3])
    shapes = {'Y1': (B, h, w, 32), 'Y2': (B, h, w, 64), 'Y3': (B, h, w, 64), 'Y4': (B, 256), 'Y5': (B, 128)}
    wrong = []
    for name in FC.YS:
        assert tuple(run.Y[name].shape) == shapes[name] and run.Y[name].dtype == torch.float32
        if not torch.equal(run.Y[name].double(), Y[name]):
            wrong.append(name)
    if not torch.equal(run.feat.double(), feat):
        wrong.append('features')
    if not torch.equal(run.q.double(), q):
        wrong.append('Q')
    for mode, ref in (grads or {}).items():
        wrong += ['%s (%s backward)' % (n, mode) for n in LC.PARAMS if not torch.equal(run.grads[mode][n].double(), ref[n])]
    return wrong


def localise(key, B, scale=1.0):
    """Which single layer's forward is wrong: every other layer identity-like."""
    h, w, c, A, seed, _ = key
    bad = []
    for layer in P.LAYERS:
        state = P.probe_net(h, w, c, A, seed, identity=tuple(n for n in P.LAYERS if n != layer))
        if scale != 1.0:
            state = FC.scaled_state(state, scale)
        obs = P.probe_obs(key[5], h, w, c, seed)[:B].contiguous()
        model = M.forward_model(state, obs)
        wrong = wrong_tensors(Run(state, key, obs), model.Y, model.feat, model.q)
        if wrong:
            bad.append('%s alone: %s' % (layer, wrong))
    return '; '.join(bad) or 'no single layer reproduces it'


RUNS = FC.exact_runs()


@pytest.mark.parametrize('key,B', RUNS, ids=run_ids(RUNS))
def test_bf16_forward_equals_float64_reference(key, B):
    case = LC.backward_case(key, B)
    feat, q, _ = P.ref64(case.state, case.obs)
    Y = FC.reference_y(case.state, case.obs)
    run = Run(case.state, key, case.obs, case.dq)
    wrong = wrong_tensors(run, Y, feat, q, {'fp32': case.grads, 'bf16': case.grads})
    assert not wrong, '%s; %s' % (wrong, localise(key, B))


def test_bytes_0_255_take_the_flag_path_exactly():
    key = FC.BYTES_KEY
    case = LC.backward_case(key)
    feat, q, _ = P.ref64(case.state, case.obs)
    ones, scaled = Run(case.state, key, case.obs, case.dq), Run(case.state, key, case.obs * 255, case.dq)
    grads = {'fp32': case.grads, 'bf16': case.grads}
    assert not wrong_tensors(scaled, FC.reference_y(case.state, case.obs), feat, q, grads)
    for name in FC.YS:
        assert torch.equal(scaled.Y[name], ones.Y[name]), name
    assert torch.equal(scaled.q, ones.q) and torch.equal(scaled.feat, ones.feat)
    for mode in grads:
        for name in LC.PARAMS:
            assert torch.equal(scaled.grads[mode][name], ones.grads[mode][name]), (mode, name)


@pytest.mark.parametrize('key', FC.ROUNDING_KEYS, ids=key_ids(FC.ROUNDING_KEYS))
def test_bf16_forward_equals_the_rounding_model(key):
    c = FC.rounding_case(key)
    run = Run(c.state, key, c.obs, c.dq)
    wrong = wrong_tensors(run, c.model.Y, c.model.feat, c.model.q, c.grads)
    assert not wrong, '%s; %s' % (wrong, localise(key, key[5], FC.ROUNDING_SCALE))
    # the fp32 mode on the same input is the unrounded float64 forward: the bf16 kernels did run
    run32 = Run(c.state, key, c.obs, forward='fp32')
    assert not wrong_tensors(run32, c.exact.Y, c.exact.feat, c.exact.q)
    assert torch.equal(run.Y['Y1'], run32.Y['Y1'])
    for name in FC.YS[1:]:
        assert not torch.equal(run.Y[name], run32.Y[name]), name
    assert not torch.equal(run.q, run32.q)


@pytest.mark.parametrize('scaled', [False, True], ids=['bytes-0-1', 'bytes-0-255'])
def test_bf16_forward_real_values_within_the_model_tolerance(scaled):
    """Per tensor T in {Y1..Y5, Q, each gradient}: |got - ref64| <= 1.5 |model -
    ref64| + 1e-5 |ref64| (2-norms): ref64 the unrounded float64 forward and its
    autograd gradients, model the float64 bf16 model. The kernel differs from
    the model only by fp32 summation order (2^-24 per addition against 2^-9 per
    rounded operand) and by rare ties at a rounding boundary, hence 1.5; 1e-5 is
    the fp32 path's own tolerance, for what the model does not round. The masks
    are the model's: the CPU file asserts every unit of its chain is 2e-5 of its
    layer's scale away from its threshold."""
    state, obs, dq = FC.real_case(scaled)
    key = L16.REAL_GEOM
    model, ref_y = M.forward_model(state, obs), FC.reference_y(state, obs)
    q64, g64 = P.ref64(state, obs)[1], LC.ref_grads(state, obs, dq)
    run, run32 = Run(state, key, obs, dq), Run(state, key, obs, dq, forward='fp32')
    rows = [(n, run.Y[n], run32.Y[n], model.Y[n], ref_y[n]) for n in FC.YS] + [('Q', run.q, run32.q, model.q, q64)]
    for mode, rnd in FC.BACKWARD_RND.items():
        grads = M.backward_model(state, obs, dq, rnd, pre=model.pre)[0]
        rows += [('%s/%s' % (n, mode), run.grads[mode][n], run32.grads[mode][n], grads[n], g64[n]) for n in LC.PARAMS]
    failed = []
    for name, got, got32, mod, ref in rows:
        err, model_err = float((got.double() - ref).norm()), float((mod - ref).norm())
        ref_norm, err32 = float(ref.norm()), float((got32.double() - ref).norm())
        print('%-18s |got - ref64| %.4g  |model - ref64| %.4g  ratio %.4f  |ref64| %.4g  (fp32 forward: %.4g)' % (
            name, err, model_err, err / model_err if model_err else 0.0, ref_norm, err32))
        if not err <= 1.5 * model_err + 1e-5 * ref_norm:
            failed.append(name)
    assert not failed
    assert not torch.equal(run.Y['Y2'], run32.Y['Y2']) and not torch.equal(run.q, run32.q)


def test_rows_do_not_depend_on_their_batch():
    key = FC.PREFIX_KEY
    full = LC.backward_case(key)
    state, _ = LC.descent_batch()                       # real-valued weights: a summation order would show
    learner = make_learner(state, key, forward_precision='bf16')
    got = {}
    for B in FC.PREFIX_B:
        obs = full.obs[:B].contiguous().to(DEV)
        feat = learner.forward_features(obs)
        got[B] = dict(learner.pre_activations(), feat=feat, q=learner(obs))
    top = got[max(FC.PREFIX_B)]
    for B in FC.PREFIX_B:
        for name, t in got[B].items():
            assert torch.equal(t, top[name][:B]), (B, name)
    assert FC.fc1_chunks(key)[0] == 2                   # and fc1 did split


# ---- composition, determinism, checkpoints -----------------------------------------
def test_bf16_update_equals_its_stages_and_is_reproducible():
    check_update_equals_its_stages(ALL16, differs_after_first_step=True)


def test_checkpoints_move_between_the_forward_modes():
    check_checkpoints_move('forward_precision')


def test_mixed_target_is_the_bf16_policy_forward_after_a_sync():
    key = (4, 33, 8, 3)                                                # no bf16 plan takes it
    state = P.probe_net(5, 5, 8, 3, 1)
    real, _ = LC.descent_batch()
    obs = P.probe_obs(64, 5, 5, 8, 21).to(DEV)
    learner = make_learner(real, KEY5, forward_precision='bf16', target_precision='mixed')
    assert learner.target_precision == 'mixed' and learner._target16 is None
    learner.load_checkpoint(dict(learner.checkpoint(), target_net=state))       # target != policy
    assert not torch.equal(learner.target_q(obs), learner(obs))
    learner.sync_target()
    assert torch.equal(learner.target_q(obs), learner(obs))
    assert not torch.equal(learner(obs), make_learner(real, KEY5)(obs))         # and not the fp32 forward
    fp32_target = make_learner(real, KEY5, forward_precision='bf16')
    assert torch.equal(fp32_target.target_q(obs), make_learner(real, KEY5).target_q(obs))
    wide = make_learner(P.probe_net(*key, 0), key, target_precision='mixed')
    wobs = P.probe_obs(3, 4, 33, 8, 0).to(DEV)
    assert torch.equal(wide.target_q(wobs).double().cpu(), P.ref64(P.probe_net(*key, 0), wobs)[1])


def test_default_mode_is_the_fp32_forward():
    key = (5, 5, 8, 3, 0, 70)
    case = LC.backward_case(key)
    obs, dq = case.obs.to(DEV), case.dq.to(DEV)
    state, _ = LC.descent_batch()                                      # real-valued weights on the probe's batch
    qs, grads = [], []
    for kw in ({}, dict(forward_precision='fp32'), dict(forward_precision='bf16')):
        learner = make_learner(state, key, **kw)
        if not qs:
            with pytest.raises(ValueError, match='policy forward'):
                learner.pre_activations()
        qs.append(learner(obs))
        learner.backward(obs, dq)
        grads.append(learner.grads())
    assert make_learner(state, key).forward_precision == 'fp32'
    assert torch.equal(qs[0], qs[1]) and not torch.equal(qs[0], qs[2])
    for name in LC.PARAMS:
        assert torch.equal(grads[0][name], grads[1][name]), name
    assert not torch.equal(grads[0]['conv2.weight'], grads[2]['conv2.weight'])


def test_twenty_all_bf16_updates_lower_the_loss():
    state, batch = LC.descent_batch()
    batch = tuple(t.to(DEV) for t in batch)
    learner = make_learner(state, KEY5, **ALL16)
    losses = [float(learner.update(*batch)) for _ in range(20)]
    print('loss %.5f -> %.5f' % (losses[0], losses[-1]))
    assert losses[-1] < losses[0]
