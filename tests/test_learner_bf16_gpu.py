"""GPU checks of the bf16 backward (DQNLearner(backward_precision='bf16');
dqn_train16_kernels.hip, snake_dqn32_backward_bf16).

On the integer probes of tests/learner_cases.py bf16 holds every staged operand
exactly, so the result must EQUAL the float64 autograd reference, as the fp32
backward's does. On the rounding cases (dq x 29) it must EQUAL the float64 model
of tests/learner16_cases.py, which rounds exactly where include/snake_env.h says
the kernel rounds (tests/test_learner_bf16_cpu.py proves both preconditions).
On real values it stays within a tolerance the model sets. update() in bf16 mode
is bit-equal to its stages, reproducible, and checkpoints move between modes."""
import pytest
import torch

import dqn_probe as P
import learner16_cases as L16
import learner_cases as LC

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def make_learner(state, key, **kw):
    from marlenv import DQNLearner
    h, w, c, A = key[:4]
    return DQNLearner(state, h, w, c, num_actions=A, device=DEV, **kw)


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


@pytest.mark.parametrize('key,B', RUNS, ids=['%dx%dx%d-A%d-s%d-B%d' % (k[:5] + (b,)) for k, b in RUNS])
def test_bf16_backward_equals_float64_reference(key, B):
    case = LC.backward_case(key, B)
    q, got = run_backward(case.state, key, case.obs, case.dq)
    assert torch.equal(q.double(), P.probe(*key).q[:B])
    wrong = mismatches(got, case.grads)
    assert not wrong, '%s; %s' % (wrong, localise(key, B))


@pytest.mark.parametrize('key', L16.ROUNDING_KEYS, ids=['%dx%dx%d-A%d-s%d-B%d' % k for k in L16.ROUNDING_KEYS])
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
def probe_batch(B=64):
    g = P._gen(B, 31337)
    state, next_state = P.probe_obs(B, 5, 5, 8, 21), P.probe_obs(B, 5, 5, 8, 22)
    action = torch.randint(0, 3, (B,), generator=g)
    reward = torch.randint(-2, 3, (B,), generator=g).float()
    done = (torch.rand(B, generator=g) < 0.25).float()
    return tuple(t.to(DEV) for t in (state, action, reward, next_state, done))


KEY5 = (5, 5, 8, 3)


def snapshot(learner):
    return [learner._param.clone(), learner._m.clone(), learner._v.clone(), learner._target.clone()]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_bf16_update_equals_its_stages_and_is_reproducible():
    state, _ = LC.descent_batch()                                     # real-valued: rounding matters from step 1
    batch = probe_batch()
    s, a, r, ns, d = batch
    kw = dict(backward_precision='bf16')
    whole, by_hand, fp32 = make_learner(state, KEY5, **kw), make_learner(state, KEY5, **kw), make_learner(state, KEY5)
    losses, hand_losses, ckpt = [], [], None
    for i in range(3):
        losses.append(whole.update(*batch))
        fp32.update(*batch)
        nq = by_hand.target_q(ns)
        q = by_hand(s)
        loss, dq = by_hand.td_loss(q, a, r, d, nq)
        by_hand.backward(s, dq)
        by_hand.apply()
        hand_losses.append(loss)
        if i == 0:
            ckpt = whole.checkpoint()
    assert whole.step == by_hand.step == 3
    assert same(snapshot(whole), snapshot(by_hand))
    assert all(torch.equal(x, y) for x, y in zip(losses, hand_losses))
    assert not torch.equal(whole._param, fp32._param)                  # the bf16 backward is another computation
    assert torch.equal(whole._target, fp32._target)
    # updates 2 and 3 again, twice, from the checkpoint after update 1 (a fresh learner each time)
    for _ in range(2):
        again = make_learner(P.probe_net(5, 5, 8, 3, 1), KEY5, **kw)
        again.load_checkpoint(ckpt)
        assert again.step == 1
        l2, l3 = again.update(*batch), again.update(*batch)
        assert same(snapshot(again), snapshot(whole))
        assert torch.equal(l2, losses[1]) and torch.equal(l3, losses[2])
    assert float(whole.grad_norm) > 0


def test_checkpoints_move_between_the_modes():
    state, _ = LC.descent_batch()
    batch = probe_batch()
    for first, second in (('bf16', 'fp32'), ('fp32', 'bf16')):
        a = make_learner(state, KEY5, backward_precision=first)
        a.update(*batch)
        ckpt = a.checkpoint()
        b = make_learner(P.probe_net(5, 5, 8, 3, 1), KEY5, backward_precision=second)
        b.load_checkpoint(ckpt)
        assert b.backward_precision == second and b.step == 1
        assert same(snapshot(b), snapshot(a))
        # from the same state, the loaded learner continues as one of its own mode does
        c = make_learner(P.probe_net(5, 5, 8, 3, 1), KEY5, backward_precision=second)
        c.load_checkpoint(ckpt)
        assert torch.equal(b.update(*batch), c.update(*batch)) and same(snapshot(b), snapshot(c))
        a.update(*batch)
        assert not torch.equal(a._param, b._param)                     # and not as the other mode


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
