"""GPU checks of the learner (marlenv.DQNLearner; dqn_train_kernels.hip).

The backward must EQUAL the float64 autograd reference on the integer probes of
tests/learner_cases.py (tests/test_learner_cpu.py proves that any fp32 summation
order is exact there); the TD loss equals it on the dyadic case and stays
within a derived bound on real values; clip + Adam stays within a bound derived
from the kernel's operation count; update() is bit-equal to its stages run by
hand, reproducible from run to run and across a checkpoint."""
import ctypes

import numpy as np
import pytest
import torch

import dqn_probe as P
import learner_cases as LC
from learner_gpu_util import DEV, KEY5, make_learner, probe_batch, run_ids, same, snapshot

pytestmark = pytest.mark.gpu


def run_backward(state, key, obs, dq):
    learner = make_learner(state, key)
    obs = obs.to(DEV)
    q = learner(obs)
    learner.backward(obs, dq.to(DEV))
    return q.cpu(), {k: v.cpu() for k, v in learner.grads().items()}


def localise(key, B):
    """Which single layer's backward is wrong: every other layer identity-like."""
    h, w, c, A, seed, _ = key
    bad = []
    for layer in P.LAYERS:
        state = P.probe_net(h, w, c, A, seed, identity=tuple(n for n in P.LAYERS if n != layer))
        obs, dq = P.probe_obs(key[5], h, w, c, seed)[:B].contiguous(), LC.probe_dq(key)[:B].contiguous()
        ref = LC.ref_grads(state, obs, dq)
        _, got = run_backward(state, key, obs, dq)
        wrong = [n for n in LC.PARAMS if not torch.equal(got[n].double(), ref[n])]
        if wrong:
            bad.append('%s alone: %s' % (layer, wrong))
    return '; '.join(bad) or 'no single layer reproduces it'


RUNS = LC.gpu_backward_runs()


@pytest.mark.parametrize('key,B', RUNS, ids=run_ids(RUNS))
def test_backward_equals_float64_reference(key, B):
    case = LC.backward_case(key, B)
    q, got = run_backward(case.state, key, case.obs, case.dq)
    assert torch.equal(q.double(), P.probe(*key).q[:B])
    wrong = {}
    for name in LC.PARAMS:
        assert got[name].shape == case.grads[name].shape
        if not torch.equal(got[name].double(), case.grads[name]):
            diff = (got[name].double() - case.grads[name]).abs()
            wrong[name] = (int((diff != 0).sum()), float(diff.max()))
    assert not wrong, '%s; %s' % (wrong, localise(key, B))


def test_backward_reads_the_scaled_observation():
    """Bytes above 1: the forward divides by 255, and conv1's weight gradient
    must read the same values (tolerance: the fp32 forward's own, 1e-5 of the
    reference's scale, since x / 255 is no integer)."""
    key = (5, 5, 8, 3, 0, 70)
    case = LC.backward_case(key)
    obs = (case.obs * 255).contiguous()
    ref = LC.ref_grads(case.state, obs, case.dq)
    _, got = run_backward(case.state, key, obs, case.dq)
    for name in LC.PARAMS:
        scale = float(ref[name].abs().max())
        assert float((got[name].double() - ref[name]).abs().max()) <= 1e-5 * scale, name


def test_backward_rejects_wrong_inputs():
    key = (5, 5, 8, 3, 0, 70)
    case = LC.backward_case(key)
    learner = make_learner(case.state, key)
    obs, dq = case.obs.to(DEV), case.dq.to(DEV)
    with pytest.raises(ValueError, match='last policy forward'):
        learner.backward(obs, dq)
    learner(obs)
    with pytest.raises(ValueError, match='last policy forward'):
        learner.backward(obs.clone(), dq)
    with pytest.raises(TypeError, match='dq'):
        learner.backward(obs, dq.double())
    with pytest.raises(ValueError, match='dq shape'):
        learner.backward(obs, dq[:5])
    with pytest.raises(TypeError, match='uint8'):
        learner(obs.float())
    with pytest.raises(ValueError, match='shape'):
        learner(obs[:, :4].contiguous())
    with pytest.raises(ValueError, match='on cpu'):
        learner(case.obs)


# ---- TD loss -------------------------------------------------------------------
def td_learner(gamma):
    return make_learner(P.probe_net(5, 5, 8, 3, 0), (5, 5, 8, 3), gamma=gamma)


@pytest.mark.parametrize('B', [64, 1])
def test_td_loss_dyadic_is_exact(B):
    inputs = tuple(t[:B].contiguous() for t in LC.td_dyadic_case(64))
    loss64, dq64, _ = LC.td_ref64(*inputs, 0.5)
    learner = td_learner(0.5)
    loss, dq = learner.td_loss(*(t.to(DEV) for t in inputs))
    assert loss.shape == () and loss.dtype == torch.float32
    assert torch.equal(dq.cpu().double(), dq64)
    assert float(loss) == float(loss64)
    assert int(learner.err.item()) == 0


def test_td_loss_real_values_within_the_derived_bound():
    """gamma = 0.99, B = 70. Bound (tests/learner_cases.py td_bounds): four
    rounded operations on quantities of magnitude <= S = |r| + |max q'| + |q|
    give |d - d64| <= E = 4 U S (U = 2^-24); dq adds one division: E / B + U
    (|dq| + E / B); the loss: (sum E + 10 U (sum l + sum E)) / B + U |loss| (a
    row's own rounding, 8 tree levels, the division)."""
    inputs = LC.td_real_case(70)
    loss64, dq64, _ = LC.td_ref64(*inputs, 0.99)
    loss_bound, dq_bound = LC.td_bounds(*inputs, 0.99)
    loss, dq = td_learner(0.99).td_loss(*(t.to(DEV) for t in inputs))
    err_dq = (dq.cpu().double() - dq64).abs()
    print('loss err %.3g (bound %.3g), dq err %.3g (bound %.3g)' % (
        abs(float(loss) - float(loss64)), loss_bound, float(err_dq.max()), float(dq_bound.max())))
    assert bool((err_dq <= dq_bound).all())
    assert abs(float(loss) - float(loss64)) <= loss_bound


def test_td_loss_clamps_an_action_out_of_range():
    q, action, reward, done, next_q = (t[:8].contiguous() for t in LC.td_dyadic_case(64))
    action = action.clone()
    action[5], action[6] = 7, -2
    clamped = action.clamp(0, 2)
    loss64, dq64, _ = LC.td_ref64(q, clamped, reward, done, next_q, 0.5)
    learner = td_learner(0.5)
    loss, dq = learner.td_loss(*(t.to(DEV) for t in (q, action, reward, done, next_q)))
    assert torch.equal(dq.cpu().double(), dq64) and float(loss) == float(loss64)
    assert int(learner.err.item()) == 1


def test_td_loss_rejects_wrong_inputs():
    learner = td_learner(0.5)
    q, action, reward, done, next_q = (t.to(DEV) for t in LC.td_dyadic_case(64))
    with pytest.raises(TypeError, match='action'):
        learner.td_loss(q, action.int(), reward, done, next_q)
    with pytest.raises(TypeError, match='reward'):
        learner.td_loss(q, action, reward.double(), done, next_q)
    with pytest.raises(ValueError, match='done'):
        learner.td_loss(q, action, reward, done[:5], next_q)
    with pytest.raises(ValueError, match='q shape'):
        learner.td_loss(q[:, :2], action, reward, done, next_q)
    with pytest.raises(ValueError, match='is on'):
        learner.td_loss(q, action.cpu(), reward, done, next_q)


# ---- clip + Adam ---------------------------------------------------------------
ADAM_N = 5000
HYPER = dict(lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=10.0)


def adam_inputs(scale, step):
    g = P._gen(ADAM_N, step, int(scale * 1000))
    grad = torch.randn(ADAM_N, generator=g) * scale
    grad[::7] = 0.0                                                 # exact zeros
    p = torch.randn(ADAM_N, generator=g)
    if step == 1:
        m, v = torch.zeros(ADAM_N), torch.zeros(ADAM_N)
    else:
        m, v = torch.randn(ADAM_N, generator=g) * scale, (torch.randn(ADAM_N, generator=g) * scale) ** 2
        m[::7], v[::7] = 0.0, 0.0
    return p, grad, m, v


@pytest.mark.parametrize('step', [1, 2, 1000])
@pytest.mark.parametrize('scale', [1.0, 0.01], ids=['norm-above-10', 'norm-below-10'])
def test_adam_step_within_the_derived_bound(scale, step):
    """Against float64 on the same fp32 inputs: |p - p64| <= ulp(p) / 2 + K U S,
    S the step's magnitude and K from the kernel's operation count
    (tests/learner_cases.py adam_bounds, where the count is written out)."""
    from marlenv import _native
    L = _native.lib()
    p, grad, m, v = adam_inputs(scale, step)
    p64, m64, v64, norm64, S = LC.adam_ref64(p, grad, m, v, step, **HYPER)
    assert (norm64 > 10.0) == (scale == 1.0)
    dp, dg, dm, dv = (t.to(DEV) for t in (p, grad, m, v))
    scratch = torch.zeros(_native.ADAM_SCRATCH_BYTES, dtype=torch.uint8, device=DEV)
    norm = torch.zeros((), dtype=torch.float32, device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    _native.check(L.snake_adam_step(vp(dp), vp(dg), vp(dm), vp(dv), ADAM_N, step, HYPER['lr'], HYPER['beta1'],
                                    HYPER['beta2'], HYPER['eps'], HYPER['max_norm'], vp(scratch), vp(norm),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), L)
    e_n, K = LC.adam_bounds(ADAM_N)
    got = dp.cpu()
    half_ulp = torch.from_numpy(np.spacing(np.maximum(got.abs().numpy(), p64.abs().float().numpy()))).double() / 2
    err = (got.double() - p64).abs()
    bound = half_ulp + K * LC.U * S
    print('norm rel err %.3g (bound %.3g); worst p err / bound %.3f' % (
        abs(float(norm) - norm64) / norm64, e_n + LC.U, float((err / bound.clamp(min=1e-300)).max())))
    assert abs(float(norm) - norm64) <= (e_n + LC.U) * norm64        # (+ U: the float the norm is stored as)
    assert bool((err <= bound).all())
    zero = (grad == 0) & (m == 0) & (v == 0)
    assert int(zero.sum()) > 100 and torch.equal(got[zero], p[zero])
    assert torch.equal(dg.cpu(), grad)                                # the gradient is not written
    # m and v: the same counts (adam_bounds): (e_g + 3 U) of the terms' magnitudes, 2 e_g + 4 U of v
    e_g = e_n + 3 * LC.U
    b1, b2 = float(np.float32(HYPER['beta1'])), float(np.float32(HYPER['beta2']))
    coef = min(1.0, 10.0 / (norm64 + 1e-6))
    am = (b1 * m.double()).abs() + ((1 - b1) * coef * grad.double()).abs()
    assert bool(((dm.cpu().double() - m64).abs() <= (e_g + 3 * LC.U) * LC.SLACK * am).all())
    assert bool(((dv.cpu().double() - v64).abs() <= (2 * e_g + 4 * LC.U) * LC.SLACK * v64).all())


# ---- composition and determinism -------------------------------------------------
def test_update_equals_its_stages_and_is_reproducible():
    """On the integer probe net, so not learner_gpu_util.check_update_equals_its_stages
    (a real-valued net against its fp32 twin)."""
    state = P.probe_net(5, 5, 8, 3, 0)
    batch = probe_batch()
    s, a, r, ns, d = batch
    whole, by_hand = make_learner(state, KEY5), make_learner(state, KEY5)
    losses, hand_losses, ckpt = [], [], None
    for i in range(3):
        losses.append(whole.update(*batch))
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
    assert not torch.equal(whole._param, whole._target)               # the policy moved, the target did not
    w = whole.state_dict()['fc2.weight']
    assert not torch.equal(w, w.round())                              # non-integer weights after Adam
    # updates 2 and 3 again, twice, from the checkpoint after update 1 (a fresh learner each time)
    for _ in range(2):
        again = make_learner(P.probe_net(5, 5, 8, 3, 1), KEY5)
        again.load_checkpoint(ckpt)
        assert again.step == 1
        l2, l3 = again.update(*batch), again.update(*batch)
        assert same(snapshot(again), snapshot(whole))
        assert torch.equal(l2, losses[1]) and torch.equal(l3, losses[2])
    assert float(whole.grad_norm) > 0


def test_sync_target_and_state_dict():
    state, _ = LC.descent_batch()
    learner = make_learner(state, KEY5)
    batch = probe_batch()
    obs = batch[0]
    learner.update(*batch)
    assert not torch.equal(learner.target_q(obs), learner(obs))
    learner.sync_target()
    q = learner(obs)
    assert torch.equal(learner.target_q(obs), q)
    ref = LC.TorchDQN(5, 5, 8, 3).double()
    ref.load_state_dict(learner.state_dict())
    q64 = ref(obs.cpu()).detach()
    assert float((q.double().cpu() - q64).abs().max()) <= 1e-5 * float(q64.abs().max())
    assert learner.forward_features(obs).shape == (64, 128)
    for name, t in learner.checkpoint()['optimizer']['exp_avg'].items():
        assert t.shape == state[name].shape


def test_twenty_updates_lower_the_loss():
    state, batch = LC.descent_batch()
    learner = make_learner(state, KEY5)
    batch = tuple(t.to(DEV) for t in batch)
    losses = [learner.update(*batch) for _ in range(20)]
    first, last = float(losses[0]), float(losses[-1])
    print(first, last)
    assert last < first


def test_collector_drives_the_learner():
    """The README's loop: Collector.run(learner, ...) then update on a sample."""
    from marlenv import Collector, ReplayBuffer, SnakeVecEnv
    env = SnakeVecEnv(16, num_snakes=2, height=10, width=10, vision_range=2, seed=3)
    S, h, w, c = env.obs_shape
    buf = ReplayBuffer(env.obs_shape, 4096)
    torch.manual_seed(5)
    learner = make_learner(LC.TorchDQN(h, w, c, 3).state_dict(), (h, w, c, 3))
    Collector(env, buf).run(learner, steps=8, epsilon=0.5)
    loss = learner.update(*buf.sample(64))
    assert loss.shape == () and bool(torch.isfinite(loss)) and learner.step == 1
