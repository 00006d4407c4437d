"""GPU checks of where the fused bf16 DQN forward rounds (DQNForward(precision=
'bf16'): k_dqn_conv, k_dqn_map_conv and k_dqn_fc of dqn_kernels.hip, behind
snake_dqn_forward and snake_dqn_map_forward).

On the rounding cases of tests/dqn_round_cases.py (integer probes, conv1 x 61)
the features and Q must EQUAL the float64 model of tests/learner_model.py, which
rounds relu(Y + b) of conv1, conv2, conv3 and fc1 to nearest even and nothing
else, exactly where include/snake_env.h says these kernels round
(tests/test_dqn_round_cpu.py proves the preconditions, and that truncation, ties
rounded up, a missed or an added rounding point each give another Q). The same
holds in later iterations of a persistent workgroup, on bytes above 1 (read at
their value), and for a learner's actor, its bf16 target and its mixed-precision
forward, which then agree bit for bit. On real values the kernels stay within a
tolerance the model sets."""
import pytest
import torch

import dqn_probe as P
import dqn_round_cases as RC
import learner_fwd16_cases as FC
import learner_model as M
from learner_gpu_util import DEV, key_ids, make_learner

pytestmark = pytest.mark.gpu


def map_waves():
    from marlenv.dqn import MAP_CONV_WAVES
    return MAP_CONV_WAVES


def fused(state, key, plan, waves=0):
    from marlenv.dqn import DQNForward
    h, w, c, A = key[:4]
    net = DQNForward({k: v.to(DEV) for k, v in state.items()}, h, w, c, A, device=DEV, conv_waves=waves, plan=plan)
    assert net.plan == plan and net.precision == 'bf16'
    return net


def run(net, obs):
    """(features, q) as float64 on the CPU."""
    q, feat = net(obs), net.forward_features(obs)
    torch.cuda.synchronize()
    return feat.double().cpu(), q.double().cpu()


def differing(got, want, what):
    """'' where got equals want, else a line on what differs."""
    if got.shape == want.shape and torch.equal(got, want):
        return ''
    if got.shape != want.shape:
        return '%s: shape %s, want %s' % (what, tuple(got.shape), tuple(want.shape))
    bad = (got != want).nonzero()
    i = tuple(bad[0].tolist())
    return '%s: %d of %d differ, first at %s: got %r, want %r; rows %s' % (
        what, bad.size(0), want.numel(), i, float(got[i]), float(want[i]), sorted(set(bad[:, 0].tolist()))[:16])


def wrong_tensors(net, obs, model, rows=None):
    feat, q = run(net, obs)
    want_f, want_q = (model.feat, model.q) if rows is None else (model.feat[rows], model.q[rows])
    return [s for s in (differing(feat, want_f, 'features'), differing(q, want_q, 'Q')) if s]


def localise(key, plan, waves):
    """Which single layer's forward is wrong: every other layer identity-like, conv1 x 61."""
    h, w, c, A, seed, B = key
    obs = P.probe_obs(B, h, w, c, seed)
    bad = []
    for layer in P.LAYERS:
        state = FC.scaled_state(P.probe_net(h, w, c, A, seed, identity=tuple(n for n in P.LAYERS if n != layer)))
        wrong = wrong_tensors(fused(state, key, plan, waves), obs.to(DEV), M.forward_model(state, obs))
        if wrong:
            bad.append('%s alone: %s' % (layer, wrong))
    return '; '.join(bad) or 'no single layer reproduces it'


def check_rounding_case(key, plan, all_waves):
    c = RC.rounding_case(key)
    obs = c.obs.to(DEV)
    for waves in all_waves:
        net = fused(c.state, key, plan, waves)
        wrong = wrong_tensors(net, obs, c.model)
        assert not wrong, 'conv_waves %d: %s; %s' % (waves, wrong, localise(key, plan, waves))
        # and the case did reach the rounding: this is not the unrounded chain's result
        feat, q = run(net, obs)
        assert not torch.equal(q, c.exact.q) and not torch.equal(feat, c.exact.feat)


@pytest.mark.parametrize('key', RC.WINDOW_KEYS, ids=key_ids(RC.WINDOW_KEYS))
def test_window_forward_equals_the_rounding_model(key):
    check_rounding_case(key, 'window', RC.WINDOW_WAVES)


@pytest.mark.parametrize('key', RC.MAP_KEYS, ids=key_ids(RC.MAP_KEYS))
def test_map_forward_equals_the_rounding_model(key):
    check_rounding_case(key, 'map', map_waves())


@pytest.mark.parametrize('plan', sorted(RC.PERSIST_KEYS))
def test_rounding_survives_the_persistent_loop(plan):
    """The batch of test_bf16_persistent_loop / test_map_persistent_loop: more
    observations than twice the workgroups the device holds, so every workgroup
    runs at least two, gathered from 64 unique rows by a random index vector."""
    key = RC.PERSIST_KEYS[plan]
    c = RC.rounding_case(key)
    net = fused(c.state, key, plan)
    obs = c.obs.to(DEV)
    assert not wrong_tensors(net, obs, c.model), 'unique rows'
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 2 * (32 if plan == 'window' else 160 * 1024 // net.layout.lds_conv) * n_cu + 77
    idx = torch.randint(0, RC.PERSIST_UNIQUE, (B,), generator=torch.Generator().manual_seed(17))
    wrong = wrong_tensors(net, obs[idx.to(DEV)].contiguous(), c.model, idx)
    assert not wrong, 'B %d: %s' % (B, wrong)
    assert not torch.equal(c.model.q[idx], c.exact.q[idx])


BYTE_RUNS = [(key, plan) for key, plans in RC.BYTE_CASES for plan in plans]


@pytest.mark.parametrize('key,plan', BYTE_RUNS, ids=['%s-%s' % (i, p) for i, (_, p) in
                                                     zip(key_ids([k for k, _ in BYTE_RUNS]), BYTE_RUNS)])
def test_bytes_are_read_at_their_value(key, plan):
    """Bytes from {1, 2, 3, 128, 255}: the fused forward has no / 255 branch."""
    c = RC.byte_case(key)
    obs = c.obs.to(DEV)
    for waves in (RC.WINDOW_WAVES if plan == 'window' else map_waves()):
        net = fused(c.state, key, plan, waves)
        wrong = wrong_tensors(net, obs, c.model)
        assert not wrong, 'conv_waves %d: %s' % (waves, wrong)
    feat, q = run(net, obs)
    assert not torch.equal(q, c.exact.q)                                # rounded ...
    assert not torch.equal(q, M.forward_model(c.state, c.obs).q)        # ... and not divided by 255


@pytest.mark.parametrize('key,plan', RC.LEARNER_KEYS, ids=key_ids([k for k, _ in RC.LEARNER_KEYS]))
def test_actor_and_bf16_target_see_the_model(key, plan):
    """The fused kernels on the device pack's weights (the actor, the bf16
    target) and the mixed-precision forward on the fp32 masters round at the
    same points: all three equal the model's Q, and so each other."""
    c = FC.rounding_case(key)
    obs = c.obs.to(DEV)
    learner = make_learner(c.state, key, forward_precision='bf16')
    actor = learner.actor()
    assert actor.plan == plan and actor.precision == 'bf16'
    target = make_learner(c.state, key, target_precision='bf16')
    assert target._target16 is not None and target._target16.plan == plan
    got = {'actor': actor(obs), 'mixed-precision forward': learner(obs), 'bf16 target': target.target_q(obs)}
    torch.cuda.synchronize()
    wrong = [s for s in (differing(v.double().cpu(), c.model.q, name) for name, v in got.items()) if s]
    assert not wrong, wrong
    assert torch.equal(got['actor'], got['mixed-precision forward']) and torch.equal(got['actor'], got['bf16 target'])
    assert not torch.equal(got['actor'].double().cpu(), c.exact.q)
    assert not torch.equal(make_learner(c.state, key)(obs), got['actor'])          # the fp32 forward is another result


@pytest.mark.parametrize('plan', ['window', 'map'])
def test_real_values_within_the_model_tolerance(plan):
    """For Q and for the features: |got - ref64| <= 1.5 |model - ref64| + 1e-5
    |ref64| (2-norms), tests/test_learner_fwd16_gpu.py's criterion: ref64 the
    unrounded float64 forward, model the float64 bf16 model. The kernels differ
    from the model only by fp32 summation order (2^-24 per addition against 2^-9
    per rounded operand) and by rare ties at a rounding boundary, hence 1.5;
    1e-5 is the fp32 path's own tolerance, for what the model does not round.
    The zeros are the model's: the CPU file asserts every unit of both chains is
    2e-5 of its layer's scale away from its threshold."""
    state, obs = RC.real_case()
    key = RC.REAL_GEOM
    model = M.forward_model(state, obs)
    feat64, q64, _ = P.ref64(state, obs)
    feat, q = run(fused(state, key, plan), obs.to(DEV))
    failed = []
    for name, got, mod, ref in (('Q', q, model.q, q64), ('features', feat, model.feat, feat64)):
        err, model_err, ref_norm = float((got - ref).norm()), float((mod - ref).norm()), float(ref.norm())
        print('%-8s |got - ref64| %.4g  |model - ref64| %.4g  ratio %.4f  |ref64| %.4g  |got - model| %.4g' % (
            name, err, model_err, err / model_err if model_err else 0.0, ref_norm, float((got - mod).norm())))
        if not err <= 1.5 * model_err + 1e-5 * ref_norm:
            failed.append(name)
    assert not failed
