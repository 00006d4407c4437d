"""GPU checks of the pack kernel and of what the learner builds on it
(dqn_pack_kernels.hip; DQNForward.empty / pack32, DQNLearner.actor(),
target_precision='bf16').

k_dqn_pack must EQUAL the torch packing of tests/dqn_pack_ref.py run on the CPU,
bit for bit, on the real-valued nets of tests/dqn_pack_cases.py over 0xFF-filled
buffers; so must a DQNForward built from a state dict, which packs through the
same kernel. An actor must hold exactly the packing of learner.state_dict() and give
exactly the Q-values of a DQNForward built from it, after construction, after
updates, after a checkpoint round trip; a bf16 target net the same for
target_state_dict(). The default learner computes what it did, actor or none."""
import gc

import pytest
import torch

import dqn_pack_cases as PC
import dqn_probe as P
import learner_cases as LC

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.mark.parametrize('plan,h,w,c,A', PC.CASES, ids=PC.IDS)
def test_kernel_pack_equals_the_torch_packing(plan, h, w, c, A):
    from marlenv.dqn import DQNForward
    state, want = PC.case(plan, h, w, c, A)
    fwd = DQNForward.empty(h, w, c, num_actions=A, device=DEV, plan=plan)
    assert fwd.plan == plan
    PC.fill_ff(fwd)
    keep, net32 = PC.kernel_net(state, h, w, DEV)
    fwd.pack32(net32)
    first = PC.packed_bits(fwd)
    PC.assert_equal_bits(first, want, 'first call')
    fwd.pack32(net32)
    PC.assert_equal_bits(PC.packed_bits(fwd), first, 'second call')


@pytest.mark.parametrize('plan,h,w,c,A', [('window', 3, 3, 8, 3), ('window', 11, 11, 24, 4), ('map', 1, 7, 8, 3),
                                          ('map', 20, 20, 8, 3)])
def test_constructor_equals_the_torch_packing(plan, h, w, c, A):
    """A DQNForward built from a state dict on the device: a transient fp32 net,
    one launch of the pack kernel into uninitialised buffers."""
    from marlenv.dqn import DQNForward
    state, want = PC.case(plan, h, w, c, A)
    fwd = DQNForward(state, h, w, c, num_actions=A, device=DEV, plan=plan)
    assert fwd.plan == plan and fwd._source is None
    PC.assert_equal_bits(PC.packed_bits(fwd), want)


def test_constructor_and_empty_pack32_give_the_same_q():
    from marlenv.dqn import DQNForward
    state = PC.real_state(5, 5, 8, 3, crafted=False)
    obs = P.probe_obs(70, 5, 5, 8, 3).to(DEV)
    built = DQNForward(state, 5, 5, 8, device=DEV)
    filled = DQNForward.empty(5, 5, 8, device=DEV)
    keep, net32 = PC.kernel_net(state, 5, 5, DEV)
    filled.pack32(net32)
    q, want = built(obs), filled(obs)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    assert torch.equal(q, want)


def test_nan_packs_to_nan():
    from marlenv.dqn import DQNForward
    state = PC.real_state(3, 3, 8, 3, crafted=False)
    nans = torch.tensor([0x7f800001, 0x7fc00000, -1, 0x7fffffff], dtype=torch.int32).view(torch.float32)
    for name in ('conv1.weight', 'conv2.weight', 'conv3.weight', 'fc1.weight', 'fc2.weight'):
        state[name].view(-1)[:4] = nans
    fwd = DQNForward.empty(3, 3, 8, device=DEV)
    keep, net32 = PC.kernel_net(state, 3, 3, DEV)
    fwd.pack32(net32)
    for k in PC.BF16:
        got = fwd.tensors[k].view(torch.bfloat16).float()
        assert int(got.isnan().sum()) == 4 and not bool(got.isinf().any()), k


def test_misaligned_weights_are_refused():
    from marlenv._native import Dqn32Net, NativeError
    from marlenv.dqn import DQNForward
    fwd = DQNForward.empty(3, 3, 8, device=DEV)
    keep, net32 = PC.kernel_net(PC.real_state(3, 3, 8, 3), 3, 3, DEV)
    ptrs = [t.data_ptr() for t in keep]
    ptrs[3] += 4
    with pytest.raises(NativeError, match='aligned'):
        fwd.pack32(Dqn32Net(*ptrs))


def make_learner(state, h, w, c, A=3, **kw):
    from marlenv import DQNLearner
    return DQNLearner(state, h, w, c, num_actions=A, device=DEV, **kw)


def follows(actor, state, obs, what):
    """The two equalities: the actor's buffers are the torch packing of `state`,
    and its Q-values those of a DQNForward built from `state`."""
    from marlenv.dqn import DQNForward
    h, w, c = actor.cfg.height, actor.cfg.width, actor.cfg.channels
    A = actor.num_actions
    PC.assert_equal_bits(PC.packed_bits(actor), PC.truth(state, actor.plan, h, w, c, A), what)
    ref = DQNForward(state, h, w, c, num_actions=A, device=DEV, plan=actor.plan, conv_waves=actor.cfg.conv_waves)
    q, want = actor(obs), ref(obs)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    assert torch.equal(q, want), what
    return q


def batch8():
    state, batch = LC.descent_batch(8)
    return state, tuple(t.to(DEV) for t in batch)


def test_actor_follows_the_policy_net():
    state, batch = batch8()
    obs = P.probe_obs(70, 5, 5, 8, 3).to(DEV)
    learner = make_learner(state, 5, 5, 8)
    actor = learner.actor()
    assert actor.plan == 'window' and actor.precision == 'bf16'
    q0 = follows(actor, learner.state_dict(), obs, 'fresh')
    for _ in range(3):
        learner.update(*batch)
    q3 = follows(actor, learner.state_dict(), obs, 'after three updates')
    assert not torch.equal(q0, q3)
    # a checkpoint round trip, and a checkpoint of other weights
    learner.load_checkpoint(learner.checkpoint())
    assert torch.equal(follows(actor, learner.state_dict(), obs, 'after the round trip'), q3)
    other = make_learner(PC.real_state(5, 5, 8, 3, seed=4, crafted=False), 5, 5, 8)
    learner.load_checkpoint(other.checkpoint())
    q4 = follows(actor, other.state_dict(), obs, 'after another checkpoint')
    assert not torch.equal(q4, q3)
    # the map plan on the same geometry, asked for by name
    follows(learner.actor(plan='map', conv_waves=8), learner.state_dict(), obs, 'map plan')


def test_actor_on_the_full_map():
    state = PC.real_state(20, 20, 8, 3, crafted=False)
    learner = make_learner(state, 20, 20, 8)
    actor = learner.actor()
    assert actor.plan == 'map' and actor.layout.p16 == 416
    follows(actor, learner.state_dict(), P.probe_obs(5, 20, 20, 8, 3).to(DEV), 'full map')


def test_actor_holds_the_crafted_values():
    """Through the learner's own flat buffers, infinities and denormals included."""
    state, want = PC.case('window', 5, 5, 16, 3)
    actor = make_learner(state, 5, 5, 16).actor()
    PC.assert_equal_bits(PC.packed_bits(actor), want)


def test_actor_without_auto_sync_keeps_its_snapshot():
    from marlenv.dqn import DQNForward
    state, batch = batch8()
    obs = P.probe_obs(70, 5, 5, 8, 3).to(DEV)
    learner = make_learner(state, 5, 5, 8)
    actor = learner.actor(auto_sync=False)
    before = actor(obs).clone()
    learner.update(*batch)
    assert torch.equal(actor(obs), before)
    now = DQNForward(learner.state_dict(), 5, 5, 8, device=DEV)(obs)
    assert not torch.equal(before, now)
    actor.sync()
    assert torch.equal(actor(obs), now)
    learner.update(*batch)
    learner.sync_actor(actor)
    follows(actor, learner.state_dict(), obs, 'after sync_actor')
    with pytest.raises(ValueError, match='actor'):
        make_learner(state, 5, 5, 8).sync_actor(actor)
    with pytest.raises(ValueError, match='actor'):
        DQNForward(state, 5, 5, 8, device=DEV).sync()


def test_learner_holds_its_actors_weakly():
    state, batch = batch8()
    learner = make_learner(state, 5, 5, 8)
    a, b = learner.actor(), learner.actor(auto_sync=False)
    assert len(learner._actors) == 1
    del a
    gc.collect()
    assert len(learner._actors) == 0
    learner.update(*batch)
    assert b._source is learner


def snapshot(learner):
    return [t.clone() for t in (learner._param, learner._target, learner._m, learner._v, learner._grad,
                                learner.grad_norm)]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_bf16_target():
    from marlenv.dqn import DQNForward
    state, batch = batch8()
    s, a, r, ns, d = batch
    obs = P.probe_obs(70, 5, 5, 8, 3).to(DEV)

    def target_ref(learner):
        return DQNForward(learner.target_state_dict(), 5, 5, 8, device=DEV)(obs)

    whole, by_hand, again = (make_learner(state, 5, 5, 8, target_precision='bf16') for _ in range(3))
    assert whole.target_precision == 'bf16'
    assert torch.equal(whole.target_q(obs), target_ref(whole))
    fp32 = make_learner(state, 5, 5, 8)
    assert fp32.target_precision == 'fp32' and not torch.equal(fp32.target_q(obs), whole.target_q(obs))
    losses, hand_losses = [], []
    for i in range(3):
        losses.append(whole.update(*batch))
        nq = by_hand.target_q(ns)
        q = by_hand(s)
        loss, dq = by_hand.td_loss(q, a, r, d, nq)
        by_hand.backward(s, dq)
        by_hand.apply()
        hand_losses.append(loss)
    assert same(snapshot(whole), snapshot(by_hand)) and same(losses, hand_losses)
    assert same(losses, [again.update(*batch) for _ in range(3)]) and same(snapshot(whole), snapshot(again))
    # the target net did not move with the policy; sync_target moves it
    t0 = whole.target_q(obs)
    assert torch.equal(t0, target_ref(whole))
    assert torch.equal(t0, make_learner(state, 5, 5, 8, target_precision='bf16').target_q(obs))
    whole.sync_target()
    t1 = whole.target_q(obs)
    assert not torch.equal(t0, t1) and torch.equal(t1, target_ref(whole))
    assert torch.equal(t1, DQNForward(whole.state_dict(), 5, 5, 8, device=DEV)(obs))
    # the fp32 target buffer and the checkpoint are those of the fp32 mode's layout
    ckpt = whole.checkpoint()
    assert all(torch.equal(ckpt['target_net'][k], v) for k, v in whole.state_dict().items())
    fresh = make_learner(PC.real_state(5, 5, 8, 3, seed=4, crafted=False), 5, 5, 8, target_precision='bf16')
    fresh.load_checkpoint(ckpt)
    assert torch.equal(fresh.target_q(obs), t1)
    with pytest.raises(TypeError):
        whole.target_q(obs.float())


def test_default_learner_is_unchanged_by_an_actor():
    state, batch = batch8()
    plain, acting = make_learner(state, 5, 5, 8), make_learner(state, 5, 5, 8)
    actor = acting.actor()
    l0 = [plain.update(*batch) for _ in range(3)]
    l1 = [acting.update(*batch) for _ in range(3)]
    assert same(l0, l1) and same(snapshot(plain), snapshot(acting))
    sd0, sd1 = plain.state_dict(), acting.state_dict()
    assert all(torch.equal(sd0[k], sd1[k]) for k in sd0)
    assert actor._source is acting


@pytest.mark.parametrize('h,w,c,A,msg', [(40, 40, 8, 3, 'bordered'), (5, 5, 8, 5, 'num_actions'),
                                         (5, 5, 64, 3, 'channels')])
def test_geometries_without_a_bf16_plan(h, w, c, A, msg):
    state = {k: torch.zeros(s) for k, s in PC.shapes(h, w, c, A).items()}
    with pytest.raises(ValueError, match=msg):
        make_learner(state, h, w, c, A, target_precision='bf16')
    learner = make_learner(state, h, w, c, A)        # the fp32 learner takes them all
    with pytest.raises(ValueError, match=msg):
        learner.actor()
    assert len(learner._actors) == 0
    assert learner(torch.zeros((2, h, w, c), dtype=torch.uint8, device=DEV)).shape == (2, A)


def test_collector_acts_through_the_actor():
    """The README's loop: Collector.run(learner.actor(), ...) then update on a sample."""
    from marlenv import Collector, ReplayBuffer, SnakeVecEnv
    env = SnakeVecEnv(16, num_snakes=2, height=10, width=10, vision_range=2, seed=3)
    S, h, w, c = env.obs_shape
    buf = ReplayBuffer(env.obs_shape, 4096)
    torch.manual_seed(5)
    learner = make_learner(LC.TorchDQN(h, w, c, 3).state_dict(), h, w, c, target_precision='bf16')
    actor = learner.actor()
    collector = Collector(env, buf)
    for _ in range(2):
        collector.run(actor, steps=4, epsilon=0.5)
        loss = learner.update(*buf.sample(64))
        assert loss.shape == () and bool(torch.isfinite(loss))
    assert learner.step == 2
    obs = P.probe_obs(6, h, w, c, 1).to(DEV)
    follows(actor, learner.state_dict(), obs, 'after the loop')
