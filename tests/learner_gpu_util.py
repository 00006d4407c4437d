"""What tests/test_learner_gpu.py, tests/test_learner_bf16_gpu.py and
tests/test_learner_fwd16_gpu.py share: the learner on the device, the probe
batch, the bit-equality helpers, and the two checks that every precision option
must pass (update() equals its stages; checkpoints move between an option's
modes). The CPU files of the same names take the id formatters and the `native`
fixture from here."""
import os

import pytest
import torch

import dqn_probe as P
import learner_cases as LC

DEV = 'cuda:0'
KEY5 = (5, 5, 8, 3)


@pytest.fixture(scope='module')
def native():
    from marlenv import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _native


def run_ids(runs):
    return ['%dx%dx%d-A%d-s%d-B%d' % (k[:5] + (b,)) for k, b in runs]


def key_ids(keys):
    return ['%dx%dx%d-A%d-s%d-B%d' % k for k in keys]


def make_learner(state, key, **kw):
    from marlenv import DQNLearner
    h, w, c, A = key[:4]
    return DQNLearner(state, h, w, c, num_actions=A, device=DEV, **kw)


def probe_batch(B=64):
    g = P._gen(B, 31337)
    state, next_state = P.probe_obs(B, 5, 5, 8, 21), P.probe_obs(B, 5, 5, 8, 22)
    action = torch.randint(0, 3, (B,), generator=g)
    reward = torch.randint(-2, 3, (B,), generator=g).float()
    done = (torch.rand(B, generator=g) < 0.25).float()
    return tuple(t.to(DEV) for t in (state, action, reward, next_state, done))


def snapshot(learner):
    return [learner._param.clone(), learner._m.clone(), learner._v.clone(), learner._target.clone()]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def check_update_equals_its_stages(kw, differs_after_first_step=False):
    """Three updates of a learner built with `kw` are bit-equal to their stages
    run by hand and to a rerun from the checkpoint after the first; they are
    another computation than the fp32 learner's, with the same target."""
    state, _ = LC.descent_batch()                                     # real-valued: rounding matters from step 1
    batch = probe_batch()
    s, a, r, ns, d = batch
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
            if differs_after_first_step:
                assert not torch.equal(whole._param, fp32._param)
    assert whole.step == by_hand.step == 3
    assert same(snapshot(whole), snapshot(by_hand))
    assert all(torch.equal(x, y) for x, y in zip(losses, hand_losses))
    assert not torch.equal(whole._param, fp32._param)                  # the bf16 mode is another computation
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


def check_checkpoints_move(option):
    """option: 'backward_precision' or 'forward_precision'."""
    state, _ = LC.descent_batch()
    batch = probe_batch()
    for first, second in (('bf16', 'fp32'), ('fp32', 'bf16')):
        a = make_learner(state, KEY5, **{option: first})
        a.update(*batch)
        ckpt = a.checkpoint()
        b = make_learner(P.probe_net(5, 5, 8, 3, 1), KEY5, **{option: second})
        b.load_checkpoint(ckpt)
        assert getattr(b, option) == second and b.step == 1
        if option == 'forward_precision':
            with pytest.raises(ValueError, match='policy forward'):
                b.pre_activations()
        assert same(snapshot(b), snapshot(a))
        # from the same state, the loaded learner continues as one of its own mode does
        c = make_learner(P.probe_net(5, 5, 8, 3, 1), KEY5, **{option: second})
        c.load_checkpoint(ckpt)
        assert torch.equal(b.update(*batch), c.update(*batch)) and same(snapshot(b), snapshot(c))
        a.update(*batch)
        assert not torch.equal(a._param, b._param)                     # and not as the other mode
