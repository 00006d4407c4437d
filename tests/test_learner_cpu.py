"""CPU checks of the learner (no GPU needed): the probes of
tests/learner_cases.py satisfy what the GPU file's exact comparisons rest on
(integer gradients, sums of absolute terms below 2^24, probes that notice a
wrong weight), the dyadic TD case is exact in fp32, torch's own Adam lowers the
loss on the descent batch, and the library's host-side plan calls return the
documented sizes and messages."""
import ctypes

import pytest
import torch

import dqn_probe as P
import learner_cases as LC
from learner_gpu_util import native, run_ids  # noqa: F401 (native is a fixture)

ALL_RUNS = LC.gpu_backward_runs()


@pytest.mark.parametrize('key,B', ALL_RUNS, ids=run_ids(ALL_RUNS))
def test_probe_gradients_are_exact_integers(key, B):
    case = LC.backward_case(key, B)
    for name, g in case.grads.items():
        assert torch.equal(g, g.round()), name
    bound = LC.term_bound(case.state, case.obs, case.dq)
    print('max sum |terms| %.3g' % bound)
    assert bound < LC.SUM_LIMIT / 16          # far below 2^24
    # and the bound does bound: no gradient entry exceeds it
    assert max(float(g.abs().max()) for g in case.grads.values()) <= bound
    if key[:2] != (1, 1):
        for name, g in case.grads.items():
            share = float((g != 0).double().mean())
            floor = 0.5 if B >= 65 else 0.0
            assert share >= floor, (name, share)


def test_case_table_covers_the_paths():
    keys = [k for k, _ in ALL_RUNS]
    m = [b * k[0] * k[1] for k, b in ALL_RUNS]
    assert any(v % 128 and v > 128 and v % 128 < 64 for v in m) and any(v % 128 >= 64 for v in m)
    assert any(P.fp32_conv_on_matrix_cores(*k[:3]) for k in keys)
    assert any(not P.fp32_conv_on_matrix_cores(*k[:3]) and k[1] > 1 for k in keys)
    assert (1, 1, 8, 3, 0, 70) in keys and (20, 20, 8, 3, 0, 5) in keys and (5, 5, 64, 3, 0, 70) in keys
    # the split-M case of the table's comment: at least three chunks, the last ragged
    M = 65 * 4 * 33
    chunk = LC.chunk_rows(M)
    assert chunk == 2048 and -(-M // chunk) == 5 and M % chunk == 388 and 388 % 16
    assert LC.chunk_rows(512 * 400) == 2048 and LC.chunk_rows(16384 * 400) == 51200


def test_probes_notice_a_wrong_weight():
    """Flipping one weight of any layer changes the reference gradients."""
    case = LC.backward_case((5, 5, 8, 3, 0, 70))
    for layer in ('conv1', 'conv2', 'conv3', 'fc1', 'fc2', 'fc3'):
        state = {k: v.clone() for k, v in case.state.items()}
        w = state[layer + '.weight'].view(-1)
        i = int(w.abs().argmax())
        w[i] = -w[i]
        got = LC.ref_grads(state, case.obs, case.dq)
        assert any(not torch.equal(got[n], case.grads[n]) for n in LC.PARAMS), layer


def test_td_dyadic_case_is_exact_in_fp32():
    q, action, reward, done, next_q = LC.td_dyadic_case(64)
    loss, dq, d = LC.td_ref64(q, action, reward, done, next_q, 0.5)
    assert torch.equal(d * 2, (d * 2).round())                       # multiples of 1/2
    assert d[0] == 1.0 and d[1] == -1.0 and d[2] == 0.5 and d[3] == 0.0
    assert done[1] == 1.0 and done[3] == 1.0 and (done == 0).any()
    assert (d.abs() > 1).any() and ((d.abs() < 1) & (d != 0)).any()  # both branches of smooth-L1
    per_row = torch.where(d.abs() < 1.0, 0.5 * d * d, d.abs() - 0.5)
    assert torch.equal(per_row * 8, (per_row * 8).round())           # multiples of 1/8
    assert float(per_row.sum()) * 8 < 2 ** 24                        # any fp32 summation order is exact
    assert float(d.abs().max()) * 2 < 2 ** 24
    assert torch.equal(dq.float().double(), dq) and float(loss) == float(loss.float())
    # a single row
    q1, a1, r1, d1, n1 = (t[:1] for t in LC.td_dyadic_case(64))
    loss1, dq1, dd = LC.td_ref64(q1, a1, r1, d1, n1, 0.5)
    assert float(dd[0]) == 1.0 and float(loss1) == 0.5 and float(dq1[0, a1[0]]) == 1.0


def test_td_real_case_covers_both_branches():
    q, action, reward, done, next_q = LC.td_real_case(70)
    _, _, d = LC.td_ref64(q, action, reward, done, next_q, 0.99)
    assert (d.abs() > 1).sum() >= 5 and (d.abs() < 1).sum() >= 5 and done.sum() >= 5
    loss_bound, dq_bound = LC.td_bounds(q, action, reward, done, next_q, 0.99)
    assert 0 < loss_bound < 1e-5 and float(dq_bound.max()) < 1e-6


def test_adam_reference_and_bounds():
    g = torch.zeros(8)
    p = torch.arange(8.0)
    out, m, v, norm, S = LC.adam_ref64(p, g, g, g, 1, 5e-4, 0.9, 0.999, 1e-8, 10.0)
    assert torch.equal(out, p.double()) and norm == 0.0              # zero gradients leave p alone
    g = torch.full((8,), 100.0)
    out, m, v, norm, S = LC.adam_ref64(p, g, torch.zeros(8), torch.zeros(8), 1, 5e-4, 0.9, 0.999, 1e-8, 10.0)
    assert abs(norm - 800 ** 0.5 * 10) < 1e-9
    assert torch.allclose(p.double() - out, torch.full((8,), 5e-4, dtype=torch.float64), rtol=1e-6)   # first step: lr
    e_n, K = LC.adam_bounds(5000)
    assert LC.norm_depth(5000) == 4 + 8 + 1 + 8 and K < 64


def test_torch_adam_lowers_the_loss_on_the_descent_batch():
    state, batch = LC.descent_batch()
    policy, target = LC.TorchDQN(5, 5, 8, 3), LC.TorchDQN(5, 5, 8, 3)
    policy.load_state_dict(state)
    target.load_state_dict(state)
    opt = torch.optim.Adam(policy.parameters(), lr=5e-4)
    losses = [float(LC.torch_update(policy, target, opt, batch)) for _ in range(20)]
    print(losses[0], losses[-1])
    assert losses[-1] < losses[0]


def scratch(native, fn, h, w, c, A, B):
    cfg = native.DqnCfg(h, w, c, A, 0)
    n = getattr(native.lib(), fn)(ctypes.byref(cfg), B)
    return n, native.lib().snake_last_error().decode()


def test_train_scratch_sizes(native):
    f = 'snake_dqn32_train_scratch'
    # dY5 | dY4 | dY3 | dY2 | dY1, then the partials: 4 floats when nothing is split, 256 bias floats per chunk
    assert scratch(native, f, 5, 5, 8, 3, 0)[0] == 4 * (4 + 256)
    B, P_ = 70, 25
    assert scratch(native, f, 5, 5, 8, 3, B)[0] == 4 * (B * (128 + 256) + B * P_ * (64 + 64 + 32) + 4 + 256)
    # 65 * 132 rows: five chunks of conv3's 64 x 576 partial
    B, P_ = 65, 132
    assert scratch(native, f, 4, 33, 8, 3, B)[0] == 4 * (B * 384 + B * P_ * 160 + 5 * 64 * 576 + 5 * 256)
    # the reference's Config at B = 512: 100 chunks
    B, P_ = 512, 400
    assert scratch(native, f, 20, 20, 8, 3, B)[0] == 4 * (B * 384 + B * P_ * 160 + 100 * 64 * 576 + 100 * 256)
    for h, w, c, A, B, _ in P.FP32_CASES:                                # every geometry of the forward
        assert scratch(native, f, h, w, c, A, B)[0] > 0


@pytest.mark.parametrize('fn', ['snake_dqn32_scratch', 'snake_dqn32_train_scratch'])
@pytest.mark.parametrize('args,rc,msg', [
    ((0, 5, 8, 3, 1), -1, 'observation'), ((5, 256, 8, 3, 1), -1, 'observation'), ((5, 5, 12, 3, 1), -1, 'channels'),
    ((5, 5, 136, 3, 1), -1, 'channels'), ((5, 5, 8, 0, 1), -1, 'num_actions'), ((5, 5, 8, 65, 1), -1, 'num_actions'),
    ((5, 5, 8, 3, -1), -2, 'batch'),
])
def test_plan_functions_reject(native, fn, args, rc, msg):
    n, err = scratch(native, fn, *args)
    assert n == rc and msg in err
    if rc == -1:
        with pytest.raises(ValueError):
            native.check(int(n))


def test_learner_rejects_a_config_before_any_device_work(native):
    from marlenv import DQNLearner
    state = P.probe_net(5, 5, 8, 3, 0)
    with pytest.raises(ValueError, match='channels'):
        DQNLearner(state, 5, 5, 12, 3)
    with pytest.raises(ValueError, match='num_actions'):
        DQNLearner(state, 5, 5, 8, 65)
    with pytest.raises(ValueError, match='fc1.weight'):
        DQNLearner(state, 5, 6, 8, 3)
    with pytest.raises(ValueError, match='lr'):
        DQNLearner(state, 5, 5, 8, 3, lr=0.0)


def test_layout_round_trip():
    from marlenv.learner import FIELDS, NAMES, from_kernel, kernel_shapes, to_kernel
    assert NAMES[0] == 'conv1.weight' and NAMES[6] == 'conv1.bias' and len(FIELDS) == 12
    state = P.probe_net(3, 4, 8, 3, 0)
    for name, shape in zip(NAMES, kernel_shapes(12, 8, 3)):
        k = to_kernel(name, state[name], 12)
        assert tuple(k.shape) == shape
        assert torch.equal(from_kernel(name, k.contiguous(), 12), state[name])
    # fc1: kernel column p*64 + ch is the reference's ch*P + p
    k = to_kernel('fc1.weight', state['fc1.weight'], 12)
    assert k[7, 5 * 64 + 9] == state['fc1.weight'][7, 9 * 12 + 5]


def test_exports(native):
    new = ('snake_dqn32_train_scratch', 'snake_dqn32_backward', 'snake_dqn_td_loss', 'snake_adam_step')
    L = native.lib()
    for n in new:
        assert n in native.EXPORTS and hasattr(L, n)
    assert native.SNAKE_ABI_VERSION == 20 and L.snake_abi_version() == 20
    import marlenv
    assert marlenv.DQNLearner.__name__ == 'DQNLearner'
