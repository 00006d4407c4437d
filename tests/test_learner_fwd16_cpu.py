"""CPU checks of the bf16 forward's tests (no GPU needed): what
tests/test_learner_fwd16_gpu.py's comparisons rest on.

Probes: bf16 holds every staged GEMM operand exactly, so the model of
tests/learner_model.py equals dqn_probe.ref64 and the gradients that
continue from it equal the autograd reference. Rounding cases (conv1 x 61): all
integers, every sum of absolute terms below 2^24, rounding does change operands
and results. Real-valued case: no unit of the model's chain sits close to its
ReLU threshold. The split-K rule, restated, puts the GPU cases on both sides of
it. And the new entry points are exported and validate their arguments like the
fp32 ones, before any launch."""
import ctypes

import pytest
import torch

import dqn_probe as P
import learner16_cases as L16
import learner_cases as LC
import learner_fwd16_cases as FC
import learner_model as M
from learner_gpu_util import key_ids, native, run_ids  # noqa: F401 (native is a fixture)

ALL_RUNS = FC.exact_runs()
RUN_IDS, KEY_IDS = run_ids(ALL_RUNS), key_ids(FC.ROUNDING_KEYS)


@pytest.mark.parametrize('key,B', ALL_RUNS, ids=RUN_IDS)
def test_probes_stage_only_bf16_values(key, B):
    case = LC.backward_case(key, B)
    model = M.forward_model(case.state, case.obs)
    feat, q, acts = P.ref64(case.state, case.obs)
    assert set(model.staged) == set(P.ROUNDED)
    for name, v in model.staged.items():
        assert torch.equal(v, v.round()) and float(v.abs().max()) < 256, name     # integers below 2^8: exact in bf16
        assert torch.equal(M.bf16(v), v), name
    for name in P.LAYERS:
        w = case.state[name + '.weight'].double()
        assert torch.equal(M.bf16(w), w), name
    for i, dst in enumerate(('c1', 'c2', 'c3', 'h1', 'h2')):
        assert torch.equal(torch.relu(model.pre[i]), acts[dst]), dst
    assert torch.equal(model.feat, feat) and torch.equal(model.q, q)
    assert torch.equal(q, P.probe(*key).q[:B])
    assert model.bound < LC.SUM_LIMIT
    for rnd in FC.BACKWARD_RND.values():
        grads, _, bound = M.backward_model(case.state, case.obs, case.dq, rnd, pre=model.pre)
        assert bound < LC.SUM_LIMIT
        for name in LC.PARAMS:
            assert torch.equal(grads[name], case.grads[name]), name


@pytest.mark.parametrize('key', FC.SPLIT_K_KEYS, ids=key_ids(FC.SPLIT_K_KEYS))
def test_split_k_geometries_are_exact_probes(key):
    """The two geometries added for fc1's split K: every activation of the probe
    is a small integer and the largest sum of absolute gradient terms stays
    below 2^24, so the forward and both backwards are exact in any order."""
    case = LC.backward_case(key)
    acts = P.ref64(case.state, case.obs)[2]
    top = max(float(v.max()) for v in acts.values())
    assert all(torch.equal(v, v.round()) and float(v.min()) >= 0 for v in acts.values())
    bound = LC.term_bound(case.state, case.obs, case.dq)
    print('%s: largest activation %g, term bound %g' % (key, top, bound))
    assert (top, bound) == FC.SPLIT_K_FACTS[key] and bound < LC.SUM_LIMIT
    for name in LC.PARAMS:
        assert torch.equal(case.grads[name], case.grads[name].round()), name


@pytest.mark.parametrize('key', FC.FORWARD_ONLY_KEYS, ids=key_ids(FC.FORWARD_ONLY_KEYS))
def test_forward_only_probes_stage_only_bf16_values(key):
    p = P.probe(*key)
    model = M.forward_model(p.state, p.obs)
    for name, v in model.staged.items():
        assert torch.equal(v, v.round()) and float(v.abs().max()) < 256 and torch.equal(M.bf16(v), v), name
    assert torch.equal(model.feat, p.feat) and torch.equal(model.q, p.q) and model.bound < LC.SUM_LIMIT


def test_the_backward_chain_is_learner16_cases_chain():
    """backward_model's default start is the unrounded forward_model's pre-activations,
    those are dqn_probe.ref64's, and learner16_cases' stored gradients are that chain's."""
    case, dq, stored = L16.rounding_case(L16.ROUNDING_KEYS[0])
    pre = M.forward_model(case.state, case.obs, M.exact).pre
    grads, _, bound = M.backward_model(case.state, case.obs, dq)
    given, _, given_bound = M.backward_model(case.state, case.obs, dq, pre=pre)
    assert bound == given_bound
    acts = P.ref64(case.state, case.obs)[2]
    for p, dst in zip(pre, ('c1', 'c2', 'c3', 'h1', 'h2')):
        assert torch.equal(torch.relu(p), acts[dst]) and torch.equal(p > 0, acts[dst] > 0), dst
    for name in LC.PARAMS:
        assert torch.equal(grads[name], given[name]) and torch.equal(grads[name], stored[name]), name


def test_bytes_0_255_case_is_the_0_1_case():
    case = LC.backward_case(FC.BYTES_KEY)
    obs = case.obs * 255
    assert int(obs.max()) == 255
    assert torch.equal(M.staged_input(obs), M.staged_input(case.obs))         # 255 / 255 is 1.0f
    a, b = M.forward_model(case.state, obs), M.forward_model(case.state, case.obs)
    assert torch.equal(a.q, b.q) and all(torch.equal(a.Y[n], b.Y[n]) for n in FC.YS)


@pytest.mark.parametrize('key', FC.ROUNDING_KEYS, ids=KEY_IDS)
def test_rounding_cases_are_exact_and_do_round(key):
    c = FC.rounding_case(key)
    model, unrounded = c.model, c.exact
    # integers everywhere, sums of absolute terms below 2^24: fp32 accumulation in any order is exact
    for name in FC.YS:
        assert torch.equal(model.Y[name], model.Y[name].round()), name
    for name, v in model.staged.items():
        assert torch.equal(v, v.round()), name
    for name, v in c.state.items():
        assert torch.equal(v, v.round()), name
    assert torch.equal(model.q, model.q.round()) and torch.equal(model.feat, model.feat.round())
    print('forward max sum |terms| %.4g, gradients %.4g of 2^24 = %.4g' % (model.bound, c.grad_bound, LC.SUM_LIMIT))
    assert model.bound < LC.SUM_LIMIT and c.grad_bound < LC.SUM_LIMIT
    assert max(float(model.Y[n].abs().max()) for n in FC.YS) <= model.bound
    for mode in FC.BACKWARD_RND:
        for name in LC.PARAMS:
            g = c.grads[mode][name]
            assert torch.equal(g, g.round()) and float(g.abs().max()) <= c.grad_bound, (mode, name)
    # the unrounded model is the float64 forward
    feat, q, _ = P.ref64(c.state, c.obs)
    assert torch.equal(unrounded.q, q) and torch.equal(unrounded.feat, feat)
    # rounding changes entries of c1, c2, c3 and h1 (x and the weights are bf16 values) ...
    changed = {n: int((M.bf16(v) != v).sum()) for n, v in model.staged.items()}
    print('unrepresentable staged entries: %s' % changed)
    assert changed['x'] == 0
    for name in ('c1', 'c2', 'c3', 'h1'):
        assert changed[name] > 0, name
    for name in P.LAYERS:
        w = c.state[name + '.weight'].double()
        assert torch.equal(M.bf16(w), w), name
    # ... so Y1 is the unrounded one, and Y2..Y5 and Q are not
    assert torch.equal(model.Y['Y1'], unrounded.Y['Y1'])
    for name in FC.YS[1:]:
        assert not torch.equal(model.Y[name], unrounded.Y[name]), name
    nq = int((model.q != unrounded.q).sum())
    print('Q entries changed: %d of %d' % (nq, model.q.numel()))
    assert nq > 0
    if key == (5, 5, 8, 3, 0, 70):
        assert changed['c1'] == 91 and nq == 206
    if key == (20, 20, 8, 3, 0, 5):
        assert (changed['c1'], changed['h1'], nq) == (97, 507, 15)


def test_scale_29_would_not_round_conv1s_output():
    """Why the scale is 61: at learner16_cases' 29 every c1 entry stays a bf16 value."""
    case = LC.backward_case(FC.ROUNDING_KEYS[0])
    c1 = M.forward_model(FC.scaled_state(case.state, 29.0), case.obs).staged['c1']
    assert torch.equal(M.bf16(c1), c1)


@pytest.mark.parametrize('scaled', [False, True], ids=['bytes-0-1', 'bytes-0-255'])
def test_real_case_is_stable_on_the_models_chain(scaled):
    state, obs, dq = FC.real_case(scaled)
    assert tuple(obs.shape) == (6, 3, 4, 8) and int(obs.max()) == (255 if scaled else 1)
    margin = M.margin(state, obs, M.bf16)
    print('model chain: min |Y + b| / max |Y + b| = %.3g' % margin)
    assert margin >= L16.MASK_MARGIN
    model, ref = M.forward_model(state, obs), FC.reference_y(state, obs)
    for name in FC.YS:
        rel = float((model.Y[name] - ref[name]).norm() / ref[name].norm())
        print('%s |model - ref64| / |ref64| = %.3g' % (name, rel))
        assert 0 < rel < 2e-2, name                                             # a few bf16 roundings (2^-9 each)
    q64 = P.ref64(state, obs)[1]
    assert 0 < float((model.q - q64).norm() / q64.norm()) < 2e-2


def test_real_seed_is_the_first_stable_one():
    assert L16.first_stable_seed(M.bf16) == FC.REAL_SEED


# ---- the split-K rule ------------------------------------------------------------------
def test_split_k_rule_and_the_cases_on_both_sides_of_it():
    for K in (64, 256, 768, 1024):
        assert FC.split_k_chunks(K) == 1
    assert FC.split_k_chunk(1088) == 1024 and FC.split_k_chunks(1088) == 2
    assert FC.split_k_chunk(25600) == 1600 and FC.split_k_chunks(25600) == 16
    assert FC.split_k_chunk(64 * 255 * 255) % 64 == 0 and FC.split_k_chunks(64 * 255 * 255) == 16
    for K in range(64, 64 * 700, 64):
        c, n = FC.split_k_chunk(K), FC.split_k_chunks(K)
        assert c % 64 == 0 and c >= 1024 and n <= 16 and (n - 1) * c < K <= n * c
    keys = [k for k, _ in ALL_RUNS]
    assert FC.fc1_chunks((1, 1, 8, 3, 0, 70)) == (1, 64) and (1, 1, 8, 3, 0, 70) in keys        # a single chunk
    assert FC.fc1_chunks((4, 33, 8, 3, 0, 65)) == (9, 256) and (4, 33, 8, 3, 0, 65) in keys     # ragged last chunk
    assert FC.fc1_chunks((5, 5, 8, 3, 0, 70)) == (2, 576)
    assert FC.fc1_chunks((20, 20, 8, 3, 0, 5)) == (16, 1600)                                    # the most chunks, even
    assert FC.fc1_chunks(L16.REAL_GEOM) == (1, 768)
    assert FC.split_k_chunk(64 * 17 * 17) == 1216 and FC.fc1_chunks((17, 17, 8, 3, 0, 5)) == (16, 256)    # above the floor, ragged
    assert FC.split_k_chunk(64 * 3 * 11) == 1024 and FC.fc1_chunks((3, 11, 8, 3, 0, 37)) == (3, 64)
    for key in FC.SPLIT_K_KEYS:
        assert key in keys
    for key in FC.ROUNDING_KEYS + (FC.PREFIX_KEY,):
        assert key in keys


# ---- exports and validation ------------------------------------------------------------
def test_exports(native):
    L = native.lib()
    for name in ('snake_dqn32_forward_bf16', 'snake_dqn32_forward_bf16_scratch'):
        assert name in native.EXPORTS and hasattr(L, name)
    assert native.SNAKE_ABI_VERSION == 20 and L.snake_abi_version() == 20
    assert L.snake_dqn32_forward_bf16.argtypes == L.snake_dqn32_forward.argtypes
    assert L.snake_dqn32_forward_bf16_scratch.argtypes == L.snake_dqn32_scratch.argtypes


def call(native, fn, cfg=(5, 5, 8, 3), batch=1, net=0x1000, obs=0x100, scratch=0x3000, q=0x4000, bad_w=None):
    """Both functions validate before any launch, so host-only calls with
    made-up addresses reach every check (none is dereferenced)."""
    L = native.lib()
    c = native.DqnCfg(*cfg, 0) if cfg else None
    wts = [net + 64 * i for i in range(12)]
    if bad_w is not None:
        wts[3] = bad_w
    n = native.Dqn32Net(*wts)
    p = ctypes.c_void_p
    rc = getattr(L, fn)(ctypes.byref(c) if c else None, ctypes.byref(n) if net else None, p(obs), batch, p(scratch),
                        p(q), None, None)
    return rc, L.snake_last_error().decode()


BAD_ARGS = [
    (dict(cfg=None), 'NULL cfg'), (dict(obs=0), 'NULL buffer'), (dict(scratch=0), 'NULL buffer'),
    (dict(q=0), 'NULL buffer'), (dict(net=0), 'NULL buffer'), (dict(bad_w=0), 'NULL buffer'),
    (dict(cfg=(5, 5, 12, 3)), 'channels'), (dict(cfg=(0, 5, 8, 3)), 'observation'),
    (dict(cfg=(5, 256, 8, 3)), 'observation'), (dict(cfg=(5, 5, 8, 65)), 'num_actions'), (dict(batch=-1), 'batch'),
]


@pytest.mark.parametrize('kw,msg', BAD_ARGS, ids=[m + '-' + '-'.join(k) for k, m in BAD_ARGS])
def test_bf16_forward_rejects_what_the_fp32_one_rejects(native, kw, msg):
    rc32, err32 = call(native, 'snake_dqn32_forward', **kw)
    rc16, err16 = call(native, 'snake_dqn32_forward_bf16', **kw)
    assert rc32 < 0 and rc16 == rc32
    assert msg in err16 and msg in err32
    assert err16.replace('snake_dqn32_forward_bf16', 'snake_dqn32_forward') == err32


def test_bf16_forward_of_an_empty_batch_launches_nothing(native):
    assert call(native, 'snake_dqn32_forward_bf16', batch=0)[0] == 0
    assert call(native, 'snake_dqn32_forward', batch=0)[0] == 0


def test_scratch_size(native):
    L = native.lib()
    for geo in ((1, 1, 8, 3), (3, 4, 8, 3), (5, 5, 8, 3), (4, 33, 8, 3), (20, 20, 8, 3), (255, 255, 128, 64)):
        c = native.DqnCfg(*geo, 0)
        last = -1
        for B in (0, 1, 5, 64, 65, 512):
            n16 = L.snake_dqn32_forward_bf16_scratch(ctypes.byref(c), B)
            n32 = L.snake_dqn32_scratch(ctypes.byref(c), B)
            chunks = FC.split_k_chunks(64 * geo[0] * geo[1])
            assert n16 == n32 + (4 * chunks * B * 256 if chunks > 1 else 0) and n16 >= n32 and n16 % 16 == 0
            assert n16 > last or (B == 0 and n16 == 16)
            last = n16
    for bad, msg in (((5, 5, 12, 3), 'channels'), ((0, 5, 8, 3), 'observation'), ((5, 5, 8, 0), 'num_actions')):
        c = native.DqnCfg(*bad, 0)
        rc = L.snake_dqn32_forward_bf16_scratch(ctypes.byref(c), 1)
        assert rc < 0 and rc == L.snake_dqn32_scratch(ctypes.byref(c), 1) and msg in L.snake_last_error().decode()
    assert L.snake_dqn32_forward_bf16_scratch(None, 1) < 0
    c = native.DqnCfg(5, 5, 8, 3, 0)
    assert L.snake_dqn32_forward_bf16_scratch(ctypes.byref(c), -1) == L.snake_dqn32_scratch(ctypes.byref(c), -1) < 0
    assert 'batch' in L.snake_last_error().decode()


def test_learner_rejects_a_precision_before_any_device_work(native):
    from marlenv import DQNLearner
    state = P.probe_net(5, 5, 8, 3, 0)
    for bad in ('fp16', 'BF16', 'mixed', None, 16):
        with pytest.raises(ValueError, match='forward_precision'):
            DQNLearner(state, 5, 5, 8, 3, forward_precision=bad)
    for bad in ('fp16', 'MIXED', None):
        with pytest.raises(ValueError, match='target_precision'):
            DQNLearner(state, 5, 5, 8, 3, target_precision=bad)
    if not torch.cuda.is_available():
        for kw in (dict(forward_precision='fp32'), dict(forward_precision='bf16'), dict(target_precision='mixed'),
                   dict(forward_precision='bf16', target_precision='mixed', backward_precision='bf16')):
            with pytest.raises(RuntimeError, match='HIP device'):       # accepted: the next check is the device
                DQNLearner(state, 5, 5, 8, 3, **kw)
        # 'mixed' takes geometries no bf16 plan accepts
        with pytest.raises(RuntimeError, match='HIP device'):
            DQNLearner(P.probe_net(4, 33, 8, 3, 0), 4, 33, 8, 3, target_precision='mixed')
