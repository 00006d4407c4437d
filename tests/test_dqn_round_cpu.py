"""CPU checks of the fused bf16 forward's rounding cases (no GPU needed): what
tests/test_dqn_round_gpu.py's comparisons rest on. They are conditions on the
cases of tests/dqn_round_cases.py, not on the kernels.

Rounding and byte cases: all integers; every sum of absolute terms, and every
Y + b, below 2^24, so fp32 accumulation in any order is exact and a kernel that
rounds where the model rounds must EQUAL it; the weights are bf16 values, so a
difference is activation rounding; rounding does change c1, c2, c3, h1 and most
rows of Q. Sharpness: each wrong way to round that
tests/test_dqn.py's tolerance lets through -- truncation, ties rounded up, no
rounding, one rounding point missed, one added before fc3 -- gives another Q on
these cases, so the GPU comparison bites. Real-valued case: no unit of either
chain sits close to its ReLU threshold."""
import pytest
import torch

import dqn_probe as P
import dqn_round_cases as RC
import learner16_cases as L16
import learner_model as M
from learner_gpu_util import key_ids

F = torch.nn.functional

BYTE_KEYS = tuple(k for k, _ in RC.BYTE_CASES)


def integers(model, state):
    for name, v in list(model.staged.items()) + list(model.Y.items()) + [('feat', model.feat), ('q', model.q)]:
        assert torch.equal(v, v.round()), name
    for name, v in state.items():
        assert torch.equal(v.double(), v.double().round()), name


def exact_in_fp32(model):
    """Every GEMM's sum of absolute terms, and every Y + b, is below 2^24."""
    top = max(float(p.abs().max()) for p in model.pre)
    print('max sum |terms| %.4g, max |Y + b| %.4g of 2^24 = %.4g' % (model.bound, top, RC.SUM_LIMIT))
    assert model.bound < RC.SUM_LIMIT and top < RC.SUM_LIMIT
    assert max(float(y.abs().max()) for y in model.Y.values()) <= model.bound


def weights_are_bf16(state):
    for name in P.LAYERS:
        w = state[name + '.weight'].double()
        assert torch.equal(M.bf16(w), w), name


def rounding_happens(model, unrounded, B):
    changed = {n: int((M.bf16(v) != v).sum()) for n, v in model.staged.items()}
    rows = int((model.q != unrounded.q).any(1).sum())
    print('unrepresentable staged entries: %s; rows of Q changed: %d of %d' % (changed, rows, B))
    assert changed['x'] == 0
    for name in ('c1', 'c2', 'c3', 'h1'):
        assert changed[name] > 0, name
    assert 2 * rows > B
    return changed


@pytest.mark.parametrize('key', RC.ROUNDING_KEYS, ids=key_ids(RC.ROUNDING_KEYS))
def test_rounding_cases_are_exact_and_do_round(key):
    c = RC.rounding_case(key)
    assert tuple(c.obs.shape) == (key[5],) + key[:3] and int(c.obs.max()) == 1
    integers(c.model, c.state)
    exact_in_fp32(c.model)
    exact_in_fp32(c.exact)
    weights_are_bf16(c.state)
    # the unrounded chain is the float64 forward
    feat, q, _ = P.ref64(c.state, c.obs)
    assert torch.equal(c.exact.q, q) and torch.equal(c.exact.feat, feat)
    rounding_happens(c.model, c.exact, key[5])
    # and exact ties (257 -> 256, 259 -> 260) are among what is rounded, at every rounding point
    ties = {n: int(((truncate(v) != v) & (truncate(v) + half_up(v) == 2 * v)).sum())
            for n, v in c.model.staged.items() if n != 'x'}
    print('exact ties: %s' % ties)
    assert all(n > 0 for n in ties.values())


# ---- sharpness ---------------------------------------------------------------------------
def bits(t):
    return t.float().view(torch.int32).to(torch.int64) & 0xffffffff


def from_bits(u):
    v = (u & 0xffff) << 16
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32).view(torch.float32).double()


def truncate(t):
    return from_bits(bits(t) >> 16)


def half_up(t):
    return from_bits((bits(t) + 0x8000) >> 16)


def nearest_even(t):
    u = bits(t)
    return from_bits((u + 0x7fff + ((u >> 16) & 1)) >> 16)


def chain(state, x, rnd, feat_rnd=M.exact):
    """Q of the forward with rnd[name] applied to the staged tensor of that name
    ('c1', 'c2', 'c3', 'h1'; the input and the weights are bf16 values) and
    feat_rnd to the features. This file's own: the wrong chains live here only."""
    s = {k: v.detach().double().cpu() for k, v in state.items()}
    t = x
    for i, (name, act) in enumerate(zip(P.LAYERS, P.ROUNDED)):
        if name == 'fc1':
            t = t.reshape(t.size(0), -1)
        t = rnd.get(act, M.exact)(t)
        op = (lambda a, w, b: F.conv2d(a, w, b, padding=1)) if i < 3 else F.linear
        t = F.relu(op(t, s[name + '.weight'], s[name + '.bias']))
    return F.linear(feat_rnd(t), s['fc3.weight'], s['fc3.bias'])


ACTS = ('c1', 'c2', 'c3', 'h1')


def everywhere(fn):
    return {n: fn for n in ACTS}


def wrong_chains():
    """name -> (rnd, feat_rnd)"""
    out = {'truncation': (everywhere(truncate), M.exact), 'ties up': (everywhere(half_up), M.exact),
           'no rounding': ({}, M.exact), 'features rounded': (everywhere(M.bf16), M.bf16)}
    for skip in ACTS:
        out['no rounding at ' + skip] = ({n: M.bf16 for n in ACTS if n != skip}, M.exact)
    out['ties up at h1 alone'] = (dict(everywhere(M.bf16), h1=half_up), M.exact)
    out['truncation at c3 alone'] = (dict(everywhere(M.bf16), c3=truncate), M.exact)
    return out


def test_the_bit_formulas_are_what_their_names_say():
    v = torch.tensor([255.0, 256.0, 257.0, 258.0, 259.0, 261.0, 511.0, 513.0, 514.0, 515.0, 0.0, 3.0]).double()
    assert torch.equal(nearest_even(v), M.bf16(v))
    assert nearest_even(v).tolist() == [255.0, 256.0, 256.0, 258.0, 260.0, 260.0, 512.0, 512.0, 512.0, 516.0, 0.0, 3.0]
    assert truncate(v).tolist() == [255.0, 256.0, 256.0, 258.0, 258.0, 260.0, 510.0, 512.0, 512.0, 512.0, 0.0, 3.0]
    assert half_up(v).tolist() == [255.0, 256.0, 258.0, 258.0, 260.0, 262.0, 512.0, 512.0, 516.0, 516.0, 0.0, 3.0]
    g = P._gen(16, 0)
    r = torch.randn(4096, generator=g).double() * 1000.0
    assert torch.equal(nearest_even(r), M.bf16(r))


@pytest.mark.parametrize('key', RC.ROUNDING_KEYS, ids=key_ids(RC.ROUNDING_KEYS))
def test_every_wrong_rounding_changes_q(key):
    c = RC.rounding_case(key)
    x = M.staged_input(c.obs)
    assert torch.equal(chain(c.state, x, everywhere(M.bf16)), c.model.q)       # the local forward is the model's
    assert torch.equal(chain(c.state, x, everywhere(nearest_even)), c.model.q)
    rows = {}
    for name, (rnd, feat_rnd) in wrong_chains().items():
        rows[name] = int((chain(c.state, x, rnd, feat_rnd) != c.model.q).any(1).sum())
    print('rows of Q (of %d) that differ from the model: %s' % (key[5], rows))
    for name, n in rows.items():
        assert n >= 1, name


# ---- the byte cases ------------------------------------------------------------------------
@pytest.mark.parametrize('key', BYTE_KEYS, ids=key_ids(BYTE_KEYS))
def test_byte_cases_are_exact_and_do_round(key):
    c = RC.byte_case(key)
    p = P.probe(*key)
    assert torch.equal(c.obs != 0, p.obs != 0) and int(c.obs.max()) == 255
    assert sorted(set(c.obs.unique().tolist())) == [0] + list(RC.BYTE_VALUES)
    # the staged input is the byte, not byte / 255
    assert torch.equal(c.model.staged['x'], c.obs.permute(0, 3, 1, 2).double())
    assert float(c.model.staged['x'].max()) == 255.0
    assert not torch.equal(c.model.staged['x'], M.staged_input(c.obs))
    assert all(torch.equal(v, p.state[k]) for k, v in c.state.items())          # the unscaled net
    integers(c.model, c.state)
    exact_in_fp32(c.model)
    exact_in_fp32(c.exact)
    weights_are_bf16(c.state)
    rounding_happens(c.model, c.exact, key[5])
    # and a forward that divided by 255 would not give the model's Q
    assert not torch.equal(M.forward_model(c.state, c.obs).q, c.model.q)


def test_the_staged_input_argument_leaves_the_default_alone():
    c = RC.rounding_case(RC.WINDOW_KEYS[0])
    given = M.forward_model(c.state, c.obs, x=M.staged_input(c.obs))
    assert torch.equal(given.q, c.model.q) and torch.equal(given.feat, c.model.feat)
    assert torch.equal(M.byte_input(c.obs), M.staged_input(c.obs))              # 0/1 bytes


# ---- the learner cases and the real-valued case ------------------------------------------------
def test_learner_keys_are_the_learner_forwards_rounding_keys():
    import learner_fwd16_cases as FC
    for key, _ in RC.LEARNER_KEYS:
        assert key in FC.ROUNDING_KEYS
        c = FC.rounding_case(key)
        assert torch.equal(M.forward_model(c.state, c.obs, x=M.byte_input(c.obs)).q, c.model.q)


def test_real_case_is_stable_on_both_chains():
    assert RC.first_stable_seed() == RC.REAL_SEED
    state, obs = RC.real_case()
    assert tuple(obs.shape) == (6, 5, 5, 8) and int(obs.max()) == 1
    for name, rnd in (('bf16', M.bf16), ('unrounded', M.exact)):
        margin = M.margin(state, obs, rnd)
        print('%s chain: min |Y + b| / max |Y + b| = %.3g' % (name, margin))
        assert margin >= L16.MASK_MARGIN
    model = M.forward_model(state, obs)
    feat64, q64, _ = P.ref64(state, obs)
    for name, mod, ref in (('Q', model.q, q64), ('features', model.feat, feat64)):
        rel = float((mod - ref).norm() / ref.norm())
        print('%s |model - ref64| / |ref64| = %.3g' % (name, rel))
        assert 0 < rel < 2e-2                                                   # a few bf16 roundings (2^-9 each)


def test_learner16_real_case_default_geometry_is_unchanged():
    a, b = L16.real_case(), L16.real_case(geom=L16.REAL_GEOM)
    assert all(torch.equal(a[0][k], b[0][k]) for k in a[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert tuple(a[1].shape) == (L16.REAL_B,) + L16.REAL_GEOM[:3]
