"""The float64 model of the bf16 backward (snake_dqn32_backward_bf16) and the
cases of its tests (no GPU needed here), so that tests/test_learner_bf16_cpu.py
proves exactly what tests/test_learner_bf16_gpu.py relies on.

The model is the backward layer by layer in float64 with bf16 rounding,
t.float().bfloat16().double(), at exactly the points include/snake_env.h names:
both operands of the five weight-gradient GEMMs of the matrix cores (dY, and
act(X) after it is formed) and of the four input-gradient GEMMs (dY and W).
Masks come from the float64 forward; dX is kept unrounded between layers; bias
gradients sum the unrounded dY; fc3's three stages are unrounded.

Cases:
  existing    tests/learner_cases.py's probes: every staged operand is an integer
              of magnitude < 256, which bf16 holds exactly, so the model equals
              the autograd reference and the kernel must equal both.
  rounding    the probe's dq times 29 on three probes: dY grows past 256, where
              odd integers are no bf16 values; everything stays an integer and
              every GEMM's sum of absolute terms below 2^24, so fp32
              accumulation in any order is exact and the kernel must EQUAL the
              model -- which a kernel that rounds elsewhere, or nowhere, does not.
  real        a small random-real net; the kernel differs from the model by
              fp32 accumulation order and rare rounding ties only."""
import functools
import math

import torch

import learner_cases as LC

F = torch.nn.functional
G = torch.nn.grad

CONVS = ('conv1', 'conv2', 'conv3')

ROUNDING_KEYS = ((5, 5, 8, 3, 0, 70), (5, 5, 24, 5, 0, 70), (20, 20, 8, 3, 0, 5))
ROUNDING_SCALE = 29.0
# the dY buffers in which rounding must change at least one entry, per rounding case
ROUNDED_DY = {ROUNDING_KEYS[0]: (1, 2, 3, 4, 5), ROUNDING_KEYS[1]: (1, 2, 3, 4, 5), ROUNDING_KEYS[2]: (1, 2, 3, 4)}


def bf16(t):
    """Round to nearest even to bf16, as a float64 tensor."""
    return t.float().bfloat16().double()


def exact(t):
    return t


def forward_pre(state, obs):
    """The float64 forward: (x NCHW, the five pre-activations Y + b, conv ones NCHW)."""
    s = {k: v.detach().double().cpu() for k, v in state.items()}
    x = LC.input64(obs)
    pre, t = [], x
    for name in CONVS:
        p = F.conv2d(t, s[name + '.weight'], s[name + '.bias'], padding=1)
        pre.append(p)
        t = F.relu(p)
    t = t.reshape(t.size(0), -1)
    for name in ('fc1', 'fc2'):
        p = F.linear(t, s[name + '.weight'], s[name + '.bias'])
        pre.append(p)
        t = F.relu(p)
    return x, pre


def backward_model(state, obs, dq, rnd=bf16):
    """(grads, staged, sum_bound). grads: reference names and layouts. staged:
    every value a matrix-core GEMM stages, BEFORE rounding: 'x', 'c1', 'c2', 'c3',
    'h1' (the activations), 'w:conv2', 'w:conv3', 'w:fc1', 'w:fc2' (the input
    gradients' weights), 'dY1'..'dY5'. sum_bound: the largest sum of absolute
    terms of any output element of any GEMM or bias sum of the chain, on the
    operands as the chain stages them (rounded)."""
    s = {k: v.detach().double().cpu() for k, v in state.items()}
    x, pre = forward_pre(state, obs)
    masks = [(p > 0).double() for p in pre]
    c1, c2, c3, h1, h2 = (F.relu(p) for p in pre)
    B = x.size(0)
    # the observation as conv1's weight gradient stages it: the byte, or byte / 255 in fp32
    xb = obs.cpu().permute(0, 3, 1, 2).float()
    x_in = (xb / 255.0 if float(xb.max()) > 1.0 else xb).double()
    dq = dq.double().cpu()
    grads, staged, bound = {}, {'x': x_in, 'c1': c1, 'c2': c2, 'c3': c3, 'h1': h1}, [0.0]

    def note(v):
        bound[0] = max(bound[0], float(v.max()))

    # fc3: unrounded
    grads['fc3.weight'], grads['fc3.bias'] = dq.t() @ h2, dq.sum(0)
    note(dq.abs().t() @ h2.abs())
    note(dq.abs().sum(0))
    dy = (dq @ s['fc3.weight']) * masks[4]
    note(dq.abs() @ s['fc3.weight'].abs())
    # fc2, fc1
    c3f = c3.reshape(B, -1)
    for name, act, mask, idx in (('fc2', h1, masks[3], 5), ('fc1', c3f, masks[2].reshape(B, -1), 4)):
        staged['dY%d' % idx], staged['w:' + name] = dy, s[name + '.weight']
        r_dy, r_act, r_w = rnd(dy), rnd(act), rnd(s[name + '.weight'])
        grads[name + '.weight'], grads[name + '.bias'] = r_dy.t() @ r_act, dy.sum(0)
        note(r_dy.abs().t() @ r_act.abs())
        note(dy.abs().sum(0))
        note(r_dy.abs() @ r_w.abs())
        dy = (r_dy @ r_w) * mask
    dy = dy.reshape(c3.shape)
    # conv3, conv2, conv1
    for name, act, mask, idx in (('conv3', c2, masks[1], 3), ('conv2', c1, masks[0], 2), ('conv1', x_in, None, 1)):
        w = s[name + '.weight']
        staged['dY%d' % idx] = dy
        r_dy, r_act = rnd(dy), rnd(act)
        grads[name + '.weight'] = G.conv2d_weight(r_act, w.shape, r_dy, padding=1)
        grads[name + '.bias'] = dy.sum((0, 2, 3))
        note(G.conv2d_weight(r_act.abs(), w.shape, r_dy.abs(), padding=1))
        note(dy.abs().sum((0, 2, 3)))
        if mask is not None:
            staged['w:' + name] = w
            r_w = rnd(w)
            note(G.conv2d_input(act.shape, r_w.abs(), r_dy.abs(), padding=1))
            dy = G.conv2d_input(act.shape, r_w, r_dy, padding=1) * mask
    return grads, staged, bound[0]


def ref_grads_bf16(state, obs, dq):
    """The float64 model of snake_dqn32_backward_bf16: the gradients of
    sum(dq * Q(obs)) with bf16 rounding at the header's rounding points;
    reference names and layouts, like learner_cases.ref_grads."""
    return backward_model(state, obs, dq, bf16)[0]


@functools.lru_cache(maxsize=None)
def rounding_case(key):
    """(case, dq * 29, the model's gradients); shared, nobody writes to its tensors."""
    case = LC.backward_case(key)
    dq = (case.dq * ROUNDING_SCALE).contiguous()
    return case, dq, ref_grads_bf16(case.state, case.obs, dq)


# ---- the real-valued case ---------------------------------------------------------
REAL_GEOM = (3, 4, 8, 3)        # h, w, c, A
REAL_B = 6
# The first seed from 0 at which mask_margin() >= MASK_MARGIN holds for the case
# and for its obs * 255 variant (tests/test_learner_bf16_cpu.py asserts it holds).
REAL_SEED = 0
# |Y + b| >= 2e-5 of the layer's max |Y + b|: twice the fp32 forward's documented
# 1e-5 accuracy, so the fp32 forward's masks are the float64 forward's
MASK_MARGIN = 2e-5


def real_case(seed=None, scaled=False):
    """(state, obs, dq): weights uniform in +-1/sqrt(fan_in), Bernoulli bytes
    (times 255 with scaled: the /255 branch), dq normal / B."""
    h, w, c, A = REAL_GEOM
    g = torch.Generator().manual_seed(REAL_SEED if seed is None else seed)
    shapes = (('conv1', (32, c, 3, 3)), ('conv2', (64, 32, 3, 3)), ('conv3', (64, 64, 3, 3)),
              ('fc1', (256, 64 * h * w)), ('fc2', (128, 256)), ('fc3', (A, 128)))
    state = {}
    for name, shape in shapes:
        k = 1.0 / math.sqrt(math.prod(shape[1:]))
        state[name + '.weight'] = (torch.rand(shape, generator=g) * 2 - 1) * k
        state[name + '.bias'] = (torch.rand(shape[0], generator=g) * 2 - 1) * k
    obs = (torch.rand((REAL_B, h, w, c), generator=g) < 0.5).to(torch.uint8)
    dq = torch.randn((REAL_B, A), generator=g) / REAL_B
    if scaled:
        obs = obs * 255
    return state, obs.contiguous(), dq.contiguous()


def mask_margin(state, obs):
    """min over the five ReLU layers of min |Y + b| / max |Y + b| (float64)."""
    _, pre = forward_pre(state, obs)
    return min(float(p.abs().min() / p.abs().max()) for p in pre)


def first_stable_seed(limit=200):
    for seed in range(limit):
        if all(mask_margin(*real_case(seed, sc)[:2]) >= MASK_MARGIN for sc in (False, True)):
            return seed
    raise AssertionError('no seed below %d keeps every unit off its ReLU threshold' % limit)
