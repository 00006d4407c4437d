"""The float64 model of the bf16 mixed-precision forward
(snake_dqn32_forward_bf16) and the cases of its tests (no GPU needed here), so
that tests/test_learner_fwd16_cpu.py proves exactly what
tests/test_learner_fwd16_gpu.py relies on.

The model is the forward layer by layer in float64 with bf16 rounding,
t.float().bfloat16().double(), applied to act(X) and W at the five GEMMs of the
matrix cores (conv1, conv2, conv3, fc1, fc2) and nowhere else, as
include/snake_env.h states: act(X) is the byte (or byte / 255 in fp32 when the
batch holds a value > 1) or relu(Y_prev + b_prev); Y as stored, the biases, fc3
and the features are not rounded. backward_from() continues from the model's Y
(masks and act(X) are the model's) with tests/learner16_cases.py's rounding
points for the bf16 backward, or none for the fp32 one.

Cases:
  probes      tests/learner_cases.py's integer probes: every staged value is an
              integer below 256, so the model equals dqn_probe.ref64 and the
              kernel must equal both.
  0/255       one probe with obs * 255: 255 / 255 is exactly 1.0f, so the flag
              path must reproduce the 0/1 run.
  rounding    conv1's weight and bias times 61 on four probes: c1 grows past 256,
              where odd integers are no bf16 values; everything stays an integer
              and every sum of absolute terms below 2^24, so the kernel must
              EQUAL the model -- which a kernel that rounds elsewhere, or
              nowhere, does not.
  real        a small random-real net: the kernel differs from the model by fp32
              summation order and rare rounding ties only."""
import functools

import torch

import dqn_probe as P
import learner16_cases as L16
import learner_cases as LC

F = torch.nn.functional
G = torch.nn.grad

YS = ('Y1', 'Y2', 'Y3', 'Y4', 'Y5')
bf16, exact = L16.bf16, L16.exact

BYTES_KEY = (5, 5, 8, 3, 0, 70)
ROUNDING_KEYS = ((5, 5, 8, 3, 0, 70), (5, 5, 24, 5, 0, 70), (20, 20, 8, 3, 0, 5), (4, 33, 8, 3, 0, 65))
ROUNDING_SCALE = 61.0
PREFIX_KEY, PREFIX_B = (5, 5, 8, 3, 1, 129), (1, 127, 129)


# ---- the split-K rule of the dense layers (include/snake_env.h) ---------------------
def split_k_chunk(K):
    return max(1024, -(-(-(-K // 16)) // 64) * 64)


def split_k_chunks(K):
    return -(-K // split_k_chunk(K))


def fc1_chunks(key):
    """(chunks, steps of the last chunk) of fc1 at a case's geometry."""
    K = 64 * key[0] * key[1]
    n = split_k_chunks(K)
    return n, K - (n - 1) * split_k_chunk(K)


# ---- the forward model ------------------------------------------------------------------
def staged_input(obs):
    """conv1's act(X) as the kernels form it: the byte, or byte / 255 in fp32; NCHW float64."""
    xb = obs.cpu().permute(0, 3, 1, 2).float()
    return (xb / 255.0 if float(xb.max()) > 1.0 else xb).double()


class Forward:
    """Y: {'Y1'..'Y5'} pre-activations WITHOUT bias in the scratch's layouts (NHWC);
    pre: the five Y + b (conv ones NCHW); feat, q; staged: 'x', 'c1', 'c2', 'c3',
    'h1' before rounding; bound: the largest sum of absolute terms of any output
    of any of the six GEMMs, on the operands as staged."""


def forward_model(state, obs, rnd=bf16):
    s = {k: v.detach().double().cpu() for k, v in state.items()}
    out = Forward()
    out.Y, out.pre, out.staged, out.bound = {}, [], {}, 0.0
    t = staged_input(obs)
    for i, (name, act_name) in enumerate(zip(P.LAYERS, P.ROUNDED)):
        w, b = s[name + '.weight'], s[name + '.bias']
        if name == 'fc1':
            t = t.reshape(t.size(0), -1)
        out.staged[act_name] = t
        ra, rw = rnd(t), rnd(w)
        if i < 3:
            y = F.conv2d(ra, rw, padding=1)
            top = F.conv2d(ra.abs(), rw.abs(), padding=1)
            out.Y[YS[i]] = y.permute(0, 2, 3, 1).contiguous()
            pre = y + b[None, :, None, None]
        else:
            y = F.linear(ra, rw)
            top = F.linear(ra.abs(), rw.abs())
            out.Y[YS[i]] = y
            pre = y + b
        out.bound = max(out.bound, float(top.max()))
        out.pre.append(pre)
        t = F.relu(pre)
    out.feat = t
    out.q = F.linear(t, s['fc3.weight'], s['fc3.bias'])
    out.bound = max(out.bound, float(F.linear(t.abs(), s['fc3.weight'].abs()).max()))
    return out


def backward_from(state, obs, pre, dq, rnd=bf16):
    """(grads, sum_bound): learner16_cases.backward_model's chain -- the same
    stages and rounding points (rnd=bf16: snake_dqn32_backward_bf16; rnd=exact:
    snake_dqn32_backward) -- continued from given pre-activations `pre`."""
    s = {k: v.detach().double().cpu() for k, v in state.items()}
    masks = [(p > 0).double() for p in pre]
    c1, c2, c3, h1, h2 = (F.relu(p) for p in pre)
    x_in, B = staged_input(obs), pre[0].size(0)
    dq = dq.double().cpu()
    grads, bound = {}, [0.0]

    def note(v):
        bound[0] = max(bound[0], float(v.max()))

    grads['fc3.weight'], grads['fc3.bias'] = dq.t() @ h2, dq.sum(0)
    note(dq.abs().t() @ h2.abs())
    note(dq.abs().sum(0))
    dy = (dq @ s['fc3.weight']) * masks[4]
    note(dq.abs() @ s['fc3.weight'].abs())
    for name, act, mask in (('fc2', h1, masks[3]), ('fc1', c3.reshape(B, -1), masks[2].reshape(B, -1))):
        r_dy, r_act, r_w = rnd(dy), rnd(act), rnd(s[name + '.weight'])
        grads[name + '.weight'], grads[name + '.bias'] = r_dy.t() @ r_act, dy.sum(0)
        note(r_dy.abs().t() @ r_act.abs())
        note(dy.abs().sum(0))
        note(r_dy.abs() @ r_w.abs())
        dy = (r_dy @ r_w) * mask
    dy = dy.reshape(c3.shape)
    for name, act, mask in (('conv3', c2, masks[1]), ('conv2', c1, masks[0]), ('conv1', x_in, None)):
        w = s[name + '.weight']
        r_dy, r_act = rnd(dy), rnd(act)
        grads[name + '.weight'] = G.conv2d_weight(r_act, w.shape, r_dy, padding=1)
        grads[name + '.bias'] = dy.sum((0, 2, 3))
        note(G.conv2d_weight(r_act.abs(), w.shape, r_dy.abs(), padding=1))
        note(dy.abs().sum((0, 2, 3)))
        if mask is not None:
            r_w = rnd(w)
            note(G.conv2d_input(act.shape, r_w.abs(), r_dy.abs(), padding=1))
            dy = G.conv2d_input(act.shape, r_w, r_dy, padding=1) * mask
    return grads, bound[0]


BACKWARD_RND = {'fp32': exact, 'bf16': bf16}


def reference_y(state, obs):
    """{'Y1'..'Y5'} of the unrounded float64 forward, in the scratch's layouts."""
    return forward_model(state, obs, exact).Y


# ---- the rounding cases ------------------------------------------------------------------
def scaled_state(state, scale=ROUNDING_SCALE):
    out = dict(state)
    out['conv1.weight'], out['conv1.bias'] = state['conv1.weight'] * scale, state['conv1.bias'] * scale
    return out


class RoundingCase:
    def __init__(self, key):
        case = LC.backward_case(key)
        self.key, self.obs, self.dq = key, case.obs, case.dq
        self.state = scaled_state(case.state)
        self.model = forward_model(self.state, self.obs)
        self.exact = forward_model(self.state, self.obs, exact)
        self.grads, self.grad_bound = {}, 0.0
        for mode, rnd in BACKWARD_RND.items():
            self.grads[mode], b = backward_from(self.state, self.obs, self.model.pre, self.dq, rnd)
            self.grad_bound = max(self.grad_bound, b)


@functools.lru_cache(maxsize=None)
def rounding_case(key):
    """Shared between the tests of a session; nobody writes to its tensors."""
    return RoundingCase(key)


# ---- the real-valued case ----------------------------------------------------------------
# The first seed from 0 at which every unit of the MODEL's chain (and of its
# obs * 255 variant) is MASK_MARGIN of its layer's scale away from its ReLU
# threshold (tests/test_learner_fwd16_cpu.py asserts it): the kernel's masks and
# the next layer's zeros are then the model's.
REAL_SEED = 2


def model_margin(state, obs):
    """min over the five ReLU layers of min |Y + b| / max |Y + b| on the model's chain."""
    return min(float(p.abs().min() / p.abs().max()) for p in forward_model(state, obs).pre)


def first_stable_seed(limit=200):
    for seed in range(limit):
        if all(model_margin(*L16.real_case(seed, sc)[:2]) >= L16.MASK_MARGIN for sc in (False, True)):
            return seed
    raise AssertionError('no seed below %d keeps every unit off its ReLU threshold' % limit)


def real_case(scaled=False):
    return L16.real_case(REAL_SEED, scaled)
