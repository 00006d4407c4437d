"""The float64 model of where the learner's kernels round (no GPU needed here):
the one place in tests/ that states the rounding points include/snake_env.h
names. tests/learner16_cases.py and tests/learner_fwd16_cases.py hold the cases
that run on it.

Everything is float64, layer by layer, with rnd(t) applied to a value where a
kernel stages it for a GEMM of the matrix cores: rnd=bf16 is
t.float().bfloat16().double(), the bf16 kernels (snake_dqn32_forward_bf16,
snake_dqn32_backward_bf16); rnd=exact rounds nowhere, the fp32 kernels.

Forward: act(X) and W of the five GEMMs conv1, conv2, conv3, fc1, fc2, and
nowhere else: act(X) is the byte (or byte / 255 in fp32 when the batch holds a
value > 1) or relu(Y_prev + b_prev); Y as stored, the biases, fc3 and the
features are not rounded. The fused bf16 forward (dqn_kernels.hip: snake_dqn_forward,
snake_dqn_map_forward) rounds at the same points, as it stores relu(Y + b), and
reads a byte at its value (forward_model's x = byte_input(obs));
tests/dqn_round_cases.py holds its cases.

Backward: both operands of the five weight-gradient GEMMs (dY, and act(X) after
it is formed) and of the four input-gradient GEMMs (dY and W). Masks and act(X)
come from the pre-activations it is given (the unrounded forward's by default);
dX is kept unrounded between layers; bias gradients sum the unrounded dY; fc3's
three stages are unrounded.

dqn_probe.ref64 and learner_cases.forward64 / ref_grads / term_bound are NOT
built on this file: they are the independent references the CPU tests compare
it against."""
import torch

import dqn_probe as P

F = torch.nn.functional
G = torch.nn.grad

YS = ('Y1', 'Y2', 'Y3', 'Y4', 'Y5')


def bf16(t):
    """Round to nearest even to bf16, as a float64 tensor."""
    return t.float().bfloat16().double()


def exact(t):
    return t


def staged_input(obs):
    """conv1's act(X) as the kernels form it: the byte, or byte / 255 in fp32; NCHW float64.
    Deliberately not learner_cases.input64, which divides in float64: that one
    belongs to the autograd reference, which stays independent of this model."""
    xb = obs.cpu().permute(0, 3, 1, 2).float()
    return (xb / 255.0 if float(xb.max()) > 1.0 else xb).double()


class Forward:
    """Y: {'Y1'..'Y5'} pre-activations WITHOUT bias in the scratch's layouts (NHWC);
    pre: the five Y + b (conv ones NCHW); feat, q; staged: 'x', 'c1', 'c2', 'c3',
    'h1' before rounding; bound: the largest sum of absolute terms of any output
    of any of the six GEMMs, on the operands as staged."""


def byte_input(obs):
    """conv1's act(X) of the fused bf16 forward (snake_dqn_forward,
    snake_dqn_map_forward), which has no / 255 branch: the byte's value; NCHW float64."""
    return obs.cpu().permute(0, 3, 1, 2).double()


def forward_model(state, obs, rnd=bf16, x=None):
    """x: conv1's act(X) where it is not staged_input(obs) (byte_input(obs) for the
    fused bf16 forward on bytes above 1)."""
    s = {k: v.detach().double().cpu() for k, v in state.items()}
    out = Forward()
    out.Y, out.pre, out.staged, out.bound = {}, [], {}, 0.0
    t = staged_input(obs) if x is None else x.double().cpu()
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


def backward_model(state, obs, dq, rnd=bf16, pre=None):
    """(grads, staged, sum_bound) of the gradients of sum(dq * Q(obs)), continued
    from the five pre-activations `pre` (None: the unrounded float64 forward's,
    forward_model(state, obs, exact).pre). grads: reference names and layouts.
    staged: every value a matrix-core GEMM stages, BEFORE rounding: 'x', 'c1',
    'c2', 'c3', 'h1' (the activations), 'w:conv2', 'w:conv3', 'w:fc1', 'w:fc2'
    (the input gradients' weights), 'dY1'..'dY5'. sum_bound: the largest sum of
    absolute terms of any output element of any GEMM or bias sum of the chain,
    on the operands as the chain stages them (rounded)."""
    s = {k: v.detach().double().cpu() for k, v in state.items()}
    if pre is None:
        pre = forward_model(state, obs, exact).pre
    masks = [(p > 0).double() for p in pre]
    c1, c2, c3, h1, h2 = (F.relu(p) for p in pre)
    x_in, B = staged_input(obs), pre[0].size(0)
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


def margin(state, obs, rnd):
    """min over the five ReLU layers of min |Y + b| / max |Y + b| on the chain with that rounding."""
    return min(float(p.abs().min() / p.abs().max()) for p in forward_model(state, obs, rnd).pre)
