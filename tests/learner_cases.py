"""Cases and float64 references of the learner tests (no GPU needed here), so
that tests/test_learner_cpu.py checks exactly what tests/test_learner_gpu.py
runs.

Backward: the integer probe nets of tests/dqn_probe.py with a dense integer dq
from {-1, 0, 1} make every gradient an integer whose sum of absolute terms
stays far below 2^24, so an fp32 backward in ANY summation order must equal the
float64 autograd reference. The CPU file recomputes the bound and the
integrality for every case below.

Split M: a weight gradient's M = B*h*w rows are cut into chunks of
chunk_rows(M) rows. (4, 33, 8, 3, 0, 65) has M = 65 * 132 = 8 580 = 4 * 2 048 +
388: five chunks, the last one ragged (and 388 = 24 * 16 + 4 ends inside a
16-row stage)."""
import functools

import numpy as np
import torch

import dqn_probe as P

F = torch.nn.functional

# (h, w, c, num_actions, seed, B)
BACKWARD_CASES = (
    (5, 5, 8, 3, 0, 70),
    (5, 5, 8, 3, 1, 129),       # B*h*w = 25 * 128 + 25; also run at B = 1 and 127 (prefixes)
    (4, 33, 8, 3, 0, 65),       # the widest matrix-core patch of the forward; five split-M chunks, ragged last
    (12, 10, 8, 3, 0, 65),      # B*h*w = 61 * 128 - 8
    (2, 34, 8, 3, 0, 65),       # the forward's vector-ALU fallback
    (5, 5, 24, 5, 0, 70),
    (20, 20, 8, 3, 0, 5),       # train_dqn.py's own Config
    (1, 1, 8, 3, 0, 70),        # only the centre taps
)
PREFIXES = {(5, 5, 8, 3, 1, 129): (1, 127)}
EXTRA_CASES = ((5, 5, 64, 3, 0, 70),)       # the forward's C + 8 cell stride
SUM_LIMIT = 2 ** 24

PARAMS = tuple(n + s for n in ('conv1', 'conv2', 'conv3', 'fc1', 'fc2', 'fc3') for s in ('.weight', '.bias'))


def chunk_rows(M):
    """dqn_train_kernels.hip's split-M rule."""
    c = -(-M // 128)
    c = -(-c // 16) * 16
    return max(c, 2048)


def probe_dq(key):
    h, w, c, A, seed, B = key
    g = P._gen(h, w, c, A, seed, B, 4242)
    return torch.randint(-1, 2, (B, A), generator=g).float()


def forward64(params, x):
    """train_dqn.py:104-151 on float64 leaves; x NCHW float64."""
    t = x
    for name in ('conv1', 'conv2', 'conv3'):
        t = F.relu(F.conv2d(t, params[name + '.weight'], params[name + '.bias'], padding=1))
    t = t.reshape(t.size(0), -1)
    for name in ('fc1', 'fc2'):
        t = F.relu(F.linear(t, params[name + '.weight'], params[name + '.bias']))
    return F.linear(t, params['fc3.weight'], params['fc3.bias'])


def input64(obs):
    x = obs.cpu().permute(0, 3, 1, 2).double()
    return x / 255.0 if float(x.max()) > 1.0 else x


def ref_grads(state, obs, dq):
    """float64 autograd gradients of sum(dq * Q(obs)), reference names and layouts."""
    params = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in state.items()}
    q = forward64(params, input64(obs))
    (q * dq.double().cpu()).sum().backward()
    return {k: v.grad for k, v in params.items()}


def term_bound(state, obs, dq):
    """max over every gradient entry of the sum of the absolute values of its
    terms: |dY|^T |A| per layer, |dY| propagated through |W| with the true ReLU
    masks. Autograd computes it on a network with |W| weights whose layer inputs
    carry the TRUE activations as values and the |W| path as gradient."""
    s = {k: v.detach().double().cpu() for k, v in state.items()}
    leaves = {k: v.abs().clone().requires_grad_(True) for k, v in s.items()}
    true_in = input64(obs)
    carried = true_in
    for i, name in enumerate(('conv1', 'conv2', 'conv3', 'fc1', 'fc2')):
        if name == 'fc1':
            true_in, carried = true_in.reshape(true_in.size(0), -1), carried.reshape(carried.size(0), -1)
        op = (lambda t, wt, b: F.conv2d(t, wt, b, padding=1)) if i < 3 else F.linear
        pre = op(true_in, s[name + '.weight'], s[name + '.bias'])
        mask = (pre > 0).double()
        y = op(carried, leaves[name + '.weight'], leaves[name + '.bias']) * mask
        true_in = F.relu(pre)
        carried = true_in + (y - y.detach())
    q = F.linear(carried, leaves['fc3.weight'], leaves['fc3.bias'])
    (q * dq.double().cpu().abs()).sum().backward()
    return max(float(v.grad.max()) for v in leaves.values())


class BackwardCase:
    def __init__(self, key, B=None):
        full = P.probe(*key)
        self.key = key
        self.B = B = key[5] if B is None else B
        self.state, self.obs, self.dq = full.state, full.obs[:B].contiguous(), probe_dq(key)[:B].contiguous()
        self.grads = ref_grads(self.state, self.obs, self.dq)


@functools.lru_cache(maxsize=None)
def backward_case(key, B=None):
    """Shared between the tests of a session; nobody writes to its tensors."""
    return BackwardCase(key, B)


def gpu_backward_runs():
    """(key, B) of every backward run of the GPU file."""
    runs = []
    for key in BACKWARD_CASES + EXTRA_CASES:
        runs.append((key, key[5]))
        runs += [(key, b) for b in PREFIXES.get(key, ())]
    return runs


# ---- TD loss -----------------------------------------------------------------
def td_ref64(q, action, reward, done, next_q, gamma):
    """(loss, dq, d) in float64 from the float32 inputs; gamma a float32 value."""
    q, reward, done, next_q = (t.double().cpu() for t in (q, reward, done, next_q))
    action = action.cpu()
    B = q.shape[0]
    target = reward + ((1.0 - done) * float(np.float32(gamma))) * next_q.max(1).values
    d = q.gather(1, action[:, None])[:, 0] - target
    per_row = torch.where(d.abs() < 1.0, 0.5 * d * d, d.abs() - 0.5)
    dq = torch.zeros_like(q)
    dq[torch.arange(B), action] = d.clamp(-1.0, 1.0) / B
    return per_row.sum() / B, dq, d


def td_dyadic_case(B=64):
    """gamma = 0.5, integer rewards, integer probe Q-values: every quantity is a
    multiple of 1/2 (d), 1/8 (a row's loss) or 1/(8 B). Rows 0-3 are forced to
    d = 1, -1, 0.5 and 0; rows 1 and 3 have done = 1."""
    g = P._gen(B, 777)
    q = P.probe(5, 5, 8, 3, 0, 70).q[:B].float()
    next_q = P.probe(5, 5, 8, 3, 1, 129).q[:B].float()
    action = torch.randint(0, 3, (B,), generator=g)
    reward = torch.randint(-3, 4, (B,), generator=g).float()
    done = (torch.rand(B, generator=g) < 0.3).float()
    forced = ((0.0, 1.0), (1.0, -1.0), (0.0, 0.5), (1.0, 0.0))[:B]
    for b, (dn, d) in enumerate(forced):
        qa = float(q[b, action[b]])
        done[b] = dn
        if d == 0.5:
            next_q[b] = torch.tensor([1.0, 0.0, -1.0])      # 0.5 * max = 0.5
            reward[b] = qa - 1.0
        else:
            reward[b] = qa - d
            if dn == 0.0:
                next_q[b] = torch.tensor([0.0, -2.0, -4.0])
    return q.contiguous(), action, reward, done, next_q.contiguous()


def td_real_case(B=70):
    g = P._gen(B, 778)
    q = torch.randn((B, 3), generator=g) * 2
    next_q = torch.randn((B, 3), generator=g) * 2
    action = torch.randint(0, 3, (B,), generator=g)
    reward = torch.randn(B, generator=g)
    done = (torch.rand(B, generator=g) < 0.3).float()
    return q, action, reward, done, next_q


U = 2.0 ** -24      # the relative error of one correctly rounded fp32 operation
SLACK = 1.0 + 2.0 ** -10    # second-order terms


def td_bounds(q, action, reward, done, next_q, gamma):
    """(loss bound, dq bound [B][A]) for the fp32 kernel against td_ref64.
    Rounded operations per row: (1 - done) is exact (done is 0 or 1); * gamma,
    * max, + reward, q - target round once each, on quantities of magnitude at
    most S = |reward| + |max next_q| + |q|: |d - d64| <= E = 4 U S. clamp and
    smooth-L1 are 1-Lipschitz; dq adds the division's rounding, a row's loss one
    rounding ((0.5 d) d, or |d| - 0.5). The sum: at B <= 256 each thread holds
    one row, then 8 tree levels of one rounded addition each; the mean one
    rounded division."""
    loss64, dq64, d = td_ref64(q, action, reward, done, next_q, gamma)
    B = q.shape[0]
    qa = q.double().gather(1, action[:, None])[:, 0]
    S = reward.double().abs() + next_q.double().max(1).values.abs() + qa.abs()
    E = 4 * U * S
    dq_bound = torch.zeros_like(dq64)
    dq_bound[torch.arange(B), action] = (E / B + U * (dq64[torch.arange(B), action].abs() + E / B)) * SLACK
    per_row = torch.where(d.abs() < 1.0, 0.5 * d * d, d.abs() - 0.5)
    serial = max(0, -(-B // 256) - 1)
    loss_bound = ((E.sum() + (1 + serial + 8) * U * (per_row.sum() + E.sum())) / B + U * float(loss64)) * SLACK
    return float(loss_bound), dq_bound


# ---- clip + Adam ---------------------------------------------------------------
def adam_ref64(p, g, m, v, step, lr, beta1, beta2, eps, max_norm):
    """include/snake_env.h snake_adam_step's formulas in float64 on the float32
    inputs (hyper-parameters as float32 values). Returns p, m, v, norm, and the
    magnitude S = step_size (|beta1 m| + |(1 - beta1) g'|) / denom of the step."""
    f = lambda x: float(np.float32(x))      # noqa: E731
    lr, beta1, beta2, eps, max_norm = f(lr), f(beta1), f(beta2), f(eps), f(max_norm)
    p, g, m, v = (t.double().cpu() for t in (p, g, m, v))
    norm = float(g.pow(2).sum().sqrt())
    coef = min(1.0, max_norm / (norm + f(1e-6)))
    gc = g * coef
    m2 = beta1 * m + (1.0 - beta1) * gc
    v2 = beta2 * v + (1.0 - beta2) * gc * gc
    step_size = lr / (1.0 - beta1 ** step)
    denom = v2.sqrt() / (1.0 - beta2 ** step) ** 0.5 + eps
    S = step_size * ((beta1 * m).abs() + ((1.0 - beta1) * gc).abs()) / denom
    return p - step_size * (m2 / denom), m2, v2, norm, S


def norm_depth(n):
    """Rounded additions on the longest path of the kernel's norm: block j of G
    sums L elements, thread t every 256th (a serial chain), then 8 tree levels;
    one block adds the G partials the same way."""
    G = min(1024, -(-n // 1024))
    L = -(-(-(-n // G)) // 256) * 256
    return (L // 256) + 8 + -(-G // 256) + 8


def adam_bounds(n):
    """(norm's relative bound, K): |p - p64| <= ulp(p)/2 + K U S.
    Norm: squares round once, the non-negative sum D = norm_depth(n) times:
    relative (D + 1) U, halved by the square root, whose own error is 1 ulp =
    2 U (HIP's documented sqrtf bound): e_n = ((D + 1) / 2 + 2) U.
    coef: the addition of 1e-6 and the division (IEEE, U) -> e_n + 2 U; g' = g *
    coef one more: e_g = e_n + 3 U.
    m: 1 - beta1, its product with g', beta1 * m and the sum round once each:
    |m - m64| <= (e_g + 3 U) (|beta1 m| + |(1 - beta1) g'|).
    v (non-negative terms): 1 - beta2, two products with g' (2 e_g), beta2 * v,
    the sum: relative 2 e_g + 4 U; sqrt halves it and adds 2 U; sqrt(1 -
    beta2^t) is rounded to float (U), the division U, + eps U: denom relative
    e_g + 2 U + 2 U + 3 U = e_g + 7 U.
    step: m / denom U, step_size rounded to float U, the product U: relative
    e_g + 10 U of |step| <= S. The final subtraction: ulp(p) / 2.
    K U = (e_g + 3 U) + (e_g + 10 U)."""
    e_n = ((norm_depth(n) + 1) / 2.0 + 2.0)
    e_g = e_n + 3.0
    return e_n * U * SLACK, (2 * e_g + 13.0) * SLACK


# ---- torch restatement of the network (train_dqn.py:104-151) --------------------
class TorchDQN(torch.nn.Module):
    def __init__(self, h, w, c, num_actions):
        super().__init__()
        nn = torch.nn
        self.conv1, self.conv2, self.conv3 = nn.Conv2d(c, 32, 3, padding=1), nn.Conv2d(32, 64, 3, padding=1), \
            nn.Conv2d(64, 64, 3, padding=1)
        self.fc1, self.fc2, self.fc3 = nn.Linear(64 * h * w, 256), nn.Linear(256, 128), nn.Linear(128, num_actions)

    def forward(self, obs):
        x = obs.permute(0, 3, 1, 2).to(self.fc1.weight.dtype)
        if x.max() > 1.0:
            x = x / 255.0
        x = F.relu(self.conv1(x))
        x = F.relu(self.conv2(x))
        x = F.relu(self.conv3(x))
        x = F.relu(self.fc1(x.reshape(x.size(0), -1)))
        return self.fc3(F.relu(self.fc2(x)))


def descent_batch(B=64):
    """One fixed batch at 5x5x8 and a random-real initial net for the twenty
    updates that must lower the loss."""
    g = P._gen(B, 4711)
    state = P.probe_obs(B, 5, 5, 8, 11)
    next_state = P.probe_obs(B, 5, 5, 8, 12)
    action = torch.randint(0, 3, (B,), generator=g)
    reward = torch.randn(B, generator=g)
    done = (torch.rand(B, generator=g) < 0.2).float()
    torch.manual_seed(99)
    net = TorchDQN(5, 5, 8, 3)
    return {k: v.detach().clone() for k, v in net.state_dict().items()}, (state, action, reward, next_state, done)


def torch_update(policy, target, opt, batch, gamma=0.99):
    """Trainer.update_model (:243-257) in torch."""
    state, action, reward, next_state, done = batch
    q = policy(state).gather(1, action[:, None])
    with torch.no_grad():
        nq = target(next_state).max(1)[0]
        tq = reward + (1 - done) * gamma * nq
    loss = F.smooth_l1_loss(q.squeeze(), tq)
    opt.zero_grad()
    loss.backward()
    torch.nn.utils.clip_grad_norm_(policy.parameters(), 10)
    opt.step()
    return loss.detach()
