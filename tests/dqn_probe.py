"""Integer probe networks for the DQN forward kernels (no GPU needed here).

The reference network (train_dqn.py:104-151) with small integer weights and
biases, fed dense 0/1 bytes. bf16 holds every integer up to 256 and fp32 sums of
integers below 2^24 are exact in any order, so while every tensor the bf16
kernels round (the input, the three conv outputs after ReLU, relu(fc1)) stays an
integer <= 256, the kernels' features and Q-values must EQUAL ref64() below:
tests/test_dqn_exact.py asserts torch.equal, tests/test_dqn_probe_cpu.py proves
the preconditions and that the probes notice a wrong weight.

Recipe: a "dealt" layer gives every input index (tap x input channel, or fc
column) to one output row, round-robin through a random permutation, with a
random sign; conv1 is dealt twice and fc2 four times, so no weight column is all
zero. fc3 comes from -3..3, inputs are Bernoulli(1/4). A bias is {0, 1, 2} minus
its unit's median pre-activation over a calibration batch: with plain {0, 1, 2}
about a sixth of the conv3, fc1 and fc2 units never fired on a 70-row batch and
hid a third of the fc weights from the features.

The case tables of the GPU tests live here so that the CPU file checks exactly
the probes the GPU file runs."""
import functools

import torch

F = torch.nn.functional

LAYERS = ('conv1', 'conv2', 'conv3', 'fc1', 'fc2')      # the weighted layers before fc3
ROUNDED = ('x', 'c1', 'c2', 'c3', 'h1')                 # what the bf16 kernels round to bf16
P_ONE = 0.25
CAL_B = 64                                              # calibration batch of probe_net


def _gen(*key):
    g = torch.Generator()
    acc = 12345
    for v in key:
        acc = (acc * 1000003 + int(v) + 1) % (2 ** 31 - 1)
    g.manual_seed(acc)
    return g


def _deal(rows, cols, times, g, signed=True):
    """[rows][cols] integers: per deal, column perm[i] goes to row i % rows with a
    random sign (+1 when not signed). A later deal overwrites, never cancels."""
    w = torch.zeros((rows, cols), dtype=torch.float32)
    for _ in range(times):
        perm = torch.randperm(cols, generator=g)
        r = torch.arange(cols) % rows
        s = (torch.randint(0, 2, (cols,), generator=g) * 2 - 1) if signed else torch.ones(cols, dtype=torch.int64)
        w[r, perm] = s.float()
    return w


def _identity(rows, cols):
    """Output row o takes input column o % cols with weight 1."""
    w = torch.zeros((rows, cols), dtype=torch.float32)
    w[torch.arange(rows), torch.arange(rows) % cols] = 1.0
    return w


def probe_net(h, w, c, num_actions, seed, identity=()):
    """State dict with the reference's parameter names, float32 tensors holding
    integers. Layers named in `identity` get identity-like weights instead (a
    conv passes input channel o % cin through its centre tap, an fc row o takes
    column o % n_in; bias 0): with all but one layer so, a mismatch is that
    layer's."""
    g = _gen(h, w, c, num_actions, seed)
    P = h * w
    state = {}
    # every bias centres its unit: {0, 1, 2} minus the median pre-activation of
    # the unit (a conv channel over all positions) over a calibration batch, so
    # that no unit is dead, or saturated, on every observation and a wrong
    # weight is not hidden behind a dead ReLU
    t = probe_obs(CAL_B, h, w, c, seed + 7919).permute(0, 3, 1, 2).double()
    for name, cout, cin, times in (('conv1', 32, c, 2), ('conv2', 64, 32, 1), ('conv3', 64, 64, 1)):
        if name in identity:
            wt, bias = torch.zeros((cout, cin, 3, 3), dtype=torch.float32), torch.zeros(cout)
            wt[torch.arange(cout), torch.arange(cout) % cin, 1, 1] = 1.0
        else:
            # columns in (tap, channel) order, as the kernels' k index
            wt = _deal(cout, 9 * cin, times, g).reshape(cout, 3, 3, cin).permute(0, 3, 1, 2).contiguous()
            pre = F.conv2d(t, wt.double(), padding=1).permute(1, 0, 2, 3).reshape(cout, -1)
            bias = torch.randint(0, 3, (cout,), generator=g).float() - pre.median(1).values.float()
        state[name + '.weight'], state[name + '.bias'] = wt, bias
        t = F.relu(F.conv2d(t, wt.double(), bias.double(), padding=1))
    t = t.reshape(CAL_B, -1)
    for name, rows, cols, times in (('fc1', 256, 64 * P, 1), ('fc2', 128, 256, 4)):
        if name in identity:
            wt, bias = _identity(rows, cols), torch.zeros(rows)
        else:
            wt = _deal(rows, cols, times, g)
            bias = torch.randint(0, 3, (rows,), generator=g).float()
            bias = bias - F.linear(t, wt.double()).median(0).values.float()
        state[name + '.weight'], state[name + '.bias'] = wt, bias
        t = F.relu(F.linear(t, wt.double(), bias.double()))
    state['fc3.weight'] = torch.randint(-3, 4, (num_actions, 128), generator=g).float()
    state['fc3.bias'] = torch.randint(-3, 4, (num_actions,), generator=g).float()
    return state


def probe_obs(B, h, w, c, seed):
    """(B, h, w, c) uint8 of independent Bernoulli(1/4) bytes."""
    g = _gen(B, h, w, c, seed, 99)
    return (torch.rand((B, h, w, c), generator=g) < P_ONE).to(torch.uint8)


def ref64(state, obs, start=None, acts=None):
    """train_dqn.py:104-151 in float64 on the CPU: (features, q, acts) with acts
    the activations x, c1, c2, c3 (NCHW), h1, h2 after their ReLUs.
    start/acts: recompute from layer `start` on, from earlier activations."""
    s = {k: v.detach().double().cpu() for k, v in state.items()}
    a = dict(acts) if acts is not None else {}
    order = ('conv1', 'conv2', 'conv3', 'fc1', 'fc2')
    first = order.index(start) if start else 0
    if 'x' not in a:
        x = obs.cpu().permute(0, 3, 1, 2).double()
        a['x'] = x / 255.0 if float(x.max()) > 1.0 else x
    src = ('x', 'c1', 'c2', 'c3', 'h1')
    dst = ('c1', 'c2', 'c3', 'h1', 'h2')
    for i in range(first, 5):
        name, t = order[i], a[src[i]]
        if i < 3:
            a[dst[i]] = F.relu(F.conv2d(t, s[name + '.weight'], s[name + '.bias'], padding=1))
        else:
            a[dst[i]] = F.relu(F.linear(t.reshape(t.size(0), -1), s[name + '.weight'], s[name + '.bias']))
    q = F.linear(a['h2'], s['fc3.weight'], s['fc3.bias'])
    return a['h2'], q, a


class Probe:
    """One probe: a net and a batch, with the float64 reference computed once."""

    def __init__(self, h, w, c, num_actions, seed, B):
        self.key = (h, w, c, num_actions, seed, B)
        self.state = probe_net(h, w, c, num_actions, seed)
        self.obs = probe_obs(B, h, w, c, seed)
        self.feat, self.q, self.acts = ref64(self.state, self.obs)


@functools.lru_cache(maxsize=None)
def probe(h, w, c, num_actions, seed, B):
    """Shared between the tests of a session; nobody writes to its tensors."""
    return Probe(h, w, c, num_actions, seed, B)


# ---- the case tables ------------------------------------------------------
SEEDS = (0, 1, 2)
GRID_B = 70          # no multiple of 16 or 32: every fc wave's row tiles partly filled
GRID_SIZES = (3, 5, 7, 9, 11)
GRID_CHANNELS = (8, 16, 24, 32)
GRID_WAVES = (1, 2, 4)
TAIL_GEO = (11, 11, 8)
TAIL_B = (1, 31, 32, 33, 255, 256, 257, 513)        # prefixes of one 513-row probe
ACTIONS_GEO = (5, 5, 16)
ACTIONS = (1, 2, 4)
# persistent loop: (h, w, c, conv_waves); 256 unique observations, gathered
PERSIST_UNIQUE = 256
PERSIST = ((11, 11, 32, 1), (11, 11, 32, 2), (11, 11, 32, 4), (11, 11, 24, 1), (11, 11, 24, 2),
           (11, 11, 24, 4), (11, 11, 8, 0), (3, 3, 8, 0))
SHARP_GEO = ((3, 3, 8), (11, 11, 32))

# fp32 mode: (h, w, c, num_actions, B, matrix-core convolutions?). B*h*w lies on
# both sides of a multiple of 128 (k_conv32_mfma's / k_gemm32's row tile): 65 *
# 132 = 67 * 128 + 4, 65 * 120 = 61 * 128 - 8, 127 * 25 = 25 * 128 - 25, 129 * 25
# = 25 * 128 + 25; B on both sides of 128 (k_fc32_mfma's row tile).
FP32_CASES = (
    (4, 33, 8, 3, 65, True),        # the widest strip whose 64-channel patch fits
    (2, 34, 8, 3, 65, False),       # one column more: vector-ALU GEMM
    (4, 34, 8, 3, 65, False),
    (12, 10, 8, 3, 65, True),
    (1, 7, 8, 3, 70, False),
    (1, 1, 8, 3, 70, False),
    (5, 5, 8, 3, 129, True),        # run at B = 1, 127, 129 (prefixes)
    (5, 5, 24, 3, 70, True),        # cell stride C
    (5, 5, 40, 3, 70, True),
    (5, 5, 64, 3, 70, True),        # cell stride C + 8
    (5, 5, 128, 3, 70, False),      # C > 64 decides the patch size
    (12, 10, 80, 3, 65, True),      # C > 64 on the matrix cores
    (5, 5, 8, 1, 70, True),
    (5, 5, 8, 5, 70, True),
    (5, 5, 8, 64, 70, True),
    (20, 20, 8, 3, 5, True),        # train_dqn.py's own Config
)
FP32_PREFIXES = {(5, 5, 8, 3, 129): (1, 127, 129)}


def fp32_conv_on_matrix_cores(h, w, c):
    """snake_dqn32_forward's dispatch, restated: the LDS patch of 128 consecutive
    output rows at max(c, 64) channels fits 80 KiB."""
    cc = max(c, 64)
    stride = cc + (0 if cc % 16 else 8)
    rows = (127 + w - 1) // w + 1 + (127 + h * w - 1) // (h * w) + 2
    return rows * (w + 2) * stride * 4 <= 80 * 1024


def bf16_probe_keys():
    """Every (h, w, c, num_actions, seed, B) probe the bf16 GPU tests run."""
    keys = [(s, s, c, 3, seed, GRID_B) for s in GRID_SIZES for c in GRID_CHANNELS for seed in SEEDS]
    keys.append(TAIL_GEO + (3, 0, max(TAIL_B)))
    keys += [ACTIONS_GEO + (a, seed, GRID_B) for a in ACTIONS for seed in SEEDS]
    for h, w, c, _ in PERSIST:
        k = (h, w, c, 3, 0, PERSIST_UNIQUE)
        if k not in keys:
            keys.append(k)
    return keys


def fp32_probe_keys():
    return [(h, w, c, a, seed, B) for h, w, c, a, B, _ in FP32_CASES for seed in SEEDS[:2]]
