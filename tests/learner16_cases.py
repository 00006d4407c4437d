"""The cases of the bf16 backward's tests (snake_dqn32_backward_bf16; no GPU
needed here), so that tests/test_learner_bf16_cpu.py proves exactly what
tests/test_learner_bf16_gpu.py relies on. The float64 model they run on, and
the rounding points it states, are tests/learner_model.py's backward_model.

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
import learner_model as M

ROUNDING_KEYS = ((5, 5, 8, 3, 0, 70), (5, 5, 24, 5, 0, 70), (20, 20, 8, 3, 0, 5))
ROUNDING_SCALE = 29.0
# the dY buffers in which rounding must change at least one entry, per rounding case
ROUNDED_DY = {ROUNDING_KEYS[0]: (1, 2, 3, 4, 5), ROUNDING_KEYS[1]: (1, 2, 3, 4, 5), ROUNDING_KEYS[2]: (1, 2, 3, 4)}


def ref_grads_bf16(state, obs, dq):
    """The float64 model of snake_dqn32_backward_bf16: the gradients of
    sum(dq * Q(obs)) with bf16 rounding at the header's rounding points;
    reference names and layouts, like learner_cases.ref_grads."""
    return M.backward_model(state, obs, dq, M.bf16)[0]


@functools.lru_cache(maxsize=None)
def rounding_case(key):
    """(case, dq * 29, the model's gradients); shared, nobody writes to its tensors."""
    case = LC.backward_case(key)
    dq = (case.dq * ROUNDING_SCALE).contiguous()
    return case, dq, ref_grads_bf16(case.state, case.obs, dq)


# ---- the real-valued case ---------------------------------------------------------
REAL_GEOM = (3, 4, 8, 3)        # h, w, c, A
REAL_B = 6
# The first seed from 0 at which margin(..., exact) >= MASK_MARGIN holds for the case
# and for its obs * 255 variant (tests/test_learner_bf16_cpu.py asserts it holds).
REAL_SEED = 0
# |Y + b| >= 2e-5 of the layer's max |Y + b|: twice the fp32 forward's documented
# 1e-5 accuracy, so the fp32 forward's masks are the float64 forward's
MASK_MARGIN = 2e-5


def real_case(seed=None, scaled=False, geom=REAL_GEOM):
    """(state, obs, dq): weights uniform in +-1/sqrt(fan_in), Bernoulli bytes
    (times 255 with scaled: the /255 branch), dq normal / B."""
    h, w, c, A = geom
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


def first_stable_seed(rnd, limit=200):
    """The first seed at which every unit of the chain with that rounding (and of
    its obs * 255 variant) is MASK_MARGIN of its layer's scale off its ReLU threshold."""
    for seed in range(limit):
        if all(M.margin(*real_case(seed, sc)[:2], rnd) >= MASK_MARGIN for sc in (False, True)):
            return seed
    raise AssertionError('no seed below %d keeps every unit off its ReLU threshold' % limit)
