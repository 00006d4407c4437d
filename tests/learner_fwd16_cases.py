"""The cases of the bf16 mixed-precision forward's tests
(snake_dqn32_forward_bf16; no GPU needed here), so that
tests/test_learner_fwd16_cpu.py proves exactly what
tests/test_learner_fwd16_gpu.py relies on. The float64 model they run on, and
the rounding points it states, are tests/learner_model.py's forward_model;
the gradients continue from the model's Y through its backward_model (masks and
act(X) are the model's), with the bf16 backward's rounding or none.

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

import learner16_cases as L16
import learner_cases as LC
import learner_model as M

YS = M.YS

BYTES_KEY = (5, 5, 8, 3, 0, 70)
ROUNDING_KEYS = ((5, 5, 8, 3, 0, 70), (5, 5, 24, 5, 0, 70), (20, 20, 8, 3, 0, 5), (4, 33, 8, 3, 0, 65))
ROUNDING_SCALE = 61.0
PREFIX_KEY, PREFIX_B = (5, 5, 8, 3, 1, 129), (1, 127, 129)

# Two geometries for fc1's split K that tests/learner_cases.py's table lacks (the
# table's fc1 chunks sit at the 1 024 floor, or end even):
#   (17, 17, 8, 3, 0, 5)   K = 18 496, chunk 1 216 (above the floor), 16 chunks, the last of 256 steps
#   (3, 11, 8, 3, 0, 37)   K = 2 112: three chunks, the last of 64 steps
SPLIT_K_KEYS = ((17, 17, 8, 3, 0, 5), (3, 11, 8, 3, 0, 37))
# largest probe activation and learner_cases.term_bound of the two, as computed once
SPLIT_K_FACTS = {(17, 17, 8, 3, 0, 5): (117, 158020), (3, 11, 8, 3, 0, 37): (49, 86974)}
# one more probe the guard-band tests run through the bf16 forward only
# (tests/test_guard_dqn_gpu.py): five actions at 5x5x8
FORWARD_ONLY_KEYS = ((5, 5, 8, 5, 0, 70),)


def exact_runs():
    """(key, B) of every run that must EQUAL the float64 reference: the learner
    table's runs and the split-K geometries."""
    return LC.gpu_backward_runs() + [(k, k[5]) for k in SPLIT_K_KEYS]


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


# rnd of learner_model.backward_model per backward_precision
BACKWARD_RND = {'fp32': M.exact, 'bf16': M.bf16}


def reference_y(state, obs):
    """{'Y1'..'Y5'} of the unrounded float64 forward, in the scratch's layouts."""
    return M.forward_model(state, obs, M.exact).Y


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
        self.model = M.forward_model(self.state, self.obs)
        self.exact = M.forward_model(self.state, self.obs, M.exact)
        self.grads, self.grad_bound = {}, 0.0
        for mode, rnd in BACKWARD_RND.items():
            self.grads[mode], _, b = M.backward_model(self.state, self.obs, self.dq, rnd, pre=self.model.pre)
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


def real_case(scaled=False):
    return L16.real_case(REAL_SEED, scaled)
