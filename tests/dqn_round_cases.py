"""The cases that hold the fused bf16 DQN forward (dqn_kernels.hip: k_dqn_conv,
k_dqn_map_conv, k_dqn_fc behind snake_dqn_forward and snake_dqn_map_forward) to
its rounding points (no GPU needed here), so that tests/test_dqn_round_cpu.py
proves exactly what tests/test_dqn_round_gpu.py relies on. The float64 model
they run on, and the rounding points it states, are tests/learner_model.py's
forward_model: the fused forward rounds relu(Y + b) of conv1, conv2, conv3 and
fc1 to bf16 (nearest even) as it stores them, and nothing else but the weights.

Cases:
  rounding    tests/dqn_probe.py's integer probes with conv1's weight and bias
              times 61 (learner_fwd16_cases.scaled_state): c1 grows past 256,
              where odd integers are no bf16 values and most of them are exact
              ties; everything stays an integer and every sum of absolute terms
              below 2^24, so fp32 accumulation in any order is exact and the
              kernels must EQUAL the model -- which a kernel that truncates,
              rounds ties up, rounds elsewhere or nowhere does not.
  persistent  one key per plan with 64 unique rows, gathered on the GPU to the
              batch of the persistent-loop tests.
  bytes       the unscaled probe net on bytes from {1, 2, 3, 128, 255} at the
              probe's ones: the fused forward has no / 255 branch, the model is
              fed the byte's value.
  real        a small random-real net: the kernels differ from the model by fp32
              summation order and rare rounding ties only."""
import functools

import torch

import dqn_probe as P
import learner16_cases as L16
import learner_fwd16_cases as FC
import learner_model as M

SUM_LIMIT = 2 ** 24

# (h, w, c, num_actions, seed, B); B = 70 and 37 are no multiples of 16
WINDOW_KEYS = ((3, 3, 8, 3, 0, 70), (5, 5, 16, 2, 0, 70), (9, 9, 16, 3, 1, 70), (11, 11, 8, 3, 0, 70),
               (11, 11, 24, 3, 0, 70),      # the overlaid LDS plan
               (11, 11, 32, 3, 0, 70))
WINDOW_WAVES = P.GRID_WAVES                 # conv_waves 1, 2 and 4
# every one under plan='map' and every value of marlenv.dqn.MAP_CONV_WAVES
MAP_KEYS = ((20, 20, 8, 3, 0, 37), (22, 22, 32, 3, 0, 37), (12, 10, 8, 3, 0, 37), (13, 13, 16, 3, 0, 37),
            (11, 11, 8, 3, 0, 37))

# the persistent loop: 64 unique rows, gathered to test_bf16_persistent_loop's and
# test_map_persistent_loop's batch; conv_waves 0 (the library's default)
PERSIST_UNIQUE = 64
PERSIST_KEYS = {'window': (11, 11, 24, 3, 0, PERSIST_UNIQUE), 'map': (20, 20, 8, 3, 0, PERSIST_UNIQUE)}

ROUNDING_KEYS = WINDOW_KEYS + MAP_KEYS + tuple(PERSIST_KEYS.values())

# (key, plans): the unscaled probe net on bytes from BYTE_VALUES
BYTE_VALUES = (1, 2, 3, 128, 255)
BYTE_CASES = (((5, 5, 8, 3, 0, 70), ('window', 'map')), ((20, 20, 8, 3, 0, 37), ('map',)))

# DQNLearner.actor(), the bf16 target and the mixed-precision forward on one
# expectation: (key of learner_fwd16_cases.ROUNDING_KEYS, the plan 'auto' takes)
LEARNER_KEYS = (((5, 5, 8, 3, 0, 70), 'window'), ((20, 20, 8, 3, 0, 5), 'map'))


class RoundingCase:
    """model: the float64 model with bf16 rounding; exact: the unrounded chain."""

    def __init__(self, key):
        p = P.probe(*key)
        self.key, self.obs = key, p.obs
        self.state = FC.scaled_state(p.state)
        self.model = M.forward_model(self.state, self.obs)
        self.exact = M.forward_model(self.state, self.obs, M.exact)


@functools.lru_cache(maxsize=None)
def rounding_case(key):
    """Shared between the tests of a session; nobody writes to its tensors."""
    return RoundingCase(key)


class ByteCase:
    def __init__(self, key):
        p = P.probe(*key)
        g = P._gen(*(key + (255,)))
        pick = torch.randint(0, len(BYTE_VALUES), tuple(p.obs.shape), generator=g)
        self.key, self.state = key, p.state
        self.obs = (p.obs * torch.tensor(BYTE_VALUES, dtype=torch.uint8)[pick]).contiguous()
        x = M.byte_input(self.obs)
        self.model = M.forward_model(self.state, self.obs, x=x)
        self.exact = M.forward_model(self.state, self.obs, M.exact, x=x)


@functools.lru_cache(maxsize=None)
def byte_case(key):
    return ByteCase(key)


# ---- the real-valued case ----------------------------------------------------------------
REAL_GEOM = (5, 5, 8, 3)
# The first seed from 0 at which every unit of the bf16 chain AND of the unrounded
# chain is MASK_MARGIN of its layer's scale away from its ReLU threshold
# (tests/test_dqn_round_cpu.py asserts it): the kernels' zeros are then the
# model's, and the model's the float64 reference's.
REAL_SEED = 5


def real_case(seed=REAL_SEED):
    """(state, obs): learner16_cases.real_case's net and 0/1 bytes at 5x5x8, B = 6."""
    return L16.real_case(seed, geom=REAL_GEOM)[:2]


def real_margin(seed):
    state, obs = real_case(seed)
    return min(M.margin(state, obs, M.bf16), M.margin(state, obs, M.exact))


def first_stable_seed(limit=200):
    for seed in range(limit):
        if real_margin(seed) >= L16.MASK_MARGIN:
            return seed
    raise AssertionError('no seed below %d keeps every unit off its ReLU threshold' % limit)
