"""The reference evaluator's action rule on the GPU.

train_dqn.py's `--mode eval` / `--mode battle` do not take the argmax of the
Q-values directly: DQN_Evaluator.get_action (train_dqn.py:433-580, driven by
the loop at :625-646) first masks the moves that leave the map, run into a wall
or a body, land beside an enemy head, land on a cell an earlier snake of the env
has just claimed, or lead into a pocket smaller than the snake (a flood fill
capped at 60 cells). SafeActions is that rule for a whole batch, through
snake_safe_actions (marl-snake_amd/csrc/policy_kernels.hip; the exact semantics
are in include/snake_env.h); evaluate() is the vector form of
DQN_Evaluator.evaluate.
"""
import ctypes

from ._device import get_torch as _torch, bind_device, check_tensor, ptr, skip_mask, stream_ptr
from ._native import DEFINES, PolicyCfg, check, lib

DIR_UNKNOWN = DEFINES['SNAKE_DIR_UNKNOWN']      # both bytes of a direction not known yet


class _ObsPolicy:
    """What SafeActions and GreedyActions (arena.py) share: a rule on the (N, S,
    h, w, 8) observations with one direction per snake, kept across calls."""

    def __init__(self, obs_shape, fill_limit, device, lib_path):
        if len(obs_shape) != 4:
            raise ValueError('obs_shape must be (S, h, w, 8) (got %r)' % (tuple(obs_shape),))
        S, h, w, c = (int(v) for v in obs_shape)
        self._L = L = lib(lib_path)
        self.cfg = PolicyCfg(h, w, c, S, int(fill_limit))
        check(L.snake_policy_plan(ctypes.byref(self.cfg)), L)      # ValueError before any device work
        self.obs_shape = (S, h, w, c)
        self.device = _torch().device(device) if device is not None else None   # None: the first obs's
        self.dirs = None        # (N, S, 2) int8 (dy, dx), kept across calls when none are passed

    def _batch(self, obs):
        """(device, N) of an observation batch; binds this object to its device."""
        check_tensor(type(self).__name__, 'obs', obs, 'uint8', (None,) + self.obs_shape, contiguous=True)
        bind_device(self, obs.device, 'observations', 'obs is')
        return obs.device, obs.shape[0]

    def _check_dirs(self, dirs, N, dev):
        torch = _torch()
        if dirs is not None and (dirs.dtype != torch.int8 or tuple(dirs.shape) != (N, self.obs_shape[0], 2)
                                 or not dirs.is_contiguous() or dirs.device != dev):
            raise TypeError('dirs must be a contiguous int8 (N, S, 2) tensor on %s' % dev)

    def _dirs(self, dirs, N, dev):
        """The caller's dirs (after _check_dirs), or this object's own, all unknown when N changes."""
        if dirs is not None:
            return dirs
        if self.dirs is None or self.dirs.shape[0] != N:
            torch = _torch()
            self.dirs = torch.full((N, self.obs_shape[0], 2), DIR_UNKNOWN, dtype=torch.int8, device=dev)
        return self.dirs

    def forget(self, mask):
        """Directions of the envs where mask (N,) is True become unknown (an
        episode ended: the reference starts each one with current_directions = None)."""
        if self.dirs is not None:
            torch = _torch()
            m = torch.as_tensor(mask, device=self.dirs.device).to(torch.bool).reshape(-1, 1, 1)
            self.dirs.masked_fill_(m, DIR_UNKNOWN)


class SafeActions(_ObsPolicy):
    """get_action for (N, S) snakes at once.

    obs_shape: (S, h, w, 8), a SnakeVecEnv's obs_shape (frame_stack 1, h and w
    at most 64, at most 16 snakes; anything else raises ValueError).
    fill_limit: the flood fill's cap (the reference's 60)."""

    def __init__(self, obs_shape, fill_limit=60, device=None, lib_path=None):
        super().__init__(obs_shape, fill_limit, device, lib_path)

    def __call__(self, obs, q, skip=None, dirs=None):
        """obs: contiguous uint8 (N, S, h, w, 8); q: float32 (N, S, 3) or (N*S, 3);
        skip: (N, S) bool/uint8 or None -- snakes that get action 0 and keep
        their direction (done, or not controlled by this policy); dirs: int8
        (N, S, 2), read and updated in place (None: this object's own tensor,
        all unknown at first). Returns the actions, int8 (N, S), ready for
        SnakeVecEnv.step."""
        torch = _torch()
        S = self.obs_shape[0]
        dev, N = self._batch(obs)
        check_tensor('SafeActions', 'q', q, 'float32')
        if tuple(q.shape) not in ((N, S, 3), (N * S, 3)):
            raise ValueError('q shape %s is neither (%d, %d, 3) nor (%d, 3)' % (tuple(q.shape), N, S, N * S))
        q = q.to(dev).contiguous()
        skip = skip_mask(skip, N, S, dev)
        self._check_dirs(dirs, N, dev)
        dirs = self._dirs(dirs, N, dev)
        actions = torch.empty((N, S), dtype=torch.int8, device=dev)
        with torch.cuda.device(dev):
            check(self._L.snake_safe_actions(ctypes.byref(self.cfg), ptr(obs), ptr(q), ptr(skip), ptr(dirs),
                                             ptr(actions), N, stream_ptr(dev)), self._L)
        self._keep = (obs, q, skip)
        return actions


def evaluate(env, qnet, steps, policy=None):
    """The vector form of DQN_Evaluator.evaluate (train_dqn.py:582-676): steps
    `env` (a SnakeVecEnv with all-done auto-reset) `steps` times with the
    safe-action rule on qnet's Q-values. qnet: any callable from uint8
    (N*S, h, w, 8) observations to float32 (N*S, 3), e.g. DQNForward(...) on
    the 20x20 full map (bf16 map path; precision='fp32' where the argmax has to
    follow the reference's fp32 arithmetic bit for bit). A snake that is done gets action 0
    until its env's episode ends, and every episode starts with unknown
    directions, as in the reference.

    Returns (episodes, mean_score, mean_steps): the episodes that finished and,
    over them, the means per snake of info['episode_scores'] and
    info['episode_steps'] -- the reference's "average reward per snake" and
    "average timelife" (nan when no episode finished). An episode ends by the
    env's own rule, its max_episode_steps included, not by the reference's cap
    of 1 000 steps per episode."""
    torch = _torch()
    N = env.num_envs
    S, h, w, c = env.obs_shape
    if policy is None:
        policy = SafeActions(env.obs_shape, device=env.device)
    obs = env.reset()
    policy.forget(torch.ones(N, dtype=torch.bool, device=env.device))
    skip = None
    episodes = torch.zeros((), dtype=torch.int64, device=env.device)
    score = torch.zeros((), dtype=torch.float64, device=env.device)
    life = torch.zeros((), dtype=torch.float64, device=env.device)
    for _ in range(int(steps)):
        q = qnet(obs.view(N * S, h, w, c))
        actions = policy(obs, q, skip=skip)
        obs, _, done, info = env.step(actions)
        ended = info['episode_done']
        policy.forget(ended)
        skip = done & ~ended[:, None]
        episodes += ended.sum()
        score += info['episode_scores'].sum()       # (zeros where the episode goes on)
        life += info['episode_steps'].sum()
    n = int(episodes)
    if n == 0:
        return 0, float('nan'), float('nan')
    return n, float(score) / (n * S), float(life) / (n * S)
