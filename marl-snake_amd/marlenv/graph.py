"""The graph observation of the reference's SnakeGraph-v1 on the GPU.

GraphSnakeEnv._process_obs (graph_snake_env.py:47-103) turns every live snake's
grid observation into 5 ray-cast feature vectors -- forward, left, right and
the two forward diagonals, each the distance-weighted sum of the cells' channels
up to the first wall. GraphObs is that rule for a whole batch in one launch,
through snake_graph_obs (marl-snake_amd/csrc/graph_kernels.hip; the exact
semantics are in include/snake_env.h); GraphVecEnv is a SnakeVecEnv that returns
these features in place of the grid observation.

source='own': snake s reads its own observation, dead snakes get zero rows.
source='reference': the reference indexes the observations with a counter of
the live snakes, so once a snake below s has died, live snake s reads another
snake's observation; this mode reproduces that, and is what the single-env
GraphSnakeEnv (envs/graph_snake_env.py) is built on.
"""
import ctypes

import numpy as np

from . import spaces
from ._device import get_torch as _torch, check_on, check_tensor, ptr, stream_ptr
from ._native import GraphCfg, check, lib
from .vec_env import SnakeVecEnv

SOURCES = ('own', 'reference')
RAYS = 5
HUMAN_MESSAGE = "This is not yet implemented for 'human' observers."      # graph_snake_env.py:50-51


def _out_dtype(dtype):
    torch = _torch()
    dtype = torch.float64 if dtype is None else dtype
    if dtype not in (torch.float64, torch.float32):
        raise ValueError('dtype must be torch.float64 or torch.float32 (got %r)' % (dtype,))
    return dtype


def _check_source(source):
    if source not in SOURCES:
        raise ValueError("source must be 'own' or 'reference' (got %r)" % (source,))
    return source


class GraphObs:
    """_process_obs for the (N, S) snakes of a SnakeVecEnv at once.

    env: the SnakeVecEnv whose snake records (head, direction, alive) are read;
    observer 'snake', at most 16 snakes, at most 16 stacked frames, a vision
    range of at most 127 (anything else raises ValueError, before any device
    work). dtype: torch.float64 (the reference's), or torch.float32 = the
    float64 result rounded once."""

    def __init__(self, env, source='own', dtype=None, lib_path=None):
        torch = _torch()
        self.source = _check_source(source)
        self.dtype = _out_dtype(dtype)
        if int(env.cfg.observer) != 0:
            raise ValueError(HUMAN_MESSAGE)
        S, h, w, c = (int(v) for v in env.obs_shape)
        self._L = L = lib(lib_path)
        self.cfg = GraphCfg(h, w, c, S, int(env.cfg.vision_range), SOURCES.index(source),
                            int(self.dtype == torch.float32))
        check(L.snake_graph_plan(ctypes.byref(self.cfg)), L)       # ValueError before any device work
        self.env = env
        self.obs_shape = (S, h, w, c)
        self.out_shape = (S, RAYS, c)

    def __call__(self, obs=None):
        """obs: contiguous uint8 (N, S, h, w, C) on the env's device, the
        observation of the env's last step or reset (None: that tensor itself,
        as long as the caller still holds it). Returns (N, S, 5, C), freshly
        allocated; the rows of dead snakes are zero. Enqueued on the current
        stream, which must be ordered after the step (it is when both run on
        the same stream)."""
        torch = _torch()
        env = self.env
        if obs is None:
            obs = env.latest_obs()
            if obs is None:
                raise ValueError('GraphObs: the env has no observation that is still alive; pass obs')
        N = env.num_envs
        check_tensor('GraphObs', 'obs', obs, 'uint8', (N,) + self.obs_shape, contiguous=True)
        check_on('obs', obs, env.device, 'GraphObs')
        out = torch.empty((N,) + self.out_shape, dtype=self.dtype, device=env.device)
        with torch.cuda.device(env.device):
            check(self._L.snake_graph_obs(ctypes.byref(self.cfg), ptr(obs), ptr(env.snake), ptr(out), N,
                                          stream_ptr(env.device)), self._L)
        return out

    def alive(self):
        """(N, S) bool: the snakes whose rows are features (the others' are zero)."""
        env = self.env
        return ((env.snake.view(env.num_envs, env.num_snakes, 4)[..., 1] >> 8) & 1).bool()


class GraphVecEnv:
    """SnakeVecEnv with the graph observation: the same constructor arguments
    plus source and dtype (GraphObs); reset() and step() return the (N, S, 5, C)
    features where SnakeVecEnv returns the grid observation, which is kept as
    .grid_obs. Everything else (rewards, dones, info, auto-reset, the state
    accessors) is the SnakeVecEnv's, reached through this object."""

    def __init__(self, num_envs, num_snakes=4, source='own', dtype=None, **kwargs):
        if kwargs.get('observer', 'snake') != 'snake':
            raise ValueError(HUMAN_MESSAGE)
        _check_source(source)
        dtype = _out_dtype(dtype)
        self.env = SnakeVecEnv(num_envs, num_snakes=num_snakes, **kwargs)
        self.graph = GraphObs(self.env, source=source, dtype=dtype, lib_path=kwargs.get('lib_path'))
        self.grid_obs = None
        self.grid_obs_shape = self.env.obs_shape
        self.obs_shape = self.graph.out_shape
        high = float(np.sum(1.0 / np.arange(1, (self.env.cfg.vision_range or RAYS) + 1)))
        np_dtype = np.float64 if self.graph.cfg.out_f32 == 0 else np.float32
        self.single_observation_space = spaces.Box(0.0, high, self.obs_shape, np_dtype)
        self.observation_space = spaces.Box(0.0, high, (self.env.num_envs,) + self.obs_shape, np_dtype)

    def __getattr__(self, name):
        if name.startswith('__') or name == 'env':
            raise AttributeError(name)
        return getattr(self.env, name)

    def reset(self, mask=None):
        """SnakeVecEnv.reset; the features of every env are recomputed (from
        uninitialised grid rows for the envs outside mask, as .grid_obs has them)."""
        self.grid_obs = self.env.reset(mask)
        return self.graph(self.grid_obs)

    def step(self, actions):
        self.grid_obs, rew, done, info = self.env.step(actions)
        return self.graph(self.grid_obs), rew, done, info

    def alive(self):
        return self.graph.alive()

    def close(self):
        self.env.close()
