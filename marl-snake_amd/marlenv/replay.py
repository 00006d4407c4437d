"""The reference trainer's replay buffer and rollout loop on the GPU.

train_dqn.py's `--mode train` pushes one Transition(state, action, reward,
next_state, done) per live snake and step into a deque(maxlen=BUFFER_SIZE)
(train_dqn.py:89-100, :290-298) and update_model samples its batches from it
(:228-240). ReplayBuffer is that deque in device memory, filled straight from a
SnakeVecEnv's output tensors through snake_replay_push and read through
snake_replay_gather (marl-snake_amd/csrc/replay_kernels.hip; the exact
semantics are in include/snake_env.h); Collector is the vector form of the
inner loop of Trainer.train (:277-308). Nothing on the way syncs with the host.

Observations are 0/1 bytes in channel groups of 8, so the rings keep one byte
per cell and frame: 1/8 of the memory of the tensors that were pushed. A byte
that is neither 0 nor 1 comes back as 1.
"""
import ctypes

from ._device import get_torch as _torch, bind_device, check_on, check_tensor, default_device, ptr, stream_ptr
from ._native import DEFINES, ReplayCfg, ReplayLayout, ReplayRings, check, lib
from .pyrandom import PyRandom

FORMATS = {'uint8': DEFINES['SNAKE_REPLAY_U8_NHWC'], 'float32': DEFINES['SNAKE_REPLAY_F32_NCHW']}


class ReplayBuffer:
    """deque(maxlen=capacity) of transitions, on the device.

    obs_shape: (S, h, w, C), a SnakeVecEnv's obs_shape (C a multiple of 8, at
    most 16 snakes; anything else raises ValueError). early_death: None or
    (steps, penalty), the reference's EARLY_DEATH_THRESHOLD and
    EARLY_DEATH_PENALTY: a snake that dies at an episode step below `steps` is
    stored with reward + penalty. Logical index 0 is the oldest transition
    held, len(buf) - 1 the newest, as in the reference's deque."""

    def __init__(self, obs_shape, capacity, early_death=None, device=None, lib_path=None):
        if len(obs_shape) != 4:
            raise ValueError('obs_shape must be (S, h, w, C) (got %r)' % (tuple(obs_shape),))
        S, h, w, c = (int(v) for v in obs_shape)
        steps, penalty = (0, 0.0) if early_death is None else early_death
        self._L = L = lib(lib_path)
        self.cfg = ReplayCfg(h, w, c, S, int(capacity), int(steps), float(penalty))
        self.layout = ReplayLayout()
        check(L.snake_replay_plan(ctypes.byref(self.cfg), 0, ctypes.byref(self.layout)), L)   # ValueError before any device work
        self.obs_shape = (S, h, w, c)
        self.capacity = int(capacity)
        self.device = _torch().device(device) if device is not None else None   # None: the first push's
        self.count = None       # int64 (1,) on the device: transitions ever stored
        self._rings = None
        self._scratch = {}      # num_envs -> the push's scratch
        self._keep = None

    # ---------------------------------------------------------------- buffers
    def _allocate(self, dev):
        torch = _torch()
        lay = self.layout

        def zeros(nbytes):
            return torch.zeros(max(int(nbytes), 16), dtype=torch.uint8, device=dev)

        self.device = dev
        self._state, self._next_state = zeros(lay.state), zeros(lay.next_state)
        self._action, self._reward, self._done = zeros(lay.action), zeros(lay.reward), zeros(lay.done)
        self.count = torch.zeros(1, dtype=torch.int64, device=dev)
        self._rings = ReplayRings(self._state.data_ptr(), self._next_state.data_ptr(), self._action.data_ptr(),
                                  self._reward.data_ptr(), self._done.data_ptr(), self.count.data_ptr())

    def _own_device(self):
        """The buffer's device; before any push, the rings are made on the one
        it was given, or on the current one."""
        if self._rings is None:
            self._allocate(default_device(self.device, 'ReplayBuffer'))
        return self.device

    # -------------------------------------------------------------------- API
    def push(self, obs, next_obs, actions, rewards, done, skip=None, step=None):
        """One env step's transitions. obs, next_obs: contiguous uint8 (N, S, h,
        w, C), the observations before and after the step; actions: int8 (N, S);
        rewards: float64 (N, S); done: bool/uint8 (N, S), the dones after the
        step; skip: bool/uint8 (N, S) or None -- snakes that were done before
        the step and store nothing; step: int32 (N,) or None -- the index of
        this step in each env's episode (0 for the first), for the early-death
        penalty. Stored in (env, snake) order. Asynchronous on the current
        stream; the inputs are kept alive until the next call."""
        torch = _torch()
        S = self.obs_shape[0]
        for name, t in (('obs', obs), ('next_obs', next_obs)):
            check_tensor('ReplayBuffer.push', name, t, 'uint8', (None,) + self.obs_shape, contiguous=True)
        if next_obs.shape[0] != obs.shape[0]:
            raise ValueError('obs holds %d envs, next_obs %d' % (obs.shape[0], next_obs.shape[0]))
        N = obs.shape[0]
        small = [('actions', actions, 'int8', (N, S)), ('rewards', rewards, 'float64', (N, S)),
                 ('done', done, ('bool', 'uint8'), (N, S))]
        if skip is not None:
            small.append(('skip', skip, ('bool', 'uint8'), (N, S)))
        if step is not None:
            small.append(('step', step, 'int32', (N,)))
        for name, t, dtypes, shape in small:
            check_tensor('ReplayBuffer.push', name, t, dtypes, shape)
        dev = obs.device
        bind_device(self, dev, 'obs', 'obs is')
        for name, t in [('next_obs', next_obs)] + [(n, t) for n, t, _, _ in small]:
            check_on(name, t, dev, 'ReplayBuffer')
        if self._rings is None:
            self._allocate(dev)
        actions, rewards = actions.contiguous(), rewards.contiguous()
        done = done.contiguous().view(torch.uint8)
        if skip is not None:
            skip = skip.contiguous().view(torch.uint8)
        if step is not None:
            step = step.contiguous()
        scratch = self._scratch.get(N)
        if scratch is None:
            lay = ReplayLayout()
            check(self._L.snake_replay_plan(ctypes.byref(self.cfg), N, ctypes.byref(lay)), self._L)
            scratch = self._scratch[N] = torch.empty(int(lay.scratch), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(self._L.snake_replay_push(
                ctypes.byref(self.cfg), ctypes.byref(self._rings), ptr(obs), ptr(next_obs), ptr(actions), ptr(rewards),
                ptr(done), ptr(skip), ptr(step), N, ptr(scratch), stream_ptr(dev)), self._L)
        self._keep = (obs, next_obs, actions, rewards, done, skip, step)

    def size(self):
        """min(count, capacity) as an int64 (1,) tensor on the device (no sync)."""
        self._own_device()
        return self.count.clamp(max=self.capacity)

    def sample(self, batch_size=None, idx=None, format='uint8', replace=False, generator=None, rng=None, stream=0):
        """(state, action, reward, next_state, done): update_model's five
        tensors (train_dqn.py:236-240) -- action int64 (B,), reward and done
        float32 (B,), and the states as
          format='uint8':   uint8 (B, h, w, C), the bytes that were pushed (what
                            DQNForward and the reference's DQN.forward take);
          format='float32': float32 (B, C, h, w) of 0.0 / 1.0, what
                            x.permute(0, 3, 1, 2).float() (:122) makes of them.
        idx: int64 (B,) logical indices (0 the oldest; repeats allowed): a pure
        gather. An index outside [0, len) is a contract violation (the kernel
        clamps it so that it cannot read outside the rings). Without idx,
        batch_size indices are drawn on the device from the device-side size,
        without a host sync: replace=False (random.sample does not repeat) by
        the top batch_size of random keys over the slots held, replace=True by
        floor(u * size). The caller guarantees len(buf) >= batch_size (the
        reference's MIN_BUFFER_SIZE guard). generator: a torch.Generator of the
        buffer's device.
        rng: a PyRandom; the indices are then the reference's own
        random.sample(self.buffer, batch_size) (:96-97) drawn from its stream
        `stream` by snake_pyrandom_sample: one launch of O(batch_size) work,
        whatever the capacity, at most 4096 indices from a capacity below 2^31.
        It excludes idx and replace=True (ValueError)."""
        torch = _torch()
        if format not in FORMATS:
            raise ValueError("format must be 'uint8' or 'float32' (got %r)" % (format,))
        if rng is not None:
            if replace:
                raise ValueError('rng draws random.sample, which does not repeat: replace=True cannot go with it')
            if idx is not None:
                raise ValueError('idx and rng exclude each other: idx is a pure gather')
            if not isinstance(rng, PyRandom):
                raise TypeError('rng must be a PyRandom (got %s)' % type(rng).__name__)
        if idx is None:
            if batch_size is None:
                raise ValueError('sample needs batch_size or idx')
            B = int(batch_size)
            if B < 1 or (not replace and B > self.capacity):
                raise ValueError('batch_size must be in [1, capacity] (got %d)' % B)
            if rng is not None:
                check(self._L.snake_pyrandom_plan(1, B, self.capacity), self._L)    # ValueError before any device work
            dev = self._own_device()
            if rng is not None:
                idx = rng.sample(self.count, self.capacity, B, stream=stream)
            elif replace:
                size = self.size()
                u = torch.rand(B, device=dev, generator=generator, dtype=torch.float64)
                idx = torch.minimum((u * size).to(torch.int64), size - 1)
            else:
                size = self.size()
                keys = torch.rand(self.capacity, device=dev, generator=generator)
                held = torch.arange(self.capacity, device=dev) < size
                idx = torch.topk(keys.masked_fill_(~held, -1.0), B).indices
        else:
            if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64 or idx.dim() != 1:
                raise TypeError('idx must be an int64 (B,) tensor')
            dev = self._own_device()
            check_on('idx', idx, dev, 'ReplayBuffer')
            idx = idx.contiguous()
        B = idx.shape[0]
        S, h, w, c = self.obs_shape
        if format == 'uint8':
            state = torch.empty((B, h, w, c), dtype=torch.uint8, device=dev)
        else:
            state = torch.empty((B, c, h, w), dtype=torch.float32, device=dev)
        next_state = torch.empty_like(state)
        action = torch.empty(B, dtype=torch.int64, device=dev)
        reward = torch.empty(B, dtype=torch.float32, device=dev)
        done = torch.empty(B, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(self._L.snake_replay_gather(
                ctypes.byref(self.cfg), ctypes.byref(self._rings), ptr(idx), B, FORMATS[format], ptr(state),
                ptr(next_state), ptr(action), ptr(reward), ptr(done), stream_ptr(dev)), self._L)
        self._keep_idx = idx
        return state, action, reward, next_state, done

    def __len__(self):
        """Transitions held. Reads the device counter: this syncs with the host."""
        if self.count is None:
            return 0
        return min(int(self.count.item()), self.capacity)

    def clear(self):
        """Forget every transition (the counter goes back to 0; no sync)."""
        if self.count is not None:
            self.count.zero_()


class Collector:
    """The vector form of the inner loop of Trainer.train (train_dqn.py:277-308):
    epsilon-greedy actions from `qnet`, env.step, and one push per step into
    `buffer`, all on the device.

    env: a SnakeVecEnv with all-done auto-reset; buffer: a ReplayBuffer of
    env.obs_shape. The collector resets the env and keeps the observations,
    the per-snake "already done" mask (done & ~episode_done[:, None], the rule
    of evaluate()) and a per-env int32 episode-step counter across run() calls.

    Two deviations from the reference, both from the env's auto-reset:
      - the next_state of an episode's last transitions is the next episode's
        first observation; those transitions all have done = 1, so the TD
        target (1 - done) * gamma * max Q(next_state) never reads it;
      - an episode cut by the env's max_episode_steps is stored with done = 1,
        where the reference's MAX_STEPS_PER_EPISODE cut stores done = 0."""

    def __init__(self, env, buffer):
        if tuple(buffer.obs_shape) != tuple(env.obs_shape):
            raise ValueError('buffer obs_shape %s is not the env\'s %s' % (buffer.obs_shape, env.obs_shape))
        torch = _torch()
        self.env, self.buffer = env, buffer
        N, S = env.num_envs, env.num_snakes
        self.obs = env.reset()
        self.mask = torch.zeros((N, S), dtype=torch.bool, device=env.device)
        self.step_index = torch.zeros(N, dtype=torch.int32, device=env.device)

    def run(self, qnet, steps, epsilon=0.0, generator=None, rng=None):
        """`steps` env steps. qnet: any callable from uint8 (N*S, h, w, C)
        observations to float (N*S, 3) Q-values. Per snake u < epsilon gives a
        uniform action in {0, 1, 2}, otherwise the argmax; a snake that is
        already done gets action 0 (:281-285) and stores nothing. No host sync
        inside the loop. generator: a torch.Generator of the env's device.
        rng: a PyRandom with at least num_envs streams. Q-values then become
        actions in one launch (snake_pyrandom_act) that reproduces the draws of
        Agent.select_action (:163-165) from env e's stream e: per live snake in
        slot order random.random() < epsilon -- drawn whatever epsilon is, as
        the reference does while training -- and below it
        random.randrange(A); a snake that is already done draws nothing. With
        num_envs=1 and the stream seeded like random.seed(s) these are the
        reference trainer's own choices for the same Q-values; the first
        maximal Q-value wins a tie, as torch's argmax does."""
        torch = _torch()
        env, buf = self.env, self.buffer
        N, S = env.num_envs, env.num_snakes
        _, h, w, c = env.obs_shape
        dev = env.device
        eps = float(epsilon)
        if rng is not None:
            if not isinstance(rng, PyRandom):
                raise TypeError('rng must be a PyRandom (got %s)' % type(rng).__name__)
            if rng.n < N:
                raise ValueError('%d envs need %d streams, this PyRandom has %d' % (N, N, rng.n))
        for _ in range(int(steps)):
            obs = self.obs
            q = qnet(obs.view(N * S, h, w, c))
            if rng is not None:
                actions = rng.act(q.reshape(N * S, -1), S, eps, skip=self.mask)
            else:
                greedy = q.reshape(N, S, -1).argmax(dim=2)
                if eps > 0.0:
                    u = torch.rand((N, S), device=dev, generator=generator)
                    rnd = torch.randint(0, 3, (N, S), device=dev, generator=generator)
                    greedy = torch.where(u < eps, rnd, greedy)
                actions = greedy.masked_fill(self.mask, 0).to(torch.int8)
            next_obs, rewards, done, info = env.step(actions)
            ended = info['episode_done']
            buf.push(obs, next_obs, actions, rewards, done, skip=self.mask, step=self.step_index)
            self.obs = next_obs
            self.mask = done & ~ended[:, None]
            self.step_index = torch.where(ended, torch.zeros_like(self.step_index), self.step_index + 1)
