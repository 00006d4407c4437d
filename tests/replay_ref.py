"""numpy-and-deque restatement of the replay buffer (include/snake_env.h,
snake_replay_push / snake_replay_gather), written from the rules: the yardstick
of the replay tests.

RefReplay.push() takes one env step's arrays on the host and appends, in (env,
snake) order, one (state, action, reward, next_state, done) tuple per snake
whose skip byte is zero to a collections.deque(maxlen=capacity); rows() turns
logical indices (0 the oldest) into the five arrays a sample returns.
"""
import collections
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

NAMES = ('obs', 'next_obs', 'actions', 'rewards', 'done', 'skip', 'step')     # push()'s arguments, in order


class RefReplay:
    def __init__(self, capacity, early_death=None):
        self.buffer = collections.deque(maxlen=int(capacity))
        self.early_death = early_death      # None or (steps, penalty)
        self.count = 0                      # transitions ever stored

    def push(self, obs, next_obs, actions, rewards, done, skip=None, step=None):
        """obs, next_obs: uint8 (N, S, h, w, C); actions, rewards (float64),
        done, skip: (N, S); step: (N,) or None."""
        N, S = np.asarray(actions).shape
        for n in range(N):
            for s in range(S):
                if skip is not None and skip[n][s]:
                    continue
                r = np.float64(rewards[n][s])
                d = bool(done[n][s])
                if d and step is not None and self.early_death is not None and int(step[n]) < self.early_death[0]:
                    r = r + np.float64(self.early_death[1])
                self.buffer.append((np.array(obs[n][s], np.uint8), int(actions[n][s]), np.float32(r),
                                    np.array(next_obs[n][s], np.uint8), d))
                self.count += 1

    def __len__(self):
        return len(self.buffer)

    def rows(self, idx=None, format='uint8'):
        """(state, action int64, reward float32, next_state, done float32) of the
        logical indices idx (all of them when None). Nonzero observation bytes
        read back as 1."""
        idx = range(len(self.buffer)) if idx is None else [int(i) for i in idx]
        rec = [self.buffer[i] for i in idx]
        shape = rec[0][0].shape if rec else (0, 0, 0)
        state = np.array([r[0] for r in rec], np.uint8).reshape((len(rec),) + shape)
        nxt = np.array([r[3] for r in rec], np.uint8).reshape((len(rec),) + shape)
        state, nxt = (state != 0).astype(np.uint8), (nxt != 0).astype(np.uint8)
        if format == 'float32':
            state = np.ascontiguousarray(state.transpose(0, 3, 1, 2)).astype(np.float32)
            nxt = np.ascontiguousarray(nxt.transpose(0, 3, 1, 2)).astype(np.float32)
        return (state, np.array([r[1] for r in rec], np.int64), np.array([r[2] for r in rec], np.float32),
                nxt, np.array([r[4] for r in rec], np.float32))


def pack_obs(obs):
    """0/1 uint8 observations -> np.packbits of the flattened array."""
    o = np.asarray(obs, np.uint8)
    assert o.max(initial=0) <= 1
    return np.packbits(o.reshape(-1))


def unpack_obs(bits, shape):
    n = int(np.prod(shape))
    return np.unpackbits(bits)[:n].reshape(shape)


def load_stream(path=None):
    """tests/golden/replay_stream.npz (written by tests/golden/gen/make_replay_golden.py)
    as a dict: the recorded steps of the reference's training loop -- obs and
    next_obs (T, S, h, w, 8), action, reward (float64), done, mask (the snakes
    done before the step), step (T,) -- its settings, and the reference deque's
    final contents (final_*)."""
    z = np.load(path or os.path.join(GOLDEN, 'replay_stream.npz'), allow_pickle=False)
    S, h, w, c = (int(v) for v in z['shape'])
    T = z['action'].shape[0]
    d = {k: z[k] for k in ('action', 'reward', 'done', 'mask', 'step', 'final_action', 'final_reward', 'final_done')}
    d['obs'] = unpack_obs(z['obs'], (T, S, h, w, c))
    d['next_obs'] = unpack_obs(z['next_obs'], (T, S, h, w, c))
    K = d['final_action'].shape[0]
    d['final_state'] = unpack_obs(z['final_state'], (K, h, w, c))
    d['final_next_state'] = unpack_obs(z['final_next_state'], (K, h, w, c))
    d['capacity'] = int(z['capacity'])
    d['early_death'] = (int(z['early_death_steps']), float(z['early_death_penalty']))
    return d


def replay_stream(d, buf_push):
    """Feed the recorded steps, one push per step (N = 1), to buf_push(obs,
    next_obs, actions, rewards, done, skip, step) as numpy arrays."""
    for t in range(d['action'].shape[0]):
        buf_push(d['obs'][t][None], d['next_obs'][t][None], d['action'][t][None].astype(np.int8),
                 d['reward'][t][None], d['done'][t][None].astype(np.uint8), d['mask'][t][None].astype(np.uint8),
                 d['step'][t:t + 1].astype(np.int32))


def random_step(rs, N, S, h, w, C, p_skip=0.3):
    """One env step's arrays: 0/1 observations, float64 rewards that float32
    rounds, random dones, skip masks and episode steps around the threshold."""
    return dict(obs=rs.randint(0, 2, size=(N, S, h, w, C)).astype(np.uint8),
                next_obs=rs.randint(0, 2, size=(N, S, h, w, C)).astype(np.uint8),
                actions=rs.randint(0, 3, size=(N, S)).astype(np.int8), rewards=rs.randn(N, S),
                done=(rs.random_sample((N, S)) < 0.4).astype(np.uint8),
                skip=(rs.random_sample((N, S)) < p_skip).astype(np.uint8),
                step=rs.randint(0, 20, size=N).astype(np.int32))


def push_both(torch, buf, ref, x):
    """The same step into the device buffer and the restatement."""
    buf.push(**{k: None if x.get(k) is None else torch.from_numpy(x[k]).cuda() for k in NAMES})
    ref.push(*(x.get(k) for k in NAMES))
