#!/usr/bin/env python3
"""Golden fixture of the replay buffer: runs the REAL reference ReplayBuffer
and Transition (train_dqn.py:86-100) on the REAL reference SnakeEnv.

Run (only on the machine where the reference tree is available):

    python3 -B tests/golden/gen/make_replay_golden.py

train_dqn is imported as make_policy_golden.py imports it (-B keeps bytecode
out of the read-only tree; the modules it imports but the buffer never uses are
empty in-process stand-ins). The env is driven by the trainer's loop
(train_dqn.py:277-308) with random actions in place of the network: a snake
that is done gets action 0, a transition is pushed for every snake that was not
done before the step, a snake that dies before step EARLY_DEATH_THRESHOLD gets
the penalty added, and an episode ends when every snake is done or after
EPISODE_CAP steps. Written: tests/golden/replay_stream.npz

    shape                (S, h, w, C)
    capacity, early_death_steps, early_death_penalty
    obs, next_obs        np.packbits of the uint8 observations (0/1), T steps
    action               int8 (T, S)
    reward               float64 (T, S)      the env's rewards, before the penalty
    done                 uint8 (T, S)        the dones after the step
    mask                 uint8 (T, S)        the dones before the step
    step                 int32 (T,)          the step's index in its episode
    final_state, final_next_state   np.packbits of the deque's observations
    final_action int64, final_reward float32 (torch.tensor(..., dtype=float32),
    :238), final_done uint8                  the deque's contents, oldest first

(inputs and outputs only, no reference source). The run is also replayed
through tests/replay_ref.py, which must reproduce the deque.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(HERE, 'gymstub'), '/root/reference/marlenv', '/root/reference']
sys.path.append(os.path.dirname(OUT))      # tests/: replay_ref


def stand_in(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


import torch  # noqa: E402
import torch.utils  # noqa: E402

stand_in('neat')
stand_in('cv2')
torch.utils.tensorboard = stand_in('torch.utils.tensorboard', SummaryWriter=object)
import gym  # noqa: E402  (the offline stub)
gym.vector = stand_in('gym.vector', AsyncVectorEnv=object)
stand_in('marlenv.marlenv')
stand_in('marlenv.marlenv.wrappers', make_snake=None, RenderGUI=None)

import train_dqn  # noqa: E402
from marlenv.envs.snake_env import SnakeEnv  # noqa: E402
import replay_ref as R  # noqa: E402

ENV = dict(height=10, width=10, num_snakes=3)       # the default reward dict: float64 rewards like -0.501
CAPACITY = 97
EARLY_DEATH_THRESHOLD, EARLY_DEATH_PENALTY = 10, -1.0
EPISODE_CAP = 40
STEPS = 300
SEED = 3       # (a seed with episodes that reach the cap)


def main():
    rs = np.random.RandomState(SEED)
    np.random.seed(SEED)
    env = SnakeEnv(**ENV)
    S = ENV['num_snakes']
    memory = train_dqn.ReplayBuffer(CAPACITY)
    recs = []
    episodes = 0
    while len(recs) < STEPS:
        obs = env.reset()
        dones = [False] * S
        step = 0
        episodes += 1
        while not all(dones) and step < EPISODE_CAP and len(recs) < STEPS:
            actions = [0 if dones[i] else int(rs.randint(3)) for i in range(S)]
            next_obs, rewards, next_dones, _ = env.step(actions)
            for i in range(S):
                if not dones[i]:
                    r = rewards[i]
                    if next_dones[i] and step < EARLY_DEATH_THRESHOLD:
                        r += EARLY_DEATH_PENALTY
                    memory.push(obs[i], actions[i], r, next_obs[i], next_dones[i])
            recs.append(dict(obs=np.asarray(obs), next_obs=np.asarray(next_obs), action=np.array(actions, np.int8),
                             reward=np.array(rewards, np.float64), done=np.array(next_dones, np.uint8),
                             mask=np.array(dones, np.uint8), step=np.int32(step)))
            obs = next_obs
            dones = next_dones
            step += 1
    for r in recs:
        for k in ('obs', 'next_obs'):
            o8 = r[k].astype(np.uint8)
            assert np.array_equal(o8, r[k]) and o8.max() <= 1
            r[k] = o8
    shape = recs[0]['obs'].shape                        # (S, h, w, C)
    batch = train_dqn.Transition(*zip(*memory.buffer))
    final = dict(
        state=np.array(batch.state).astype(np.uint8), next_state=np.array(batch.next_state).astype(np.uint8),
        action=torch.tensor(batch.action, dtype=torch.long).numpy(),
        reward=torch.tensor(batch.reward, dtype=torch.float32).numpy(),
        done=torch.tensor(batch.done, dtype=torch.float32).numpy().astype(np.uint8))
    out = dict(shape=np.array(shape, np.int32), capacity=np.int64(CAPACITY),
               early_death_steps=np.int32(EARLY_DEATH_THRESHOLD), early_death_penalty=np.float64(EARLY_DEATH_PENALTY),
               obs=R.pack_obs(np.stack([r['obs'] for r in recs])),
               next_obs=R.pack_obs(np.stack([r['next_obs'] for r in recs])),
               final_state=R.pack_obs(final['state']), final_next_state=R.pack_obs(final['next_state']),
               final_action=final['action'], final_reward=final['reward'], final_done=final['done'])
    for k in ('action', 'reward', 'done', 'mask', 'step'):
        out[k] = np.stack([r[k] for r in recs])
    path = os.path.join(OUT, 'replay_stream.npz')
    np.savez_compressed(path, **out)

    # the restatement reproduces the deque
    d = R.load_stream(path)
    ref = R.RefReplay(d['capacity'], d['early_death'])
    R.replay_stream(d, ref.push)
    state, action, reward, nxt, done = ref.rows()
    assert len(ref) == len(memory) == CAPACITY
    assert np.array_equal(state, final['state']) and np.array_equal(nxt, final['next_state'])
    assert np.array_equal(action, final['action']) and np.array_equal(done, final['done'].astype(np.float32))
    assert reward.tobytes() == final['reward'].tobytes()
    stored = int((1 - out['mask']).sum())
    early = int(((out['done'] == 1) & (out['mask'] == 0) & (out['step'][:, None] < EARLY_DEATH_THRESHOLD)).sum())
    print('steps', len(recs), 'episodes', episodes, 'stored', stored, 'skipped', int(out['mask'].sum()),
          'early deaths', early, 'distinct rewards', sorted(set(out['reward'].reshape(-1).tolist())))
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 64 << 10


if __name__ == '__main__':
    main()
