#!/usr/bin/env python3
"""Golden fixture of the safe-action rule: runs the REAL reference
DQN_Evaluator.get_action (train_dqn.py) on the REAL reference SnakeEnv.

Run (container only -- /root/reference does not exist on the GPU box):

    python3 -B tests/golden/gen/make_policy_golden.py

train_dqn is imported as it is (-B keeps bytecode out of the read-only tree);
the modules it imports but the evaluator never uses (neat, cv2, tensorboard,
gym.vector, the marlenv.marlenv wrappers) are empty in-process stand-ins. The
evaluator's model is a callable returning recorded Q-values, and the reference
SnakeEnv is driven by the body of the evaluator's own loop (train_dqn.py:
625-649). Written: tests/golden/policy_calls.npz, per configuration <c>

    <c>_shape  (S, h, w)
    <c>_obs    np.packbits of the uint8 observations (0/1 values), (R, S*h*w)
    <c>_q      float32 (R, S, 3)         the model's Q-values
    <c>_skip   uint8 (R, S)              the loop's dones
    <c>_din    int8 (R, S, 2)            directions in, (-128, -128) = None
    <c>_act    int8 (R, S)               actions out
    <c>_dout   int8 (R, S, 2)            directions out

one record per kept env step (inputs and outputs only, no reference source).
Every step is also checked against tests/policy_ref.py; the kept records are
the episode starts (unknown directions) and those in which a rarer rule
decided, filled up with the others.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(HERE, 'gymstub'), '/root/reference/marlenv', '/root/reference']
sys.path.append(os.path.dirname(OUT))      # tests/: policy_ref


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
import policy_ref as R  # noqa: E402

UNKNOWN = -128
CONFIGS = [      # name, SnakeEnv kwargs, env steps to run, records to keep
    ('full20', dict(height=20, width=20, num_snakes=4, snake_length=5), 2500, 90),
    ('b12', dict(height=12, width=12, num_snakes=4, snake_length=3), 2500, 80),
    ('vr5', dict(height=20, width=20, num_snakes=4, snake_length=5, vision_range=5), 2500, 90),
    ('b10x14', dict(height=10, width=14, num_snakes=3, snake_length=4), 2500, 80),
]
EPISODE_CAPS = (40, 300)    # steps, alternating: many episode starts, and some long snakes
REWARDS = dict(fruit=1.0, kill=0.0, lose=0.0, win=0.0, time=0.0)


def draw_q(rs, S):
    """Q-values with frequent ties: half the steps from a few half-integers."""
    if rs.randint(2):
        return (rs.randint(-2, 3, size=(S, 3)) / 2).astype(np.float32)
    return rs.randn(S, 3).astype(np.float32)


def run(name, kw, steps, keep, seed):
    rs = np.random.RandomState(seed)
    np.random.seed(seed)
    env = SnakeEnv(reward_dict=REWARDS, **kw)
    S = kw['num_snakes']
    ev = train_dqn.DQN_Evaluator(train_dqn.Config, train_dqn.DQN)
    cur = {}
    ev.model = lambda x: torch.from_numpy(cur['q'][None].copy())
    recs = []
    obs, dones, dirs, t_ep, episode = env.reset(), [False] * S, [None] * S, 0, 0
    for _ in range(steps):
        o8 = np.asarray(obs).astype(np.uint8)
        assert np.array_equal(o8, np.asarray(obs)) and o8.max() <= 1
        q = draw_q(rs, S)
        din = np.array([(UNKNOWN, UNKNOWN) if d is None else d for d in dirs], np.int8)
        skip = np.array(dones, np.uint8)
        # ---- the evaluator's loop body (train_dqn.py:625-646)
        actions, occupied = [], set()
        for i in range(S):
            if dones[i]:
                actions.append(0)
                continue
            cur['q'] = q[i]
            act, new_dir, next_pos = ev.get_action(obs[i], dirs[i], occupied)
            actions.append(act)
            dirs[i] = new_dir
            if next_pos is not None:
                occupied.add(next_pos)
        dout = np.array([(UNKNOWN, UNKNOWN) if d is None else d for d in dirs], np.int8)
        a_ref, d_ref, rule = R.safe_actions(o8[None], q[None], skip[None], din[None])
        assert np.array_equal(a_ref[0], np.array(actions, np.int8)), (name, len(recs))
        assert np.array_equal(d_ref[0], dout), (name, len(recs))
        recs.append(dict(obs=np.packbits(o8.reshape(-1)), q=q, skip=skip, din=din,
                         act=np.array(actions, np.int8), dout=dout, rule=rule[0], first=t_ep == 0))
        obs, _, dones, _ = env.step(actions)
        t_ep += 1
        if all(dones) or t_ep >= EPISODE_CAPS[episode % 2]:
            obs, dones, dirs, t_ep, episode = env.reset(), [False] * S, [None] * S, 0, episode + 1
    # keep: a quarter episode starts, then the records with the rarer rules first
    def rarity(i):
        return sum(wt * int((recs[i]['rule'] == r).any()) for r, wt in
                   ((R.FILL, 8), (R.NEAR_HEAD, 4), (R.OCCUPIED, 2), (R.DEADLY_CELL, 1)))
    starts = [i for i in range(len(recs)) if recs[i]['first']][:keep // 4]
    rest = sorted((i for i in range(len(recs)) if i not in starts), key=lambda i: (-rarity(i), i))
    pick = sorted(starts + rest[:keep - len(starts)])
    h, w = np.asarray(obs).shape[1:3]
    out = {name + '_shape': np.array([S, h, w], np.int32)}
    for k in ('obs', 'q', 'skip', 'din', 'act', 'dout'):
        out[name + '_' + k] = np.stack([recs[i][k] for i in pick])
    rules = np.stack([recs[i]['rule'] for i in pick])
    print(name, 'steps', len(recs), 'kept', len(pick), 'unknown dirs',
          int((out[name + '_din'][:, :, 0] == UNKNOWN).sum()),
          {R.RULE_NAMES[r]: int((rules == r).sum()) for r in range(8)})
    return out


def main():
    out = {}
    for j, (name, kw, steps, keep) in enumerate(CONFIGS):
        out.update(run(name, kw, steps, keep, 100 + j))
    path = os.path.join(OUT, 'policy_calls.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
