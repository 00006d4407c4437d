#!/usr/bin/env python3
"""Golden fixture of the greedy opponent's rule: runs the REAL reference
GreedyEnemy.get_action (train_dqn.py) on the REAL reference SnakeEnv.

Run (container only -- /root/reference does not exist on the GPU box):

    python3 -B tests/golden/gen/make_greedy_golden.py

train_dqn is imported as it is, with the stand-in modules of
make_policy_golden.py (-B keeps bytecode out of the read-only tree). The one
thing replaced is the `random` that train_dqn sees: GreedyEnemy picks among
equally good moves with random.choice, and here choice(best) consumes a
recorded uint32 u and returns best[(u * len(best)) >> 32], the rule of
snake_greedy_actions (include/snake_env.h). Every snake of the env is a
GreedyEnemy; the agents' directions are cleared at every reset, so that unknown
directions occur. Written: tests/golden/greedy_calls.npz, per configuration <c>

    <c>_shape  (S, h, w)
    <c>_obs    np.packbits of the uint8 observations (0/1 values), (R, S*h*w)
    <c>_rnd    uint32 (R, S)             the random bits offered to each snake
    <c>_skip   uint8 (R, S)              the loop's dones
    <c>_din    int8 (R, S, 2)            directions in, (-128, -128) = None
    <c>_act    int8 (R, S)               actions out
    <c>_dout   int8 (R, S, 2)            directions out

one record per kept env step (inputs and outputs only, no reference source),
plus the configuration `crafted`: hand-made 5x5 observations through the same
get_action, for the branches a rollout does not reach (no head) or reaches
rarely. Every call is also checked against tests/greedy_ref.py; the kept
records are the episode starts and those of the rarer categories, filled up
with the others.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(HERE, 'gymstub'), '/root/reference/marlenv', '/root/reference']
sys.path.append(os.path.dirname(OUT))      # tests/: greedy_ref


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
import greedy_ref as R  # noqa: E402

UNKNOWN = -128
CONFIGS = [      # name, SnakeEnv kwargs, env steps to run, records to keep
    ('full20', dict(height=20, width=20, num_snakes=4, snake_length=5), 2500, 90),
    ('b12', dict(height=12, width=12, num_snakes=4, snake_length=3), 2500, 80),
    ('vr5', dict(height=20, width=20, num_snakes=4, snake_length=5, vision_range=5), 2500, 90),
    ('b10x14', dict(height=10, width=14, num_snakes=3, snake_length=4), 2500, 80),
]
EPISODE_CAPS = (40, 300)    # steps, alternating: many episode starts, and some long snakes
REWARDS = dict(fruit=1.0, kill=0.0, lose=0.0, win=0.0, time=0.0)
# rarer first: the order the kept records are filled in
RARITY = ((R.FRUIT_TIE, 32), (R.ALLDEAD, 16), (R.NOHEAD, 16), (R.N3, 8), (R.NOFRUIT, 4), (R.N2, 2))

CUR = {}


def recorded_choice(best):
    CUR['asked'] = True
    return best[(int(CUR['u']) * len(best)) >> 32]


train_dqn.random = types.SimpleNamespace(choice=recorded_choice)


def enc(d):
    return (UNKNOWN, UNKNOWN) if d is None else (int(d[0]), int(d[1]))


def call(agents, obs, rnd, dones):
    """One step's get_action calls; returns the record and checks it against greedy_ref."""
    S = len(agents)
    o8 = np.asarray(obs).astype(np.uint8)
    assert np.array_equal(o8, np.asarray(obs)) and o8.max() <= 1
    din = np.array([enc(a.current_direction) for a in agents], np.int8)
    skip = np.array(dones, np.uint8)
    actions, asked = [], []
    for i in range(S):
        CUR['u'], CUR['asked'] = rnd[i], False
        actions.append(0 if dones[i] else int(agents[i].get_action(obs[i])))
        asked.append(CUR['asked'])
    dout = np.array([enc(a.current_direction) for a in agents], np.int8)
    a_ref, d_ref, cat = R.greedy_actions(o8[None], rnd[None], skip[None], din[None])
    assert np.array_equal(a_ref[0], np.array(actions, np.int8)), (actions, a_ref)
    assert np.array_equal(d_ref[0], dout), (dout, d_ref)
    # random.choice is asked exactly where the rule reads rnd
    assert asked == [bool(c & (R.N1 | R.N2 | R.N3)) for c in cat[0]]
    return dict(obs=np.packbits(o8.reshape(-1)), rnd=rnd, skip=skip, din=din, act=np.array(actions, np.int8),
                dout=dout, cat=cat[0]), actions


def draw_rnd(rs, S):
    """32 random bits per snake; now and then the extremes."""
    u = rs.randint(0, 2 ** 32, size=S, dtype=np.uint64).astype(np.uint32)
    edge = rs.randint(8, size=S)
    u[edge == 0] = 0
    u[edge == 1] = 0xFFFFFFFF
    return u


def pack(name, S, h, w, recs):
    out = {name + '_shape': np.array([S, h, w], np.int32)}
    for k in ('obs', 'rnd', 'skip', 'din', 'act', 'dout'):
        out[name + '_' + k] = np.stack([r[k] for r in recs])
    cats = np.stack([r['cat'] for r in recs])
    print(name, 'kept', len(recs), 'unknown dirs', int((out[name + '_din'][:, :, 0] == UNKNOWN).sum()),
          {v: int(((cats & k) != 0).sum()) for k, v in R.CATEGORY_NAMES.items()})
    return out


def run(name, kw, steps, keep, seed):
    rs = np.random.RandomState(seed)
    np.random.seed(seed)
    env = SnakeEnv(reward_dict=REWARDS, **kw)
    S = kw['num_snakes']
    agents = [train_dqn.GreedyEnemy(i) for i in range(S)]
    recs = []
    obs, dones, t_ep, episode = env.reset(), [False] * S, 0, 0
    for _ in range(steps):
        try:
            rec, actions = call(agents, obs, draw_rnd(rs, S), dones)
        except AssertionError:
            print('mismatch at', name, len(recs))
            raise
        rec['first'] = t_ep == 0
        recs.append(rec)
        obs, _, dones, _ = env.step(actions)
        t_ep += 1
        if all(dones) or t_ep >= EPISODE_CAPS[episode % 2]:
            obs, dones, t_ep, episode = env.reset(), [False] * S, 0, episode + 1
            for a in agents:
                a.current_direction = None
    cats = np.stack([r['cat'] for r in recs])
    print(name, 'steps', len(recs), 'all calls',
          {v: int(((cats & k) != 0).sum()) for k, v in R.CATEGORY_NAMES.items()})

    def rarity(i):
        return sum(wt * int(((recs[i]['cat'] & c) != 0).any()) for c, wt in RARITY)
    starts = [i for i in range(len(recs)) if recs[i]['first']][:keep // 4]
    rest = sorted((i for i in range(len(recs)) if i not in starts), key=lambda i: (-rarity(i), i))
    pick = sorted(starts + rest[:keep - len(starts)])
    h, w = np.asarray(obs).shape[1:3]
    return pack(name, S, h, w, [recs[i] for i in pick])


def crafted():
    """5x5 observations of one snake: (cells as {(y, x): channel}, direction in, u)."""
    cases = [
        ({}, None, 0),                                                      # no head, direction stays unknown
        ({(1, 1): 1}, (0, 1), 7),                                           # no head, direction stays (0, 1)
        # fruits at (0, 2) and (2, 0), both 2 away from the head at (2, 2) heading right:
        # the first in row-major order makes `left` (up) the one best move, the last would make none better
        ({(2, 2): 5, (0, 2): 1, (2, 0): 1}, (0, 1), 0xFFFFFFFF),
        # fruit left and right of the head in its row, the head heading up: left wins
        ({(2, 2): 5, (2, 0): 1, (2, 4): 1}, (-1, 0), 0),
        # walled in on three sides, the body below: action 0, the direction (-1, 0) is stored
        ({(2, 2): 5, (3, 2): 6, (1, 2): 0, (2, 1): 3, (2, 3): 4}, None, 123),
        # head in the corner, unknown direction, no body: (-1, 0), forward is outside
        ({(0, 0): 5, (4, 4): 1}, None, 0x80000000),
        # tail to the right gives direction (0, -1); no fruit: three moves tie at 0
        ({(2, 2): 5, (2, 3): 7}, None, 0x55555556),
        ({(2, 2): 5, (2, 3): 7}, None, 0xAAAAAAAA),
        ({(2, 2): 5, (2, 3): 7}, None, 0xFFFFFFFF),
    ]
    recs = []
    for cells, d, u in cases:
        o = np.zeros((1, 5, 5, 8), np.float32)
        for (y, x), ch in cells.items():
            o[0, y, x, ch] = 1
        agent = train_dqn.GreedyEnemy(0)
        agent.current_direction = d
        recs.append(call([agent], o, np.array([u], np.uint32), [False])[0])
    return pack('crafted', 1, 5, 5, recs)


def main():
    out = {}
    for j, (name, kw, steps, keep) in enumerate(CONFIGS):
        out.update(run(name, kw, steps, keep, 200 + j))
    out.update(crafted())
    path = os.path.join(OUT, 'greedy_calls.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
