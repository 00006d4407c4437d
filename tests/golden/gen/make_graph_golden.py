#!/usr/bin/env python3
"""Golden fixture of the graph observation: runs the REAL reference
GraphSnakeEnv (marlenv/envs/graph_snake_env.py) with random actions and records
every _process_obs call.

Run (container only -- /root/reference does not exist on the GPU box):

    python3 -B tests/golden/gen/make_graph_golden.py

The env is imported as it is over the offline gym stub next to this file (-B
keeps bytecode out of the read-only tree). _process_obs is wrapped: its
argument (the S per-snake observations), the snakes' heads, directions and
alive flags at the call, and its float64 return are recorded, and every call
is also checked against tests/graph_ref.py with source='reference'. Written:
tests/golden/graph_calls.npz (inputs and outputs only, no reference source),
per configuration <c>

    <c>_shape    (S, h, w, C, vision_range or 0)
    <c>_obs      np.packbits of the uint8 observations (0/1 values), (R, ceil(S*h*w*C / 8))
    <c>_heads    uint8 (R, S, 2)           head row, column
    <c>_dirs     uint8 (R, S)              0 UP, 1 RIGHT, 2 DOWN, 3 LEFT
    <c>_alive    uint8 (R, S)
    <c>_rows     float64 (R, S, 5, C)      _process_obs' return: the live snakes' rows first, zero padded
    <c>_n_alive  int32 (R,)
    <c>_ret      uint8 (R, S, 5, C)        the same as the env returned it (cast to uint8)

and one short whole rollout for the single-env class

    <c>_tkw      (height, width, num_snakes, snake_length, vision_range or 0, frame_stack)
    <c>_tseed    np.random.seed before the env is made
    <c>_tact     int8 (T, S)               the steps' actions
    <c>_tevents  int32 (E,)                -1 = reset(), t = step(_tact[t]); reset() follows an all-done step
    <c>_tcount   int32 (E,)                rows of the event's returned array (0: shape (0,))
    <c>_tobs     uint8, the returned arrays' bytes one after another

The kept records are those with a dead snake below a live one first, then the
others evenly over the run.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(HERE, 'gymstub'), '/root/reference/marlenv']
sys.path.append(os.path.dirname(OUT))      # tests/: graph_ref

from marlenv.envs.graph_snake_env import GraphSnakeEnv  # noqa: E402
import graph_ref as R  # noqa: E402

CONFIGS = [      # name (graph_ref.CONFIGS), GraphSnakeEnv kwargs, env steps to run
    ('b8', dict(height=8, width=8, num_snakes=3), 2500),
    ('r9x12fs2', dict(height=9, width=12, num_snakes=4, frame_stack=2), 2500),
    ('r8x10vr2fs2', dict(height=8, width=10, num_snakes=3, vision_range=2, frame_stack=2), 2500),
    ('b20vr5', dict(height=20, width=20, num_snakes=4, snake_length=5, vision_range=5), 2500),
    ('b20vr5fs2', dict(height=20, width=20, num_snakes=4, vision_range=5, frame_stack=2), 2500),
    ('r7x11s1', dict(height=7, width=11, num_snakes=1), 600),
]
KEEP = 60
DIR_CODE = {d: i for i, d in enumerate(R.DIRS)}
CALLS = []


class Recorded(GraphSnakeEnv):
    def _process_obs(self, obs):
        out = super()._process_obs(obs)
        o = np.stack([np.asarray(x) for x in obs])
        o8 = o.astype(np.uint8)
        assert np.array_equal(o8, o) and o8.max() <= 1
        assert out.dtype == np.float64
        CALLS.append(dict(
            obs=o8,
            heads=np.array([s.head_coord for s in self.snakes], np.int64),
            dirs=np.array([DIR_CODE[s.direction.value] for s in self.snakes], np.uint8),
            alive=np.array([s.alive for s in self.snakes], np.uint8),
            out=out))
        return out


def check(c, vr):
    """The restatement on one call, exactly; returns how the live snakes' rays ended."""
    want, ended = R.graph_obs(c['obs'][None], c['heads'][None], c['dirs'][None], c['alive'][None], vr, 'reference')
    got = R.compact(want[0], c['alive'])
    assert got.shape == c['out'].shape and np.array_equal(got, c['out']), (got.shape, c['out'].shape)
    assert not (ended == R.CLIPPED).any()
    return ended[0]


def run(name, kw, steps, seed):
    del CALLS[:]
    S, vr = kw['num_snakes'], kw.get('vision_range') or 0
    rs = np.random.RandomState(seed)
    np.random.seed(seed)
    env = Recorded(**kw)
    rets = [env.reset()]
    tact, tevents, tret = [], [-1], [rets[0]]
    all_dead, t_end = 0, None
    for t in range(steps):
        a = rs.randint(0, 3, size=S)
        obs, _, dones, _ = env.step(a)
        rets.append(obs)
        if t_end is None:
            tact.append(a.astype(np.int8))
            tevents.append(t)
            tret.append(obs)
        if all(dones):
            all_dead += 1
            obs = env.reset()
            rets.append(obs)
            if t_end is None:
                tevents.append(-1)
                tret.append(obs)
                if all_dead == 2:        # the rollout: two whole episodes
                    t_end = t
    assert len(rets) == len(CALLS) and t_end is not None
    C = CALLS[0]['obs'].shape[-1]
    for c, ret in zip(CALLS, rets):
        check(c, vr)
        assert ret.dtype == np.uint8 and np.array_equal(ret, c['out'].astype(np.uint8))
        assert ret.shape == ((int(c['alive'].sum()), 5, C) if c['alive'].any() else (0,))
        if c['alive'].any():
            assert (c['heads'][c['alive'] != 0] < 256).all()
    assert any(len(r) == 0 for r in tret)

    def shifted(c):      # a dead snake below a live one
        al = c['alive']
        return any(al[s] and not al[:s].all() for s in range(S))
    first = [i for i, c in enumerate(CALLS) if shifted(c)]
    first = first[::max(1, len(first) // (KEEP // 2))][:KEEP // 2]
    rest = [i for i in range(len(CALLS)) if i not in first]
    rest = rest[::max(1, len(rest) // (KEEP - len(first)))][:KEEP - len(first)]
    pick = sorted(first + rest)
    recs = [CALLS[i] for i in pick]
    h, w = recs[0]['obs'].shape[1:3]

    def padded(x, dtype):
        p = np.zeros((S, 5, C), dtype)
        if len(x):
            p[:len(x)] = x
        return p
    out = {
        name + '_shape': np.array([S, h, w, C, vr], np.int32),
        name + '_obs': np.stack([np.packbits(c['obs'].reshape(-1)) for c in recs]),
        name + '_heads': np.stack([np.clip(c['heads'], 0, 255).astype(np.uint8) for c in recs]),
        name + '_dirs': np.stack([c['dirs'] for c in recs]),
        name + '_alive': np.stack([c['alive'] for c in recs]),
        name + '_rows': np.stack([padded(c['out'], np.float64) for c in recs]),
        name + '_n_alive': np.array([int(c['alive'].sum()) for c in recs], np.int32),
        name + '_ret': np.stack([padded(c['out'].astype(np.uint8), np.uint8) for c in recs]),
        name + '_tkw': np.array([kw['height'], kw['width'], S, kw.get('snake_length', 3), vr,
                                 kw.get('frame_stack', 1)], np.int32),
        name + '_tseed': np.array(seed, np.int64),
        name + '_tact': np.stack(tact),
        name + '_tevents': np.array(tevents, np.int32),
        name + '_tcount': np.array([len(r) for r in tret], np.int32),
        name + '_tobs': np.concatenate([r.reshape(-1) for r in tret]),
    }
    print(name, 'calls', len(CALLS), 'kept', len(recs), 'shifted', sum(shifted(c) for c in recs),
          'rollout events', len(tevents), 'all-dead', sum(len(r) == 0 for r in tret))
    return out


def main():
    assert [c[0] for c in CONFIGS] == list(R.CONFIGS)
    out = {}
    for j, (name, kw, steps) in enumerate(CONFIGS):
        out.update(run(name, kw, steps, 300 + j))
    path = os.path.join(OUT, 'graph_calls.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
