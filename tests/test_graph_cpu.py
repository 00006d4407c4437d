"""CPU checks of the graph observation's rule (no GPU needed): the numpy
restatement (tests/graph_ref.py) reproduces every recorded call of the
reference's GraphSnakeEnv._process_obs (tests/golden/graph_calls.npz) exactly,
the fixture covers what it has to, the library's weight table is numpy's in
both arithmetic modes, and the host-side argument checks of snake_graph_plan,
snake_graph_obs, GraphObs, GraphVecEnv and make_graph_snake reject what they
should."""
import ctypes
import os

import numpy as np
import pytest

import graph_ref as R


@pytest.fixture(scope='module')
def native():
    from marlenv import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _native


@pytest.fixture(scope='module')
def calls():
    return R.load_calls()


@pytest.fixture(scope='module')
def restated(calls):
    return {name: R.graph_obs(c['obs'], c['heads'], c['dirs'], c['alive'], c['vr'], 'reference')
            for name, c in calls.items()}


def compacted(rows, alive):
    """(R, S, 5, C) rows by snake index -> the live rows first, zero padded (the fixture's layout)."""
    out = np.zeros_like(rows)
    for i in range(len(rows)):
        live = rows[i][alive[i] != 0]
        out[i, :len(live)] = live
    return out


def test_restatement_reproduces_the_reference(calls, restated):
    assert sorted(calls) == sorted(R.CONFIGS)
    for name, c in calls.items():
        rows, _ = restated[name]
        assert rows.dtype == np.float64
        got = compacted(rows, c['alive'])
        assert np.array_equal(got, c['rows']), name
        assert np.array_equal(c['n_alive'], c['alive'].sum(axis=1)), name
        # the env's return: the same rows cast to uint8 (which truncates)
        assert np.array_equal(got.astype(np.uint8), c['ret']), name


def test_fixture_covers_the_rule(calls, restated):
    shapes = {(c['h'], c['w'], c['vr']) for c in calls.values()}
    assert any(h != w and vr == 0 for h, w, vr in shapes)          # a rectangular full map
    assert any(c['vr'] and c['C'] > 8 for c in calls.values()) and any(c['S'] == 1 for c in calls.values())
    dirs_seen = set()
    ends = {(kind, how): 0 for kind in ('axis', 'diag') for how in (R.WALL, R.FULL)}
    above_one = between = truncated = 0
    for name, c in calls.items():
        assert 50 <= len(c['n_alive']) <= 70, name
        rows, ended = restated[name]
        live = c['alive'] != 0
        dirs_seen |= set(c['dirs'][live].tolist())
        assert not (ended == R.CLIPPED).any(), name         # no ray leaves the observation
        for how in (R.WALL, R.FULL):
            ends['axis', how] += int((ended[:, :, :3][live] == how).sum())
            ends['diag', how] += int((ended[:, :, 3:][live] == how).sum())
        above_one += int((c['rows'] > 1).sum())
        between += int(((c['rows'] > 0) & (c['rows'] < 1)).sum())
        truncated += int((c['ret'] != c['rows']).sum())
        if c['S'] > 1:
            # a dead snake below a live one: the reference's counter then differs from the index
            shifted = [any(a[s] and not a[:s].all() for s in range(c['S'])) for a in c['alive']]
            assert sum(shifted) >= 20, (name, sum(shifted))
            own, _ = R.graph_obs(c['obs'], c['heads'], c['dirs'], c['alive'], c['vr'], 'own')
            assert not np.array_equal(own, rows), name      # ... and the two sources differ
    assert dirs_seen == {0, 1, 2, 3}
    for key, n in ends.items():
        assert n >= 1, (key, n)
    assert above_one >= 1 and between >= 1 and truncated >= 1


def test_trajectories_contain_an_all_dead_record():
    for name, t in R.load_trajectories().items():
        assert t['events'][0] == -1 and len(t['events']) == len(t['obs']), name
        assert any(o.shape == (0,) for o in t['obs']), name
        steps = t['events'][t['events'] >= 0]
        assert np.array_equal(steps, np.arange(len(t['actions']))), name
        for o in t['obs']:
            assert o.dtype == np.uint8 and (o.shape == (0,) or o.shape[1:] == (5, 8 * t['kwargs']['frame_stack']))


def test_ray_steps_are_the_reference_trigonometry():
    """int(cos(angle + turn)), int(sin(angle + turn)) of graph_snake_env.py:63-66 for
    the four directions and the three turns (0, +pi/2, -pi/2)."""
    import math
    for d, (dr, dc) in enumerate(R.DIRS):
        angle = math.atan2(dc, dr)
        want = [(int(math.cos(angle + t)), int(math.sin(angle + t))) for t in (0.0, math.pi / 2, -math.pi / 2)]
        want += [(want[0][0] + want[1][0], want[0][1] + want[1][1]), (want[0][0] + want[2][0], want[0][1] + want[2][1])]
        assert list(R.ray_steps(d)) == want, d


def test_a_clipped_ray_ends_without_reading():
    """A head on the border heading out (records the env never writes): forward
    and both diagonals leave at once, the side rays run along the border."""
    obs = np.zeros((1, 1, 4, 6, 8), np.uint8)
    obs[0, 0, 0, :, 0] = 1
    obs[0, 0, 0, 3, 1] = 1
    rows, ended = R.graph_obs(obs, np.array([[[0, 2]]]), np.array([[0]]), np.array([[1]]), 0)
    assert ended[0, 0].tolist() == [R.CLIPPED, R.WALL, R.WALL, R.CLIPPED, R.CLIPPED]
    assert not rows[0, 0, [0, 3, 4]].any()
    assert rows[0, 0, 1, 0] == 1.0 and rows[0, 0, 2, 0] == 1.0 and rows[0, 0, 2, 1] == 1.0 and rows[0, 0, 1, 1] == 0.0


@pytest.mark.parametrize('f32', [0, 1])
def test_weight_table_is_numpys(native, f32):
    L = native.lib()
    for n in (1, 2, 5, 11, 64, 127):
        out = np.full((2, n), -1.0)
        assert L.snake_graph_weights(n, f32, out.ctypes.data_as(ctypes.c_void_p)) == 0
        assert np.array_equal(out, R.weights(n, bool(f32))), (n, f32)
    assert not np.array_equal(R.weights(5, True), R.weights(5, False))
    buf = np.zeros(2)
    for n in (0, 128, -1):
        assert L.snake_graph_weights(n, f32, buf.ctypes.data_as(ctypes.c_void_p)) == -2
    assert L.snake_graph_weights(1, f32, None) == -2


def test_plan_rejects(native):
    L = native.lib()
    G = native.GraphCfg
    assert L.snake_graph_plan(ctypes.byref(G(11, 11, 8, 4, 5, 0, 0))) == 0
    assert L.snake_graph_plan(ctypes.byref(G(255, 7, 128, 16, 0, 1, 1))) == 0
    assert L.snake_graph_plan(ctypes.byref(G(255, 255, 8, 1, 127, 0, 0))) == 0
    for cfg, msg in [
        (G(11, 11, 12, 4, 5, 0, 0), 'obs_c'), (G(11, 11, 0, 4, 5, 0, 0), 'obs_c'), (G(11, 11, 136, 4, 5, 0, 0), 'obs_c'),
        (G(11, 11, 8, 17, 5, 0, 0), 'num_snakes'), (G(11, 11, 8, 0, 5, 0, 0), 'num_snakes'),
        (G(11, 11, 8, 4, 4, 0, 0), 'vision_range 4'), (G(11, 13, 8, 4, 5, 0, 0), 'vision_range 5'),
        (G(11, 11, 8, 4, 128, 0, 0), 'vision_range'), (G(11, 11, 8, 4, -1, 0, 0), 'vision_range'),
        (G(256, 11, 8, 4, 0, 0, 0), 'obs_h'), (G(11, 0, 8, 4, 0, 0, 0), 'obs_h'),
        (G(11, 11, 8, 4, 5, 2, 0), 'source'), (G(11, 11, 8, 4, 5, 0, 2), 'out_f32'),
    ]:
        assert L.snake_graph_plan(ctypes.byref(cfg)) == -1, msg
        assert msg in L.snake_last_error().decode(), (msg, L.snake_last_error())
    assert L.snake_graph_plan(None) == -1


def test_call_rejects_bad_arguments_on_the_host(native):
    """Bad arguments return before any device work, so this runs without a GPU."""
    L = native.lib()
    buf = (ctypes.c_uint8 * 64)()
    P = ctypes.c_void_p
    a16 = (ctypes.addressof(buf) + 15) & ~15
    ok = native.GraphCfg(5, 5, 8, 2, 2, 0, 0)
    for cfg, obs, rec, out, n, rc, msg in [
        (native.GraphCfg(5, 5, 9, 2, 2, 0, 0), a16, a16, a16, 1, -1, 'obs_c'),
        (ok, None, a16, a16, 1, -2, 'NULL'), (ok, a16, None, a16, 1, -2, 'NULL'), (ok, a16, a16, None, 1, -2, 'NULL'),
        (ok, a16 + 4, a16, a16, 1, -2, 'aligned'), (ok, a16, a16 + 8, a16, 1, -2, 'aligned'),
        (ok, a16, a16, a16 + 8, 1, -2, 'aligned'),
        (ok, a16, a16, a16, -1, -2, 'num_envs'), (ok, a16, a16, a16, (1 << 26) + 1, -2, 'num_envs'),
        (native.GraphCfg(5, 5, 128, 16, 2, 0, 0), a16, a16, a16, 1 << 26, -2, '2^31'),
    ]:
        got = L.snake_graph_obs(ctypes.byref(cfg), P(obs) if obs else None, P(rec) if rec else None,
                                P(out) if out else None, n, None)
        assert got == rc, (msg, got)
        assert msg in L.snake_last_error().decode()
    assert L.snake_graph_obs(ctypes.byref(ok), P(a16), P(a16), P(a16), 0, None) == 0      # no envs: no launch


class FakeEnv:
    """What GraphObs reads of a SnakeVecEnv before any device work."""

    def __init__(self, obs_shape, vision_range=0, observer=0):
        self.obs_shape = obs_shape
        self.cfg = type('Cfg', (), dict(vision_range=vision_range, observer=observer))()


def test_graph_obs_rejects_before_any_device_work(native):
    import torch
    from marlenv import GraphObs
    g = GraphObs(FakeEnv((4, 11, 11, 8), 5))
    assert g.out_shape == (4, 5, 8) and g.cfg.source == 0 and g.cfg.out_f32 == 0
    g = GraphObs(FakeEnv((3, 9, 12, 16)), source='reference', dtype=torch.float32)
    assert (g.cfg.source, g.cfg.out_f32, g.cfg.vision_range) == (1, 1, 0)
    for env in (FakeEnv((4, 11, 11, 12), 5), FakeEnv((4, 11, 11, 136), 5),      # bad obs_c
                FakeEnv((4, 11, 11, 8), 4), FakeEnv((4, 9, 11, 8), 5),          # window / vision_range mismatch
                FakeEnv((17, 11, 11, 8), 5),                                    # S > 16
                FakeEnv((4, 11, 11, 8), 5, observer=1)):                        # human observer
        with pytest.raises(ValueError):
            GraphObs(env)
    with pytest.raises(ValueError, match='source'):
        GraphObs(FakeEnv((4, 11, 11, 8), 5), source='theirs')
    with pytest.raises(ValueError, match='dtype'):
        GraphObs(FakeEnv((4, 11, 11, 8), 5), dtype=torch.float16)


def test_env_constructors_reject_before_any_device_work():
    import torch
    from marlenv import GraphSnakeEnv, GraphVecEnv, make_graph_snake
    with pytest.raises(ValueError, match='human'):
        GraphVecEnv(8, observer='human')
    with pytest.raises(ValueError, match='human'):
        GraphSnakeEnv(observer='human')
    for n in (1, 8):
        with pytest.raises(ValueError, match='human'):
            make_graph_snake(num_envs=n, observer='human')
    with pytest.raises(ValueError, match='source'):
        GraphVecEnv(8, source='both')
    with pytest.raises(ValueError, match='dtype'):
        GraphVecEnv(8, dtype=torch.int32)


def test_the_env_id_is_still_refused_by_make_snake():
    """'SnakeGraph-v1' is served by make_graph_snake for now; the registry is as it was."""
    from marlenv.envs import REGISTRY, UNSUPPORTED
    assert sorted(REGISTRY) == ['Snake-v1', 'SnakeCoop-v1'] and UNSUPPORTED == {'SnakeGraph-v1'}
