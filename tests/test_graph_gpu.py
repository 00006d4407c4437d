"""The graph-observation kernel (snake_graph_obs, graph_kernels.hip) against the
reference's recorded _process_obs calls and the numpy restatement
(tests/graph_ref.py): every comparison exact (np.array_equal on float64) -- the
sums are of at most 127 weights built on the host in the reference's own
arithmetic and added in its order without contraction, so there is nothing to
tolerate. GraphSnakeEnv replays the reference's recorded rollouts."""
import ctypes

import numpy as np
import pytest

import graph_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), 'needs the GPU'
    return torch


@pytest.fixture(scope='module')
def calls():
    return R.load_calls()


def records(heads, dirs, alive):
    """Snake records int32 (N, S, 4) as k_logic packs them (SnakeVecEnv.snake_table):
    word 0 = head row | head column << 8, word 1 = direction | alive << 8. The
    tail and the ring words, which the kernel does not read, get a pattern."""
    heads, dirs, alive = (np.asarray(x).astype(np.int64) for x in (heads, dirs, alive))
    rec = np.empty(dirs.shape + (4,), np.int64)
    rec[..., 0] = heads[..., 0] | heads[..., 1] << 8 | 0x5a << 16 | 0x3c << 24
    rec[..., 1] = dirs | alive << 8 | 0xa5 << 16
    rec[..., 2] = 0x00070003
    rec[..., 3] = 0x10000002
    return rec.astype(np.int32)


def run_kernel(torch, obs, rec, vr, source, dtype=None):
    """One snake_graph_obs call on host arrays; the result on the host."""
    from marlenv import _native
    N, S, h, w, C = obs.shape
    dtype = dtype or torch.float64
    cfg = _native.GraphCfg(h, w, C, S, int(vr), ('own', 'reference').index(source), int(dtype == torch.float32))
    o = torch.from_numpy(np.ascontiguousarray(obs)).cuda()
    r = torch.from_numpy(np.ascontiguousarray(rec)).cuda()
    out = torch.full((N, S, 5, C), -7.0, dtype=dtype, device='cuda')
    P = ctypes.c_void_p
    L = _native.lib()
    _native.check(L.snake_graph_obs(ctypes.byref(cfg), P(o.data_ptr()), P(r.data_ptr()), P(out.data_ptr()), N,
                                    P(torch.cuda.current_stream().cuda_stream)), L)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('name', R.CONFIGS)
def test_golden_batch(torch_gpu, calls, name):
    """The recorded calls as one batch, one record per env."""
    torch = torch_gpu
    c = calls[name]
    rec = records(c['heads'], c['dirs'], c['alive'])
    got = run_kernel(torch, c['obs'], rec, c['vr'], 'reference')
    assert got.dtype == np.float64
    live = c['alive'] != 0
    for i in range(len(got)):       # the reference returns the live rows, in index order
        n = int(c['n_alive'][i])
        assert np.array_equal(got[i][live[i]], c['rows'][i, :n]), (name, i)
        assert not got[i][~live[i]].any(), (name, i)
    own = run_kernel(torch, c['obs'], rec, c['vr'], 'own')
    want_own, _ = R.graph_obs(c['obs'], c['heads'], c['dirs'], c['alive'], c['vr'], 'own')
    assert np.array_equal(own, want_own), name
    for source, f64 in (('reference', got), ('own', own)):
        f32 = run_kernel(torch, c['obs'], rec, c['vr'], source, torch.float32)
        assert f32.dtype == np.float32 and np.array_equal(f32, f64.astype(np.float32)), (name, source)


@pytest.mark.parametrize('N', [257, 1])
@pytest.mark.parametrize('kw', [dict(height=8, width=10, vision_range=2, frame_stack=2), dict(height=8, width=8)],
                         ids=['8x10vr2fs2', '8x8full'])
@pytest.mark.parametrize('source', ['own', 'reference'])
def test_live_rollout(torch_gpu, kw, N, source):
    """40 random steps of a GraphVecEnv (257 envs: no multiple of a wave or a
    workgroup): the features it returns equal the restatement on its own grid
    observation and snake table, copied to the host."""
    torch = torch_gpu
    from marlenv import GraphVecEnv
    S = 3
    env = GraphVecEnv(N, num_snakes=S, source=source, seed=21, **kw)
    C = 8 * kw.get('frame_stack', 1)
    assert env.obs_shape == (S, 5, C) and env.grid_obs_shape[3] == C
    vr = kw.get('vision_range', 0)
    rs = np.random.RandomState(N)
    dead_seen = 0

    def check(feat, t):
        nonlocal dead_seen
        assert feat.dtype == torch.float64 and tuple(feat.shape) == (N, S, 5, C)
        tab = env.snake_table().cpu().numpy()
        want, _ = R.graph_obs(env.grid_obs.cpu().numpy(), tab[..., 0:2], tab[..., 4], tab[..., 5], vr, source)
        assert np.array_equal(feat.cpu().numpy(), want), t
        assert np.array_equal(env.alive().cpu().numpy(), tab[..., 5] != 0)
        dead_seen += int((tab[..., 5] == 0).sum())

    check(env.reset(), -1)
    for t in range(40):
        feat, rew, done, info = env.step(torch.from_numpy(rs.randint(0, 3, size=(N, S))))
        assert tuple(rew.shape) == (N, S) and tuple(done.shape) == (N, S)
        check(feat, t)
    assert dead_seen > 0 or N == 1
    # GraphObs on its own, with the default observation (the env's latest) and as float32
    from marlenv import GraphObs
    g32 = GraphObs(env.env, source=source, dtype=torch.float32)
    assert np.array_equal(g32().cpu().numpy(), feat.cpu().numpy().astype(np.float32))
    env.close()


@pytest.mark.parametrize('name', R.CONFIGS)
def test_compat_env_replays_the_reference(torch_gpu, name):
    """GraphSnakeEnv with the reference's seed and actions: the same shapes and
    uint8 arrays at every step, resets included."""
    from marlenv import GraphSnakeEnv
    t = R.load_trajectories()[name]
    np.random.seed(t['seed'])
    env = GraphSnakeEnv(**t['kwargs'])
    for j, (ev, want) in enumerate(zip(t['events'], t['obs'])):
        if ev < 0:
            got = env.reset()
        else:
            got, rews, dones, _ = env.step([int(a) for a in t['actions'][ev]])
            assert all(dones) == (want.shape == (0,)), (name, j)
        assert got.dtype == np.uint8 and got.shape == want.shape, (name, j, got.shape, want.shape)
        assert np.array_equal(got, want), (name, j)
        assert env.graph_rows.dtype == np.float64 and env.graph_rows.shape == want.shape
        assert np.array_equal(env.graph_rows.astype(np.uint8), want)
    env.close()


def test_make_graph_snake(torch_gpu):
    from marlenv import GraphSnakeEnv, GraphVecEnv, make_graph_snake
    env, _, _, props = make_graph_snake(num_envs=1, num_snakes=2, height=8, width=8)
    assert isinstance(env.unwrapped, GraphSnakeEnv) and props == {
        'action_info': {'action_n': 3}, 'num_envs': 1, 'num_snakes': 2}
    assert env.reset().shape == (2, 5, 8)
    venv, _, _, props = make_graph_snake(num_envs=5, num_snakes=2, height=8, width=8, vision_range=2)
    assert isinstance(venv, GraphVecEnv) and props['num_envs'] == 5
    assert tuple(venv.reset().shape) == (5, 2, 5, 8) and tuple(venv.grid_obs.shape) == (5, 2, 5, 5, 8)
    venv.close()


def test_records_that_point_outside_are_clipped(torch_gpu):
    """The in-kernel bounds check: heads on the border (and past it: a head byte
    beyond the map) with directions pointing out, which the env never writes.
    Every ray ends where it leaves the observation; nothing outside is read
    (the observations sit in the middle of a batch whose neighbours are all
    ones, which a read past an edge would pick up)."""
    torch = torch_gpu
    h, w, C, S = 4, 6, 16, 2
    rs = np.random.RandomState(3)
    heads, dirs = [], []
    for r, c in [(0, 2), (3, 5), (0, 0), (2, 0), (3, 3), (0, 5), (1, 5), (200, 3), (2, 255), (255, 255)]:
        for d in range(4):
            heads.append([(r, c), (r, c)])
            dirs.append([d, (d + 1) & 3])
    heads, dirs = np.array(heads), np.array(dirs)
    N = len(heads)
    obs = (rs.random_sample((N, S, h, w, C)) < 0.4).astype(np.uint8)
    obs[:, :, :, :, 0] &= (rs.random_sample((N, S, h, w)) < 0.3)
    obs[::3] = 1            # whole envs of ones (walls everywhere) between the others
    alive = np.ones((N, S), np.uint8)
    alive[1::4, 0] = 0
    for source in ('own', 'reference'):
        want, ended = R.graph_obs(obs, heads, dirs, alive, 0, source)
        assert (ended == R.CLIPPED).sum() > 40 and (ended == R.WALL).any()
        got = run_kernel(torch, obs, records(heads & 255, dirs, alive), 0, source)
        assert np.array_equal(got, want), source
    # with a window the origin is its centre whatever the record's head says
    obs5 = (rs.random_sample((N, S, 5, 5, 8)) < 0.4).astype(np.uint8)
    want, _ = R.graph_obs(obs5, heads, dirs, alive, 2, 'own')
    assert np.array_equal(run_kernel(torch, obs5, records(heads & 255, dirs, alive), 2, 'own'), want)


def test_long_rays_and_wide_stacks(torch_gpu):
    """A vision range beyond one chunk of steps (n = 12 and the limit, 127) and
    the widest stack (C = 128), on synthetic windows with few walls, so rays of
    every length occur; both weight arithmetics at C = 128."""
    torch = torch_gpu
    rs = np.random.RandomState(9)
    for N, S, vr, C, p_wall in ((3, 2, 12, 8, 0.04), (2, 1, 127, 8, 0.004), (2, 3, 3, 128, 0.1), (2, 2, 0, 128, 0.1)):
        h = w = 2 * vr + 1 if vr else 9
        obs = (rs.random_sample((N, S, h, w, C)) < 0.5).astype(np.uint8)
        obs[..., 0] = rs.random_sample((N, S, h, w)) < p_wall
        heads = np.stack([rs.randint(0, h, size=(N, S)), rs.randint(0, w, size=(N, S))], -1)
        dirs = rs.randint(0, 4, size=(N, S))
        alive = np.ones((N, S), np.uint8)
        want, ended = R.graph_obs(obs, heads, dirs, alive, vr, 'own')
        if vr == 12:
            assert (ended == R.FULL).any() and (ended == R.WALL).any()
        assert np.array_equal(run_kernel(torch, obs, records(heads, dirs, alive), vr, 'own'), want), (vr, C)


def test_argument_errors(torch_gpu):
    torch = torch_gpu
    from marlenv import GraphObs, SnakeVecEnv
    env = SnakeVecEnv(3, num_snakes=2, height=8, width=8, vision_range=2)
    g = GraphObs(env)
    with pytest.raises(ValueError, match='pass obs'):
        g()                                     # nothing returned yet
    obs = env.reset()
    assert tuple(g().shape) == (3, 2, 5, 8)
    with pytest.raises(TypeError):
        g(obs.float())
    with pytest.raises(ValueError):
        g(obs[:2])
    with pytest.raises(ValueError, match='no CPU fallback'):
        g(obs.cpu())
    del obs
    with pytest.raises(ValueError, match='pass obs'):
        g()                                     # the caller dropped it
    env.close()
