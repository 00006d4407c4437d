"""The greedy-opponent kernel (snake_greedy_actions, greedy_kernels.hip) against
the reference's recorded calls and the numpy restatement (tests/greedy_ref.py)
on the same inputs copied to the host: every case exact (actions and directions
are integers). Every comparison runs in both layouts, four snakes per wave (the
one maps of at most 16 rows take) and rows on 64 lanes (through the library's
testing aid), which therefore agree with each other."""
import ctypes

import numpy as np
import pytest

import greedy_ref as R

pytestmark = pytest.mark.gpu

UNIT = ((-1, 0), (1, 0), (0, -1), (0, 1))


@pytest.fixture(scope='module')
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), 'needs the GPU'
    return torch


def run_kernel(torch, obs, rnd, skip, dirs, rows=False):
    """One call on host arrays; returns (actions, dirs out) on the host. With
    random bits and rows=False it goes through GreedyActions; rnd None is the C
    call with rnd = NULL (GreedyActions itself would draw), and rows=True the
    library's testing aid snake_debug_greedy_actions, which takes the
    rows-on-64-lanes layout whatever the height."""
    from marlenv import GreedyActions, _native
    ga = GreedyActions(obs.shape[1:])
    d = torch.from_numpy(np.ascontiguousarray(dirs)).cuda()
    o = torch.from_numpy(obs).cuda()
    sk = None if skip is None else torch.from_numpy(skip).cuda()
    r = None if rnd is None else torch.from_numpy(np.ascontiguousarray(rnd).view(np.int32)).cuda()
    if r is not None and not rows:
        a = ga(o, skip=sk, dirs=d, rnd=r)
    else:
        a = torch.empty(obs.shape[:2], dtype=torch.int8, device='cuda')
        P = ctypes.c_void_p
        args = (ctypes.byref(ga.cfg), P(o.data_ptr()), P(r.data_ptr()) if r is not None else None,
                P(sk.data_ptr()) if sk is not None else None, P(d.data_ptr()), P(a.data_ptr()),
                ctypes.c_int64(obs.shape[0]), P(torch.cuda.current_stream().cuda_stream))
        L = _native.lib()
        _native.check(L.snake_debug_greedy_actions(*args, ctypes.c_int(1)) if rows else L.snake_greedy_actions(*args))
        torch.cuda.synchronize()
    assert a.dtype == torch.int8 and tuple(a.shape) == obs.shape[:2]
    return a.cpu().numpy(), d.cpu().numpy()


def both_layouts(torch, obs, rnd, skip, dirs, act, dout):
    for rows in (False, True):
        got_a, got_d = run_kernel(torch, obs, rnd, skip, dirs, rows)
        np.testing.assert_array_equal(got_a, act, err_msg='rows=%s' % rows)
        np.testing.assert_array_equal(got_d, dout, err_msg='rows=%s' % rows)


def check(torch, obs, rnd, skip, dirs):
    act, dout, cat = R.greedy_actions(obs, rnd, skip, dirs)
    both_layouts(torch, obs, rnd, skip, dirs, act, dout)
    return act, dout, cat


@pytest.mark.parametrize('name', ['b10x14', 'b12', 'crafted', 'full20', 'vr5'])
def test_fixture_records(torch_gpu, name):
    """The reference's own calls, one record per env of a batch."""
    c = R.load_calls()[name]
    both_layouts(torch_gpu, c['obs'], c['rnd'], c['skip'], c['din'], c['act'], c['dout'])


def synthetic(rs, N, S, h, w):
    """Random observations with bytes from {0, 1, 2, 255} (only == 1 counts):
    per snake a blocked density from open to nearly closed maps, fruits from
    none to many, 0 to 3 heads (most snakes one; a third of them on the map's
    edge) and some body and tail cells, a few of them beside the head."""
    obs = np.zeros((N, S, h, w, 8), np.uint8)
    vals = np.array([1, 1, 1, 2, 255], np.uint8)

    def sprinkle(plane, p):
        m = rs.random_sample(plane.shape) < p
        plane[m] = vals[rs.randint(len(vals), size=int(m.sum()))]

    for n in range(N):
        for s in range(S):
            o = obs[n, s]
            block = rs.uniform(0.02, 0.6)
            sprinkle(o[:, :, 0], block * 0.6)
            sprinkle(o[:, :, 3], block * 0.2)
            sprinkle(o[:, :, 1], rs.choice([0.0, 2.0 / (h * w), 0.05, 0.3]))
            sprinkle(o[:, :, 2], 0.02)
            sprinkle(o[:, :, 4], 0.01)
            sprinkle(o[:, :, 6], rs.randint(0, 41) / (h * w))
            sprinkle(o[:, :, 7], 0.01)
            sprinkle(o[:, :, 5], 0.01 * (rs.randint(3) == 0))          # decoys and extra heads
            for _ in range(rs.choice([0, 1, 1, 1, 1, 2, 3])):
                y, x = rs.randint(h), rs.randint(w)
                if rs.randint(3) == 0:
                    y, x = [(0, x), (h - 1, x), (y, 0), (y, w - 1)][rs.randint(4)]
                o[y, x, :] = 0
                o[y, x, 5] = 1
                for ny, nx in UNIT:                                     # body or tail cells beside the head
                    if rs.randint(4) == 0 and 0 <= y + ny < h and 0 <= x + nx < w:
                        o[y + ny, x + nx, 6 + rs.randint(2)] = vals[rs.randint(len(vals))]
    rnd = rs.randint(0, 2 ** 32, size=(N, S), dtype=np.uint64).astype(np.uint32)
    edge = rs.randint(6, size=(N, S))
    rnd[edge == 0] = 0
    rnd[edge == 1] = 0xFFFFFFFF
    skip = (rs.random_sample((N, S)) < 0.2).astype(np.uint8)
    choices = np.array(UNIT + ((0, 0), (R.UNKNOWN, R.UNKNOWN), (R.UNKNOWN, R.UNKNOWN)), np.int8)
    dirs = choices[rs.randint(len(choices), size=(N, S))]
    return obs, rnd, skip, dirs


@pytest.mark.parametrize('S,h,w', [(4, 20, 20), (4, 11, 11), (1, 3, 3), (3, 7, 13), (16, 64, 64), (5, 16, 64),
                                   (4, 17, 9)])
def test_synthetic(torch_gpu, S, h, w):
    """37 envs (odd: with odd h*w the batch ends on a half 16-byte chunk).
    (4, 11, 11), (1, 3, 3), (3, 7, 13) and (5, 16, 64) take four snakes per wave:
    (1, 3, 3) leaves one snake in the last wave, the 185 snakes of (5, 16, 64)
    put snakes of two envs into one wave; (4, 17, 9) is the first height that
    must not. (16, 64, 64) puts rows on lanes 0 and 63 and columns on bits 0
    and 63."""
    rs = np.random.RandomState(1000 * S + 10 * h + w)
    obs, rnd, skip, dirs = synthetic(rs, 37, S, h, w)
    act, dout, cat = check(torch_gpu, obs, rnd, skip, dirs)
    if (S, h, w) == (4, 20, 20):        # the inputs reach every category
        for k, name in R.CATEGORY_NAMES.items():
            assert ((cat & k) != 0).any(), name
    # no skip mask and rnd = NULL: the first of the best moves
    check(torch_gpu, obs, None, None, dirs)


def cell_obs(cells, h=5, w=5):
    o = np.zeros((h, w, 8), np.uint8)
    for (y, x), ch in cells.items():
        o[y, x, ch] = 1
    return o


def test_crafted_cases(torch_gpu):
    cases = [
        # a head walled in on three sides, the body behind it: action 0, and the direction read off the body is stored
        (cell_obs({(2, 2): 5, (3, 2): 6, (1, 2): 0, (2, 1): 3, (2, 3): 4}), None, 99, 0, (-1, 0)),
        # two fruits two cells away, heading right: the first in row-major order, (0, 2), makes move 1 (up) the
        # one best move; with the last, (2, 0), all three would tie and these random bits would pick move 2
        (cell_obs({(2, 2): 5, (0, 2): 1, (2, 0): 1}), (0, 1), 0xFFFFFFFF, 1, (-1, 0)),
        # a fruit left and one right of the head in its row, two cells each, heading up: the left one
        (cell_obs({(2, 2): 5, (2, 0): 1, (2, 4): 1}), (-1, 0), 0, 1, (0, -1)),
        # the same on the map's last columns of a 64-wide row is in test_synthetic's reach; here: no head at all
        (cell_obs({(1, 1): 1}), None, 5, 0, None),
    ]
    obs = np.ascontiguousarray(np.stack([c[0] for c in cases])[:, None])
    dirs = np.array([[(R.UNKNOWN, R.UNKNOWN) if c[1] is None else c[1]] for c in cases], np.int8)
    rnd = np.array([[c[2]] for c in cases], np.uint32)
    act, dout, _ = check(torch_gpu, obs, rnd, None, dirs)
    assert act[:, 0].tolist() == [c[3] for c in cases]
    for i, c in enumerate(cases):
        assert dout[i, 0].tolist() == list(c[4] if c[4] is not None else (R.UNKNOWN, R.UNKNOWN))


def test_generator_draws_are_reproducible(torch_gpu):
    """rnd=None draws the bits from the generator: the same seed, the same
    actions; over an open map without fruit (three moves tie) all three occur."""
    torch = torch_gpu
    from marlenv import GreedyActions
    obs = np.zeros((64, 4, 7, 7, 8), np.uint8)
    obs[:, :, 3, 3, 5] = 1
    obs = torch.from_numpy(obs).cuda()
    runs = []
    for seed in (5, 5, 6):
        ga = GreedyActions((4, 7, 7, 8), generator=torch.Generator(device='cuda').manual_seed(seed))
        runs.append(torch.stack([ga(obs), ga(obs)]).cpu().numpy())
    np.testing.assert_array_equal(runs[0], runs[1])
    assert (runs[0] != runs[2]).any()
    assert set(np.unique(runs[0]).tolist()) == {0, 1, 2}


def test_argument_errors(torch_gpu):
    torch = torch_gpu
    from marlenv import GreedyActions
    ga = GreedyActions((2, 5, 5, 8))
    obs = torch.zeros((3, 2, 5, 5, 8), dtype=torch.uint8, device='cuda')
    ga(obs)
    with pytest.raises(TypeError):
        ga(obs, rnd=torch.zeros((3, 2), dtype=torch.int64, device='cuda'))
    with pytest.raises(TypeError):
        ga(obs, rnd=torch.zeros((3, 2), dtype=torch.int32))
    with pytest.raises(TypeError):
        ga(obs, rnd=torch.zeros((2, 3), dtype=torch.int32, device='cuda'))
    with pytest.raises(TypeError):
        ga(obs, dirs=torch.zeros((3, 2, 2), dtype=torch.int32, device='cuda'))
    with pytest.raises(TypeError):
        ga(obs, dirs=torch.zeros((3, 2, 4), dtype=torch.int8, device='cuda')[:, :, ::2])
    with pytest.raises(ValueError):
        ga(obs.cpu())


@pytest.mark.parametrize('vision_range', [None, 5])
def test_end_to_end_rollout(torch_gpu, vision_range):
    """80 steps of a 32-env batch driven by the kernel's own actions: at every
    step they equal the restatement run on the GPU's observations, with the
    directions kept by GreedyActions and forgotten where an episode ends."""
    torch = torch_gpu
    from marlenv import GreedyActions, SnakeVecEnv
    N, S = 32, 4
    env = SnakeVecEnv(N, num_snakes=S, height=20, width=20, snake_length=5, vision_range=vision_range, seed=11)
    ga = GreedyActions(env.obs_shape)
    obs = env.reset()
    rs = np.random.RandomState(5)
    dirs = np.full((N, S, 2), R.UNKNOWN, np.int8)
    skip = np.zeros((N, S), np.uint8)
    seen = 0
    for t in range(80):
        rnd = rs.randint(0, 2 ** 32, size=(N, S), dtype=np.uint64).astype(np.uint32)
        a = ga(obs, skip=torch.from_numpy(skip).cuda(), rnd=torch.from_numpy(rnd.view(np.int32)).cuda())
        act, dirs, cat = R.greedy_actions(obs.cpu().numpy(), rnd, skip, dirs)
        np.testing.assert_array_equal(a.cpu().numpy(), act, err_msg='step %d' % t)
        np.testing.assert_array_equal(ga.dirs.cpu().numpy(), dirs, err_msg='step %d' % t)
        seen |= int(np.bitwise_or.reduce(cat.reshape(-1)))
        obs, _, done, info = env.step(a)
        ended = info['episode_done']
        ga.forget(ended)
        dirs[ended.cpu().numpy()] = R.UNKNOWN
        skip = (done & ~ended[:, None]).cpu().numpy().astype(np.uint8)
    assert seen & R.N1 and seen & R.N2 and seen & R.SKIP
    env.close()


def test_forget_on_reset_false_keeps_the_heading(torch_gpu):
    torch = torch_gpu
    from marlenv import GreedyActions
    obs = torch.zeros((2, 1, 5, 5, 8), dtype=torch.uint8, device='cuda')
    obs[:, 0, 2, 2, 5] = 1
    obs[:, 0, 2, 1, 6] = 1              # body on the left: heading (0, 1)
    obs[:, 0, 1, 2, 0] = obs[:, 0, 3, 2, 0] = 1     # walls above and below: forward is the one live move
    for keep in (False, True):
        ga = GreedyActions((1, 5, 5, 8), forget_on_reset=not keep)
        ga(obs)
        assert ga.dirs.cpu().numpy().tolist() == [[[0, 1]], [[0, 1]]]
        ga.forget(torch.tensor([True, False]))
        want = [[[0, 1]], [[0, 1]]] if keep else [[[R.UNKNOWN, R.UNKNOWN]], [[0, 1]]]
        assert ga.dirs.cpu().numpy().tolist() == want
