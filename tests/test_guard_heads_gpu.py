"""The decision heads on outputs of exactly their size, inside a guard-band
arena (tests/guard_util.py): snake_safe_actions and snake_greedy_actions
(`actions`, and `dirs`, which is updated in place), snake_graph_obs (`out` as
float64 and as float32) and snake_genome_actions (`actions`, `outputs` and a
scratch of exactly snake_genome_plan's byte count). After the guards pass the
results are compared, exactly, with the numpy restatements (tests/policy_ref.py,
greedy_ref.py, graph_ref.py, genome_ref.py); the outputs start as 0x5A, so a
value nothing wrote shows.

A read outside a buffer is invisible to this method."""
import ctypes

import numpy as np
import pytest

import genome_ref
import graph_ref
import greedy_ref
import policy_ref
from guard_util import Arena

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

VP = ctypes.c_void_p
BATCHES = [(1, 1), (3, 3), (257, 4), (5, 16)]       # (N, S): one snake; odd; more than a workgroup's envs; 16 snakes
UNKNOWN = -128


@pytest.fixture(scope='module', autouse=True)
def native():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    from marlenv import _native
    _native.lib()
    return _native


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def policy_inputs(rs, N, S, h, w):
    """Sparse 0/1 observations with one head cell per snake (most of them), a
    few fruits, random Q-values, known and unknown directions, a skip mask."""
    obs = (rs.rand(N, S, h, w, 8) < 0.06).astype(np.uint8)
    obs[..., 5] = 0
    hy, hx = rs.randint(0, h, (N, S)), rs.randint(0, w, (N, S))
    has_head = rs.rand(N, S) < 0.9
    n, s = np.nonzero(has_head)
    obs[n, s, hy[n, s], hx[n, s], :] = 0
    obs[n, s, hy[n, s], hx[n, s], 5] = 1
    units = np.array([(-1, 0), (1, 0), (0, -1), (0, 1), (UNKNOWN, UNKNOWN)], np.int8)
    dirs = units[rs.randint(0, 5, (N, S))]
    skip = (rs.rand(N, S) < 0.2).astype(np.uint8)
    q = rs.randn(N, S, 3).astype(np.float32)
    rnd = rs.randint(0, 2 ** 32, (N, S), dtype=np.uint64).astype(np.uint32)
    return obs, q, skip, dirs, rnd


@pytest.mark.parametrize('h,w', [(7, 13), (11, 11)])
@pytest.mark.parametrize('N,S', BATCHES)
@pytest.mark.parametrize('head', ['safe', 'greedy'])
def test_action_heads(native, head, N, S, h, w):
    L = native.lib()
    rs = np.random.RandomState(1000 * N + 10 * S + h)
    obs, q, skip, dirs, rnd = policy_inputs(rs, N, S, h, w)
    cfg = native.PolicyCfg(h, w, 8, S, 60)
    ar = Arena([N * S, 2 * N * S])
    actions = ar.take('actions', N * S, torch.int8, (N, S))
    d = ar.take('dirs', 2 * N * S, torch.int8, (N, S, 2))
    d.copy_(dev(dirs))
    o, sk = dev(obs), dev(skip)
    if head == 'safe':
        qd = dev(q)
        native.check(L.snake_safe_actions(ctypes.byref(cfg), VP(o.data_ptr()), VP(qd.data_ptr()), VP(sk.data_ptr()),
                                          ar.ptr('dirs'), ar.ptr('actions'), N, None), L)
        want_a, want_d, _ = policy_ref.safe_actions(obs, q, skip, dirs, 60)
    else:
        rd = dev(rnd)
        native.check(L.snake_greedy_actions(ctypes.byref(cfg), VP(o.data_ptr()), VP(rd.data_ptr()), VP(sk.data_ptr()),
                                            ar.ptr('dirs'), ar.ptr('actions'), N, None), L)
        want_a, want_d, _ = greedy_ref.greedy_actions(obs, rnd, skip, dirs)
    ar.check('%s N=%d S=%d %dx%d' % (head, N, S, h, w))
    np.testing.assert_array_equal(actions.cpu().numpy(), want_a)
    np.testing.assert_array_equal(d.cpu().numpy(), want_d)


def records(heads, dirs, alive):
    """Snake records int32 (N, S, 4): word 0 = head row | head column << 8, word 1
    = direction | alive << 8; the bits the kernel does not read get a pattern."""
    heads, dirs, alive = (np.asarray(x).astype(np.int64) for x in (heads, dirs, alive))
    rec = np.empty(dirs.shape + (4,), np.int64)
    rec[..., 0] = heads[..., 0] | heads[..., 1] << 8 | 0x5a << 16 | 0x3c << 24
    rec[..., 1] = dirs | alive << 8 | 0xa5 << 16
    rec[..., 2] = 0x00070003
    rec[..., 3] = 0x10000002
    return rec.astype(np.int32)


@pytest.mark.parametrize('h,w,C,vr', [(5, 5, 8, 2), (8, 10, 16, 0)], ids=['5x5x8-window', '8x10x16-full-map'])
@pytest.mark.parametrize('N,S', BATCHES)
def test_graph_obs(native, N, S, h, w, C, vr):
    """`out` of exactly N * S * 5 * C doubles, then floats: every value is written."""
    L = native.lib()
    rs = np.random.RandomState(2000 * N + 10 * S + h)
    obs = (rs.rand(N, S, h, w, C) < 0.3).astype(np.uint8)
    heads = np.stack([rs.randint(0, h, (N, S)), rs.randint(0, w, (N, S))], -1)
    dirs, alive = rs.randint(0, 4, (N, S)), (rs.rand(N, S) < 0.8).astype(np.int64)
    want, _ = graph_ref.graph_obs(obs, heads, dirs, alive, vr, 'own')
    o, r = dev(obs), dev(records(heads, dirs, alive))
    n = N * S * 5 * C
    for f32 in (0, 1):
        dtype, size = (torch.float32, 4) if f32 else (torch.float64, 8)
        cfg = native.GraphCfg(h, w, C, S, vr, 0, f32)
        ar = Arena([n * size])
        out = ar.take('out', n * size, dtype, (N, S, 5, C))
        native.check(L.snake_graph_obs(ctypes.byref(cfg), VP(o.data_ptr()), VP(r.data_ptr()), ar.ptr('out'), N, None), L)
        ar.check('graph N=%d S=%d %dx%dx%d f32=%d' % (N, S, h, w, C, f32))
        got = out.cpu().numpy()
        assert np.array_equal(got, want.astype(np.float32) if f32 else want), (N, S, f32)
    assert want.any() and not want[alive == 0].any()


@pytest.mark.parametrize('fits_lds', [False, True], ids=['scratch', 'lds'])
def test_genome_actions(native, fits_lds):
    """Three relu-only genomes over 7 envs x 3 snakes: with the largest genome
    over lds_nodes its node values live in the scratch, taken at exactly
    snake_genome_plan's byte count; else the plan's scratch is 0 and NULL is
    passed. Exact against the restatement (relu-only programs are exact)."""
    from marlenv import GenomeHeads
    L = native.lib()
    N, S, I, A = 7, 3, 33, 3
    relu = (genome_ref.relu_activation,)
    rs = np.random.RandomState(77 + fits_lds)
    lay0 = native.GenomeLayout()
    cfg0 = native.GenomeCfg(I, 1, 1, 0, 0, 0)
    native.check(L.snake_genome_plan(ctypes.byref(cfg0), 64, ctypes.byref(lay0)), L)
    limit = int(lay0.lds_nodes)
    nets = [genome_ref.random_network(rs, I, A, hidden=7, acts=relu), genome_ref.chain_network(rs, I, A, 5, acts=relu),
            genome_ref.random_network(rs, I, A, hidden=12 if fits_lds else limit + 1, acts=relu)]
    assert (max(len(n.node_evals) for n in nets) > limit) == (not fits_lds)
    g = np.array([2, 0, 1, 2, 0, 2, 1])
    x = genome_ref.random_features(rs, N * S, I)
    skip = (rs.rand(N, S) < 0.25).astype(np.uint8)
    heads = GenomeHeads(nets, num_inputs=I, genome_of_env=g)
    lay, tiles, rows = heads.tiles(S)
    assert (int(lay.scratch) == 0) == fits_lds and ((tiles[:, 3] >= 0).any() == (not fits_lds))
    heads._upload(torch.device('cuda', torch.cuda.current_device()))
    ar = Arena([N * S, 8 * N * S * A, int(lay.scratch)])
    actions = ar.take('actions', N * S, torch.int8, (N, S))
    outputs = ar.take('outputs', 8 * N * S * A, torch.float64, (N, S, A))
    if lay.scratch:
        ar.take('scratch', lay.scratch)
    f, sk, t, r = dev(x), dev(skip), dev(tiles), dev(rows)
    native.check(L.snake_genome_actions(
        ctypes.byref(heads.cfg), ctypes.byref(heads._dev_prog), VP(t.data_ptr()), VP(r.data_ptr()), tiles.shape[0],
        VP(f.data_ptr()), VP(sk.data_ptr()), ar.ptr('actions'), ar.ptr('outputs'),
        ar.ptr('scratch') if lay.scratch else None, N * S, None), L)
    ar.check('genome fits_lds=%s' % fits_lds)
    out, err, act = genome_ref.reference(nets, g, x, S, skip)
    assert (err == 0.0).all()
    got = outputs.cpu().numpy()
    assert (got.view(np.uint64) == np.ascontiguousarray(out, np.float64).view(np.uint64)).all()
    np.testing.assert_array_equal(actions.cpu().numpy(), act)
