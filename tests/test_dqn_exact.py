"""The DQN forward kernels (dqn_kernels.hip, dqn32_kernels.hip) on integer probe
nets: q and features must EQUAL the float64 reference, no tolerance.

tests/dqn_probe.py builds networks whose arithmetic is exact in bf16 and fp32
(tests/test_dqn_probe_cpu.py proves it for every probe used here), so one wrong
border cell, channel pair, padding row, tail row or stale LDS cell changes an
integer. Runs what tests/test_dqn.py's tolerances cannot hold: every size x
channel padding x conv_waves kernel, the overlaid LDS plan (11x11 with 24 or 32
channels), the persistent loop's later iterations, batch tails, num_actions,
and in fp32 mode both sides of the convolution dispatch, both cell strides,
non-square, 1-wide and 1x1 maps."""
import ctypes

import pytest

torch = pytest.importorskip('torch')

import dqn_probe as dp

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5      # no probe output: those are integers


def _same(got, want, what):
    got = got.double().cpu()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        print('%s: %d of %d differ, first at %s: got %r, want %r; rows %s' % (
            what, bad.size(0), want.numel(), i, float(got[i]), float(want[i]),
            sorted(set(bad[:, 0].tolist()))[:16]))
    assert torch.equal(got, want), what


def _forward(p, waves=0, precision='bf16'):
    from marlenv.dqn import DQNForward
    h, w, c, a = p.key[:4]
    state = {k: v.cuda() for k, v in p.state.items()}
    return DQNForward(state, h, w, c, a, conv_waves=waves, precision=precision)


def _check(net, obs, feat, q, what):
    got_q = net(obs)
    got_f = net.forward_features(obs)
    torch.cuda.synchronize()
    assert got_q.shape == q.shape and got_f.shape == feat.shape
    _same(got_q, q, what + ' q')
    _same(got_f, feat, what + ' features')


@pytest.mark.parametrize('size,c', [(s, c) for s in dp.GRID_SIZES for c in dp.GRID_CHANNELS])
def test_bf16_grid(size, c):
    """Every size x channel count, conv_waves 1, 2 and 4, three nets each, B = 70."""
    for seed in dp.SEEDS:
        p = dp.probe(size, size, c, 3, seed, dp.GRID_B)
        obs = p.obs.cuda()
        for waves in dp.GRID_WAVES:
            _check(_forward(p, waves), obs, p.feat, p.q, '%dx%dx%d seed %d waves %d' % (size, size, c, seed, waves))


@pytest.fixture(scope='module')
def tail_net():
    p = dp.probe(*(dp.TAIL_GEO + (3, 0, max(dp.TAIL_B))))
    return p, _forward(p), p.obs.cuda()


@pytest.mark.parametrize('B', dp.TAIL_B)
def test_bf16_batch_tails(tail_net, B):
    """snake_dqn_forward on caller-allocated outputs longer than the batch: rows
    below B equal the reference, the rows behind them keep their sentinel."""
    p, net, obs = tail_net
    pad = 256                                 # k_dqn_fc's rows per workgroup
    a = net.num_actions
    q = torch.full((B + pad, a), SENTINEL, dtype=torch.float32, device='cuda')
    feat = torch.full((B + pad, 128), SENTINEL, dtype=torch.float32, device='cuda')
    scratch = torch.empty(B * net.layout.act_per_obs, dtype=torch.int16, device='cuda')
    x = obs[:B].contiguous()
    from marlenv._native import check
    check(net._L.snake_dqn_forward(ctypes.byref(net.cfg), ctypes.byref(net.net), ctypes.c_void_p(x.data_ptr()), B,
                                   ctypes.c_void_p(scratch.data_ptr()), ctypes.c_void_p(q.data_ptr()),
                                   ctypes.c_void_p(feat.data_ptr()),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), net._L)
    torch.cuda.synchronize()
    _same(q[:B], p.q[:B], 'B %d q' % B)
    _same(feat[:B], p.feat[:B], 'B %d features' % B)
    assert torch.equal(q[B:].cpu(), torch.full((pad, a), SENTINEL)), 'q written past row B'
    assert torch.equal(feat[B:].cpu(), torch.full((pad, 128), SENTINEL)), 'features written past row B'


@pytest.mark.parametrize('a', dp.ACTIONS)
def test_bf16_num_actions(a):
    for seed in dp.SEEDS:
        p = dp.probe(*(dp.ACTIONS_GEO + (a, seed, dp.GRID_B)))
        _check(_forward(p), p.obs.cuda(), p.feat, p.q, 'A %d seed %d' % (a, seed))


@pytest.mark.parametrize('h,w,c,waves', dp.PERSIST)
def test_bf16_persistent_loop(h, w, c, waves):
    """More observations than twice the waves the device holds: every workgroup
    of every variant runs at least two observations, neighbours in its sequence
    differ. 256 unique probe observations gathered by a random index vector;
    twice on one DQNForward (the scratch buffer is grown, then reused)."""
    p = dp.probe(h, w, c, 3, 0, dp.PERSIST_UNIQUE)
    net = _forward(p, waves)
    obs = p.obs.cuda()
    _check(net, obs, p.feat, p.q, 'unique rows')
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 2 * 32 * n_cu + 77
    for run in range(2):
        idx = torch.randint(0, dp.PERSIST_UNIQUE, (B,), generator=torch.Generator().manual_seed(17 + run))
        _check(net, obs[idx.cuda()].contiguous(), p.feat[idx], p.q[idx], 'B %d run %d' % (B, run))


FP32_IDS = ['%dx%dx%d-a%d-b%d' % c[:5] for c in dp.FP32_CASES]


@pytest.mark.parametrize('h,w,c,a,B,mfma', dp.FP32_CASES, ids=FP32_IDS)
def test_fp32_exact(h, w, c, a, B, mfma):
    """precision='fp32' on the same probes (0/1 input: the /255 branch is not
    taken). `mfma` says which convolution kernel the case reaches
    (dp.fp32_conv_on_matrix_cores, checked on the CPU)."""
    for seed in dp.SEEDS[:2]:
        p = dp.probe(h, w, c, a, seed, B)
        net = _forward(p, precision='fp32')
        obs = p.obs.cuda()
        for n in dp.FP32_PREFIXES.get((h, w, c, a, B), (B,)):
            _check(net, obs[:n].contiguous(), p.feat[:n], p.q[:n], 'seed %d B %d' % (seed, n))
