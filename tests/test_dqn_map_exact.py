"""The map path of the bf16 DQN forward (k_dqn_map_conv + k_dqn_fc) on integer
probe nets: q and features must EQUAL the float64 reference, no tolerance.

tests/dqn_probe.py's networks keep the kernels' arithmetic exact
(tests/test_dqn_map_cpu.py proves it for every probe used here), so one wrong
border cell, row-tile share, padding row, tail row or stale LDS cell changes an
integer. Every case runs plan='map' under every value of MAP_CONV_WAVES: the
full 20x20 map and the largest image the plan takes (22x22) at 8 and 32
channels, rectangular maps, row-tile counts that no wave count divides (26, 33,
9, 1), maps with fewer row tiles than waves, batch tails, the persistent loop's
later iterations and num_actions."""
import ctypes

import pytest

torch = pytest.importorskip('torch')

import dqn_map_cases as mc
import dqn_probe as dp

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5      # no probe output: those are integers


def _waves():
    from marlenv.dqn import MAP_CONV_WAVES
    return MAP_CONV_WAVES


def _same(got, want, what):
    got = got.double().cpu()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        print('%s: %d of %d differ, first at %s: got %r, want %r; rows %s' % (
            what, bad.size(0), want.numel(), i, float(got[i]), float(want[i]),
            sorted(set(bad[:, 0].tolist()))[:16]))
    assert torch.equal(got, want), what


def _forward(p, waves=0, plan='map'):
    from marlenv.dqn import DQNForward
    h, w, c, a = p.key[:4]
    state = {k: v.cuda() for k, v in p.state.items()}
    net = DQNForward(state, h, w, c, a, conv_waves=waves, plan=plan)
    assert net.plan == plan
    return net


def _check(net, obs, feat, q, what):
    got_q = net(obs)
    got_f = net.forward_features(obs)
    torch.cuda.synchronize()
    assert got_q.shape == q.shape and got_f.shape == feat.shape
    _same(got_q, q, what + ' q')
    _same(got_f, feat, what + ' features')


@pytest.mark.parametrize('h,w,c', mc.GRID, ids=['%dx%dx%d' % g for g in mc.GRID])
def test_map_grid(h, w, c):
    """Three nets each, B = 37, every conv_waves."""
    for seed in mc.SEEDS:
        p = dp.probe(h, w, c, 3, seed, mc.GRID_B)
        obs = p.obs.cuda()
        for waves in _waves():
            _check(_forward(p, waves), obs, p.feat, p.q, '%dx%dx%d seed %d waves %d' % (h, w, c, seed, waves))


@pytest.mark.parametrize('B', mc.TAIL_B)
def test_map_batch_tails(B):
    """snake_dqn_map_forward on caller-allocated outputs longer than the batch:
    rows below B equal the reference, the rows behind them keep their sentinel."""
    from marlenv._native import check
    p = dp.probe(*(mc.TAIL_GEO + (3, 0, max(mc.TAIL_B))))
    obs = p.obs.cuda()
    pad = 256                                 # k_dqn_fc's rows per workgroup
    for waves in _waves():
        net = _forward(p, waves)
        a = net.num_actions
        q = torch.full((B + pad, a), SENTINEL, dtype=torch.float32, device='cuda')
        feat = torch.full((B + pad, 128), SENTINEL, dtype=torch.float32, device='cuda')
        scratch = torch.empty(B * net.layout.act_per_obs, dtype=torch.int16, device='cuda')
        x = obs[:B].contiguous()
        check(net._L.snake_dqn_map_forward(ctypes.byref(net.cfg), ctypes.byref(net.net), ctypes.c_void_p(x.data_ptr()),
                                           B, ctypes.c_void_p(scratch.data_ptr()), ctypes.c_void_p(q.data_ptr()),
                                           ctypes.c_void_p(feat.data_ptr()),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), net._L)
        torch.cuda.synchronize()
        _same(q[:B], p.q[:B], 'B %d waves %d q' % (B, waves))
        _same(feat[:B], p.feat[:B], 'B %d waves %d features' % (B, waves))
        assert torch.equal(q[B:].cpu(), torch.full((pad, a), SENTINEL)), 'q written past row B'
        assert torch.equal(feat[B:].cpu(), torch.full((pad, 128), SENTINEL)), 'features written past row B'


@pytest.mark.parametrize('h,w,c', mc.PERSIST, ids=['%dx%dx%d' % g for g in mc.PERSIST])
def test_map_persistent_loop(h, w, c):
    """More observations than twice the workgroups the device holds (at most
    floor(160 KiB / LDS per workgroup) per CU): every workgroup runs at least two
    observations, neighbours in its sequence differ. 64 unique probe
    observations gathered by a random index vector; twice on one DQNForward (the
    scratch buffer is grown, then reused)."""
    p = dp.probe(h, w, c, 3, 0, mc.PERSIST_UNIQUE)
    obs = p.obs.cuda()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for waves in _waves():
        net = _forward(p, waves)
        _check(net, obs, p.feat, p.q, 'unique rows')
        B = 2 * (160 * 1024 // net.layout.lds_conv) * n_cu + 77
        for run in range(2):
            idx = torch.randint(0, mc.PERSIST_UNIQUE, (B,), generator=torch.Generator().manual_seed(17 + run))
            _check(net, obs[idx.cuda()].contiguous(), p.feat[idx], p.q[idx], 'waves %d B %d run %d' % (waves, B, run))


@pytest.mark.parametrize('a', mc.ACTIONS)
def test_map_num_actions(a):
    for seed in mc.SEEDS:
        p = dp.probe(*(mc.ACTIONS_GEO + (a, seed, mc.GRID_B)))
        for waves in _waves():
            _check(_forward(p, waves), p.obs.cuda(), p.feat, p.q, 'A %d seed %d waves %d' % (a, seed, waves))


def test_auto_plan():
    """'auto' takes the window path where snake_dqn_plan accepts the geometry,
    else the map path; 'window' keeps today's error on the full map."""
    from marlenv.dqn import DQNForward
    p = dp.probe(20, 20, 8, 3, 0, mc.GRID_B)
    net = DQNForward({k: v.cuda() for k, v in p.state.items()}, 20, 20, 8, 3)
    assert net.plan == 'map' and net.precision == 'bf16'
    _check(net, p.obs.cuda(), p.feat, p.q, 'auto 20x20')
    with pytest.raises(ValueError):
        DQNForward({k: v.cuda() for k, v in p.state.items()}, 20, 20, 8, 3, plan='window')
    p = dp.probe(11, 11, 8, 3, 0, mc.GRID_B)
    net = DQNForward({k: v.cuda() for k, v in p.state.items()}, 11, 11, 8, 3)
    assert net.plan == 'window'
    _check(net, p.obs.cuda(), p.feat, p.q, 'auto 11x11')
    net32 = DQNForward({k: v.cuda() for k, v in p.state.items()}, 11, 11, 8, 3, precision='fp32')
    assert net32.plan is None
