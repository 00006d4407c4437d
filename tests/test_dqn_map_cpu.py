"""The map path of the bf16 DQN forward, the parts that need no GPU: what
snake_dqn_map_plan accepts and rejects, the GEMM row table, and that every probe
tests/test_dqn_map_exact.py runs keeps the kernels' arithmetic exact and
notices a wrong weight (conditions on the probes, as tests/test_dqn_probe_cpu.py
holds them for the window path)."""
import ctypes

import pytest

torch = pytest.importorskip('torch')

import dqn_map_cases as mc
import dqn_probe as dp
from test_dqn_probe_cpu import sharpness

KEYS = mc.probe_keys()


def _plan(h, w, c, a=3, waves=0, fn='snake_dqn_map_plan'):
    from marlenv import _native
    lay = _native.DqnLayout()
    L = _native.lib()
    rc = getattr(L, fn)(ctypes.byref(_native.DqnCfg(h, w, c, a, waves)), ctypes.byref(lay))
    return rc, lay, L


@pytest.mark.parametrize('h,w,c', mc.PLAN_ACCEPTS)
def test_map_plan_accepts(h, w, c):
    from marlenv.dqn import MAP_CONV_WAVES
    assert MAP_CONV_WAVES[0] == 0
    for waves in MAP_CONV_WAVES:
        rc, lay, _ = _plan(h, w, c, waves=waves)
        assert rc == 0
        assert lay.p16 % 16 == 0 and lay.p16 >= h * w
        assert lay.act_per_obs == 64 * lay.p16 and lay.fc1_w == 256 * 64 * lay.p16
        assert lay.cpad == {8: 8, 16: 16, 24: 32, 32: 32}[c] and lay.k1 == -(-9 * lay.cpad // 32) * 32
        assert lay.conv1_w == 32 * lay.k1 and lay.conv2_w == 64 * 288 and lay.conv3_w == 64 * 576
        assert lay.lds_conv <= 160 * 1024


def test_map_plan_full_map_tiles():
    """20x20: dqn_row_of's conflict-free assignment takes 26 row tiles."""
    rc, lay, _ = _plan(20, 20, 8)
    assert rc == 0 and lay.p16 == 416 and lay.act_per_obs == 26624


@pytest.mark.parametrize('h,w,c,a', mc.PLAN_REJECTS)
def test_map_plan_rejects(h, w, c, a):
    rc, _, L = _plan(h, w, c, a)
    assert rc == -1                                  # SNAKE_E_CONFIG
    assert b'fp32' in L.snake_last_error()


def test_map_plan_rejects_other_conv_waves():
    from marlenv.dqn import MAP_CONV_WAVES
    for waves in (1, 2, 4, 7, 12, 32, -1):
        assert waves not in MAP_CONV_WAVES
        assert _plan(20, 20, 8, waves=waves)[0] == -1


def test_window_plan_still_rejects_the_full_map():
    assert _plan(20, 20, 8, fn='snake_dqn_plan')[0] == -1
    assert _plan(11, 11, 8, fn='snake_dqn_plan')[0] == 0


@pytest.mark.parametrize('h,w,c', mc.PLAN_ACCEPTS + ((22, 22, 8), (13, 13, 16), (2, 2, 8), (1, 1, 8)))
def test_map_rows_cover_every_position_once(h, w, c):
    from marlenv import _native
    L = _native.lib()
    cfg = _native.DqnCfg(h, w, c, 3)
    n = L.snake_dqn_map_rows(ctypes.byref(cfg), None, 0)
    assert n == _plan(h, w, c)[1].p16
    rows = (ctypes.c_int32 * (n + 1))(*([-7] * (n + 1)))
    assert L.snake_dqn_map_rows(ctypes.byref(cfg), ctypes.cast(rows, ctypes.c_void_p), n) == n
    assert rows[n] == -7
    rows = list(rows)[:n]
    assert sorted(x for x in rows if x >= 0) == list(range(h * w))
    assert all(x == -1 for x in rows if x < 0)
    for t in range(n // 16):     # a tile's border cells differ mod 16: distinct LDS banks
        q = [((p // w + 1) * (w + 2) + p % w + 1) % 16 for p in rows[16 * t:16 * t + 16] if p >= 0]
        assert len(set(q)) == len(q)
    assert L.snake_dqn_map_rows(ctypes.byref(cfg), ctypes.cast((ctypes.c_int32 * n)(), ctypes.c_void_p), n - 1) < 0


def test_map_rows_equal_the_window_rows():
    """On the window path's geometries both paths use one row assignment."""
    from marlenv import _native
    L = _native.lib()
    for s in dp.GRID_SIZES:
        cfg = _native.DqnCfg(s, s, 8, 3)
        n = L.snake_dqn_rows(ctypes.byref(cfg), None, 0)
        a, b = (ctypes.c_int32 * n)(), (ctypes.c_int32 * n)()
        assert L.snake_dqn_rows(ctypes.byref(cfg), ctypes.cast(a, ctypes.c_void_p), n) == n
        assert L.snake_dqn_map_rows(ctypes.byref(cfg), ctypes.cast(b, ctypes.c_void_p), n) == n
        assert list(a) == list(b)


def test_plan_keyword_is_checked_before_the_device():
    from marlenv.dqn import DQNForward
    p = dp.probe(3, 3, 8, 3, 0, mc.GRID_B)
    with pytest.raises(ValueError):
        DQNForward(p.state, 3, 3, 8, 3, device='cpu', plan='band')


@pytest.mark.parametrize('key', KEYS, ids=['%dx%dx%d-a%d-s%d-b%d' % k for k in KEYS])
def test_map_probe_valid(key):
    p = dp.probe(*key)
    for name, t in p.state.items():
        assert bool((t == t.round()).all()) and float(t.abs().max()) <= 256, name
        assert torch.equal(t.to(torch.bfloat16).float(), t), name
    for name in dp.ROUNDED:
        t = p.acts[name]
        assert bool((t == t.round()).all()) and float(t.min()) >= 0 and float(t.max()) <= 256, (name, float(t.max()))
        assert torch.equal(t.to(torch.bfloat16).double(), t), name
    assert bool((p.acts['h2'] == p.acts['h2'].round()).all()) and bool((p.q == p.q.round()).all())
    assert float(p.q.abs().max()) < 2 ** 24
    # the largest |partial sum| any summation order can meet in a layer
    for name, src in zip(dp.LAYERS + ('fc3',), dp.ROUNDED + ('h2',)):
        w = p.state[name + '.weight'].double()
        worst = (float(p.acts[src].abs().max()) * float(w.abs().reshape(w.size(0), -1).sum(1).max())
                 + float(p.state[name + '.bias'].abs().max()))
        assert worst < 2 ** 24, name
    assert int(p.obs.max()) == 1          # 0/1 bytes: no /255 anywhere
    for name in dp.LAYERS:
        wt = p.state[name + '.weight']
        if wt.dim() == 4:
            wt = wt.permute(0, 2, 3, 1).reshape(wt.size(0), -1)
        assert bool((wt != 0).any(0).all()), name + ' has an all-zero column'


@pytest.mark.parametrize('geo', mc.SHARP_GEO, ids=['%dx%dx%d' % g for g in mc.SHARP_GEO])
def test_map_probe_sharpness(geo):
    """>= 90 % of single zeroed weights change the features, per layer, on the
    lowest single net of the seeds (tests/test_dqn_probe_cpu.py's measure)."""
    pooled, lowest = sharpness(*geo, seeds=mc.SEEDS, B=mc.GRID_B)
    print('sharpness %dx%dx%d pooled %s lowest %s' % (geo + (pooled, lowest)))
    for name in dp.LAYERS:
        assert lowest[name] >= 0.90, (name, lowest[name], pooled[name])
