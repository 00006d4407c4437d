"""snake_seed / snake_reset / snake_step / snake_render_rgb as a C-API caller
(INTEGRATION.md): every state buffer at exactly its snake_plan byte count and
every output of every step at exactly layout.obs / .rew / .done / .ep_done /
.rank / .ep_stats / .err bytes, inside a guard-band arena (tests/guard_util.py).

After each step: snake_sync, the guards, then the step against the CPU oracle
(parity_util.compare_step, as test_encode_blocks._run). The outputs are
refilled with 0x5A before every call, so a byte the step did not write is
seen -- in particular rank and ep_stats where the episode goes on ("elsewhere
not written"), and the observation rows of envs a masked reset leaves out.

A read outside a buffer is invisible to this method."""
import ctypes

import numpy as np
import pytest

import plan_cases
from guard_util import FILL_BYTE, Arena
from parity_util import compare_step, oracle_batch

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

STEPS = 30
TRUNC = dict(max_episode_steps=12)
STATE = ('grid', 'snake', 'body', 'env', 'ctr', 'stats', 'mt', 'cand', 'jscratch', 'spawn', 'resetq')
OUTS = ('obs', 'rew', 'done', 'ep_done', 'rank', 'ep_stats', 'err')
OUT_DTYPES = dict(obs=np.uint8, rew=np.float64, done=np.uint8, ep_done=np.uint8, rank=np.int32,
                  ep_stats=np.float64, err=np.int32)
GPU_ONLY = ('spawn_ahead', 'spawn_background', 'autoreset')    # scheduling knobs the oracle does not have


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    from marlenv import _native
    _native.lib()


@pytest.fixture
def fused_on():
    from marlenv import _native
    _native.debug_set('fused', 1)
    yield
    _native.debug_set('fused', 0)


class CEnv:
    """The library driven through _native's structs alone: snake_plan, the state
    buffers (zeroed) and the outputs carved from one arena, snake_seed."""

    def __init__(self, N, S, seed, **kw):
        from marlenv import _native
        from marlenv.config import build_cfg
        self.nat, self.L = _native, _native.lib()
        self.N, self.S = N, S
        self.cfg, _ = build_cfg(num_snakes=S, **kw)
        self.lay = lay = _native.SnakeLayout()
        _native.check(self.L.snake_plan(ctypes.byref(self.cfg), N, ctypes.byref(lay)), self.L)
        sizes = {k: int(getattr(lay, k)) for k in STATE + OUTS}
        assert sizes['obs'] == N * S * lay.obs_h * lay.obs_w * lay.obs_c
        assert sizes['cand'] == 2 * int(lay.n_cand) * self.cfg.snake_length
        self.sizes = sizes
        extra = dict(actions=N * S, mask=N, rgb=N * self.cfg.height * self.cfg.width * 3)
        self.arena = ar = Arena(list(sizes.values()) + list(extra.values()))
        for k in STATE:
            if k == 'jscratch' and sizes[k] == 0:
                continue                                # NULL where its size is 0
            ar.take(k, sizes[k], fill='zero')
        host = np.zeros(sizes['cand'] // 2, np.int16)
        n = _native.check(self.L.snake_build_candidates(ctypes.byref(self.cfg), host.ctypes.data_as(ctypes.c_void_p),
                                                        host.size), self.L)
        assert n == lay.n_cand
        ar.payload('cand').copy_(torch.from_numpy(host.view(np.uint8)))
        for k in OUTS:
            ar.take(k, sizes[k])
        self.actions = ar.take('actions', extra['actions'], torch.int8, fill='zero')
        self.mask = ar.take('mask', extra['mask'], fill='zero')
        ar.take('rgb', extra['rgb'])
        self.state = _native.SnakeState(*[ar.ptr(k) if k in ar.names else None for k in STATE])
        self.out = _native.SnakeOut(*[ar.ptr(k) for k in OUTS])
        self.released = False
        self._call(self.L.snake_seed, N, ctypes.c_uint32(seed & 0xffffffff), 0, None)

    def _call(self, fn, *args):
        self.nat.check(fn(ctypes.byref(self.cfg), ctypes.byref(self.state), *args), self.L)

    def _fresh_outputs(self):
        for k in OUTS:
            self.arena.refill(k)

    def _finish(self, where):
        self._call(self.L.snake_sync, self.N, None)
        self.arena.check(where)
        return {k: self.arena.payload(k).cpu().numpy().view(OUT_DTYPES[k]) for k in OUTS}

    def reset(self, mask=None, where='reset'):
        self._fresh_outputs()
        m = None
        if mask is not None:
            self.mask.copy_(torch.from_numpy(np.asarray(mask, np.uint8)))
            m = self.arena.ptr('mask')
        self._call(self.L.snake_reset, self.N, m, ctypes.byref(self.out), None)
        return self._finish(where)

    def step(self, a, where='step'):
        self._fresh_outputs()
        self.actions.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.int8).reshape(-1)))
        self._call(self.L.snake_step, self.N, self.arena.ptr('actions'), ctypes.byref(self.out), None)
        return self._finish(where)

    def render(self, where='render'):
        from marlenv.core.render import palette
        pal = np.ascontiguousarray(palette())
        self.arena.refill('rgb')
        self._call(self.L.snake_render_rgb, self.N, pal.ctypes.data_as(ctypes.c_void_p), self.arena.ptr('rgb'), None)
        torch.cuda.synchronize()
        self.arena.check(where)
        H, W = self.cfg.height, self.cfg.width
        return self.arena.payload('rgb').cpu().numpy().reshape(self.N, H, W, 3)

    def obs(self, out):
        lay = self.lay
        return out['obs'].reshape(self.N, self.S, lay.obs_h, lay.obs_w, lay.obs_c)

    def state_bytes(self, k):
        return self.arena.payload(k).cpu().numpy().reshape(self.N, -1)

    def grids(self):
        """The newest ring slot of every env's grid (after snake_sync)."""
        fs, H, W = self.cfg.frame_stack, self.cfg.height, self.cfg.width
        ring = self.state_bytes('grid').reshape(self.N, fs, self.lay.grid_stride)
        cur = self.state_bytes('env').view(np.int32).reshape(self.N, 8)[:, 2]
        return ring[np.arange(self.N), cur][:, :H * W].reshape(self.N, H, W)

    def release(self):
        if not self.released:
            self.released = True
            self._call(self.L.snake_release, self.N)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()                                  # before the arena is dropped
        return False


def _info(env, out):
    """The step's info arrays, and the check that rank / ep_stats hold 0x5A in
    every row whose episode goes on."""
    N, S = env.N, env.S
    ended = out['ep_done'].astype(bool)
    assert set(np.unique(out['ep_done'])) <= {0, 1}
    rank, stats = out['rank'].reshape(N, S), out['ep_stats'].reshape(N, 4, S)
    on = ~ended
    assert (rank[on].view(np.uint8) == FILL_BYTE).all(), 'rank written where the episode goes on'
    assert (stats[on].view(np.uint8) == FILL_BYTE).all(), 'ep_stats written where the episode goes on'
    info = dict(episode_done=ended, rank=rank, error=out['err'])
    for j, k in enumerate(('episode_scores', 'episode_steps', 'episode_fruits', 'episode_kills')):
        info[k] = stats[:, j]
    return info


def _run(oracle, kw, S, N, seed, where, steps=STEPS):
    """`steps` steps of an all-done auto-reset env; returns the auto-resets seen."""
    okw = {k: x for k, x in kw.items() if k not in GPU_ONLY}
    n_act = 5 if kw.get('observer') == 'human' else 3
    with CEnv(N, S, seed, **kw) as env:
        refs, robs = oracle_batch(oracle, N, seed, S, **okw)
        np.testing.assert_array_equal(env.obs(env.reset(where=f'{where} reset')), robs)
        rs = np.random.RandomState(seed)
        resets = 0
        for t in range(steps):
            a = rs.randint(0, n_act, size=(N, S))
            w = f'{where} step {t}'
            out = env.step(a, where=w)
            info = _info(env, out)
            assert not out['err'].any(), w
            resets += int(info['episode_done'].sum())
            compare_step(refs, range(N), a, env.obs(out), out['rew'].reshape(N, S), out['done'].reshape(N, S), info,
                         grids=env.grids(), where=w)
    print(f'{where}: {resets} auto-resets in {N} envs x {steps} steps')
    return resets


def _row(name):
    """A row of plan_cases.PLAN with the 12-step truncation on top where the row
    has none of its own; its path is asserted before it runs. Returns the
    steps to run too: 30, or, where the row truncates at 60 steps itself (its
    boards are too large for random play to end an episode in 30: the oracle
    counts none), two steps past that truncation, so that every env resets."""
    pkw, S, N, _ = plan_cases.PLAN[name]
    more = {} if 'max_episode_steps' in pkw else TRUNC
    kw = dict(pkw, **more)
    plan_cases.check(name, kw, S, N, **more)
    return kw, S, N, max(STEPS, int(kw['max_episode_steps']) + 2)


ROWS = [
    'rect_tall_20x12_vr5', 'rect_wide_12x20',                               # table; descriptors in LDS
    'fused_vr5_s4', 'fused_rect_12x20',                                      # the one-launch step
    'lean_40_s8_vr8_fs4', 'rect_lean_24x40_fs4',                             # lean; lean + table
    'rect_rows_9x7_l2', 'rect_rows_14x22_groups', 'rect_rows_7x22_human_vr2',   # staged rows
    'direct_23x25', 'direct_13x15_fs3',                                      # direct
    'big_44_s4_global_links', 'rect_big_64x150_l2', 's16',                   # global links, one-wave k_logic, 16 lanes
]


@pytest.mark.parametrize('name', ROWS)
def test_plan_rows(oracle, name, request):
    if name.startswith('fused_'):
        request.getfixturevalue('fused_on')
    kw, S, N, steps = _row(name)
    resets = _run(oracle, kw, S, N, 9000 + 13 * len(name), name, steps)
    assert resets >= 1, f'{name}: no auto-reset in {steps} steps: the worker, link-table and spawn-record writes did not run'


RAGGED = dict(height=20, width=20, snake_length=3, vision_range=5)


@pytest.mark.parametrize('path', ['instep', 'background'])
@pytest.mark.parametrize('N', [1, 5, 37])
def test_table_ragged_batches(oracle, N, path):
    """Four envs per encode wave: one env, one wave and a bit, a last wave with one env."""
    from marlenv import _native
    kw = dict(RAGGED, **TRUNC, **(plan_cases.INSTEP if path == 'instep' else {}))
    got = _native.plan_paths(N, num_snakes=4, **kw)
    assert got['encode'] == plan_cases.TABLE and got['enc_per_wave'] == 4
    assert got['background'] == (0 if path == 'instep' else 1)
    resets = _run(oracle, kw, 4, N, 9100 + N, f'ragged N={N} {path}')
    assert resets >= 1


NOAUTO = {'table_board': (dict(RAGGED), 4, 5), 'rows_9x7_l2': (dict(plan_cases.PLAN['rect_rows_9x7_l2'][0]), 3, 5)}


@pytest.mark.parametrize('mode', [False, 'every_step'])
@pytest.mark.parametrize('board', sorted(NOAUTO))
def test_other_autoreset_modes(oracle, board, mode):
    """autoreset 0 (k_logic, k_encode: the terminal observation; the caller
    resets ended envs with a masked snake_reset) and 2 (k_logic, k_autoreset,
    k_encode: every env reset after every step)."""
    from marlenv import _native
    kw, S, N = NOAUTO[board]
    kw = dict(kw, **TRUNC)
    assert _native.plan_paths(N, num_snakes=S, autoreset=mode, **kw)['encode'] in (plan_cases.ROWS, plan_cases.DIRECT)
    seed = 9200 + len(board)
    with CEnv(N, S, seed, autoreset=mode, **kw) as env:
        refs, robs = oracle_batch(oracle, N, seed, S, **kw)
        np.testing.assert_array_equal(env.obs(env.reset()), robs)
        rs = np.random.RandomState(seed)
        ends = 0
        for t in range(STEPS):
            a = rs.randint(0, 3, size=(N, S))
            w = f'{board} autoreset={mode} step {t}'
            out = env.step(a, where=w)
            info = _info(env, out)
            obs, rew, done = env.obs(out), out['rew'].reshape(N, S), out['done'].reshape(N, S)
            ended = info['episode_done']
            ends += int(ended.sum())
            for i, r in enumerate(refs):
                ro, rr, rd, rinfo = r.step(a[i])
                assert rr.tobytes() == rew[i].tobytes(), (w, i)
                assert (rd == done[i]).all(), (w, i)
                assert bool(ended[i]) == bool(rinfo), (w, i)
                if rinfo:
                    assert list(info['rank'][i]) == [int(x) for x in rinfo['rank']], (w, i)
                    for k in ('episode_scores', 'episode_steps', 'episode_fruits', 'episode_kills'):
                        assert info[k][i].tobytes() == rinfo[k].tobytes(), (w, i, k)
                if mode == 'every_step':
                    ro = r.reset()
                assert (ro == obs[i]).all(), (w, i)
            if mode is False and ended.any():
                robs = env.obs(env.reset(mask=ended, where=w + ' masked reset'))
                for i in np.flatnonzero(ended):
                    assert (refs[i].reset() == robs[i]).all(), (w, i)
                assert (robs[~ended] == FILL_BYTE).all(), w
            assert (env.grids() == np.stack([r.grid for r in refs])).all(), w
    # every_step: k_autoreset reset every env after every step, checked against the
    # oracle above (an episode need not end: none lasts longer than one step);
    # autoreset 0: the caller's masked resets ran only if an episode ended
    assert mode == 'every_step' or ends >= 1, 'no episode ended'


@pytest.mark.parametrize('path', ['instep', 'background'])
def test_masked_reset_leaves_the_other_envs_alone(oracle, path):
    """snake_reset with env_mask 0,1,0,0,1 in the middle of the episodes: the
    observation rows of the unmasked envs keep 0x5A and their state slices are
    bit-equal before and after; the masked envs are the oracle's after its
    reset() (with the background spawn kernel their spawn-ahead records sit in
    the record buffer the status word names, not in buffer 0)."""
    N, S, seed = 5, 4, 9300
    kw = dict(RAGGED, **TRUNC, **(plan_cases.INSTEP if path == 'instep' else {}))
    mask = np.array([0, 1, 0, 0, 1], np.uint8)
    keep = mask == 0
    with CEnv(N, S, seed, **kw) as env:
        refs, robs = oracle_batch(oracle, N, seed, S, **{k: x for k, x in kw.items() if k not in GPU_ONLY})
        np.testing.assert_array_equal(env.obs(env.reset()), robs)
        rs = np.random.RandomState(seed)
        for t in range(7):
            a = rs.randint(0, 3, size=(N, S))
            out = env.step(a, where=f'step {t}')
            compare_step(refs, range(N), a, env.obs(out), out['rew'].reshape(N, S), out['done'].reshape(N, S),
                         _info(env, out), grids=env.grids(), where=f'step {t}')
        slices = ('grid', 'snake', 'body', 'ctr', 'stats', 'mt')
        before = {k: env.state_bytes(k) for k in slices}
        words = env.state_bytes('env').view(np.int32).reshape(N, 8)[:, :4].copy()
        out = env.reset(mask=mask, where='masked reset')
        obs = env.obs(out)
        assert (obs[keep] == FILL_BYTE).all(), 'observation rows of unmasked envs were written'
        for i in np.flatnonzero(mask):
            assert (refs[i].reset() == obs[i]).all(), i
        for k in slices:
            after = env.state_bytes(k)
            assert (after[keep] == before[k][keep]).all(), f'{k}: an unmasked env changed'
        assert (env.state_bytes('grid')[~keep] != before['grid'][~keep]).any(), 'the masked envs were not reset'
        assert (env.state_bytes('env').view(np.int32).reshape(N, 8)[keep, :4] == words[keep]).all()
        assert (env.grids() == np.stack([r.grid for r in refs])).all()
        for name in ('rew', 'done', 'ep_done', 'rank', 'ep_stats', 'err'):      # a reset writes obs only
            assert (out[name].view(np.uint8) == FILL_BYTE).all(), name


def test_render_rgb_at_189_bytes_per_env(oracle):
    """9x7, three envs: 567 bytes of rgb, no multiple of 4 or 16."""
    from oracle.snake_oracle import rgb_from_grid
    N, S, seed = 3, 3, 9400
    kw = dict(height=9, width=7, snake_length=2, **TRUNC)
    with CEnv(N, S, seed, **kw) as env:
        assert env.arena.payload('rgb').numel() == N * 9 * 7 * 3 == 567
        env.reset()
        rs = np.random.RandomState(seed)
        for t in range(9):
            if t % 4 == 0:
                rgb, grids = env.render(where=f'render {t}'), env.grids()
                for i in range(N):
                    np.testing.assert_array_equal(rgb[i], rgb_from_grid(grids[i]), err_msg=f't{t} env {i}')
            env.step(rs.randint(0, 3, size=(N, S)))
