"""Long snakes and long episodes through every path of the step kernels' body
ring (logic_body in step_logic.h), against the CPU oracle, bit-exact.

a. Rollouts under the growing policy (grow_policy.py): snakes of 16 to 90 cells
   live, move, wrap their rings and die in lane groups g > 0, with 4, 8 and 16
   lanes per env, in the fused step, with frame stacks, with the background
   spawn kernel, on frames of more than 64 chunks, on the 16-byte ring and on a
   board that fills up. What each case reaches is asserted on the oracle alone
   in test_long_snakes_cpu.py, with the same seeds, batch and steps.
b. Death at every ring phase: injected snakes of 2 to 65 cells that move 0 to 19
   steps and then hit the wall.
c. The same states run into their own bodies.
d. A snapshot taken while long snakes live restores bit-identically.
"""
import numpy as np
import pytest

import grow_policy as gp
import plan_cases
from parity_util import compare_step

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu


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


def _np(x):
    return {k: v.cpu().numpy() for k, v in x.items()} if isinstance(x, dict) else x.cpu().numpy()


def _compare_tables(tab, refs, where):
    """snake_table() rows against OracleEnv.snakes(): alive flags of every
    snake; head, tail, direction and length of the live ones."""
    for row, r in enumerate(refs):
        ref = r.snakes()
        assert (tab[row, :, 5] == ref[:, 5]).all(), f'{where} env row {row}: alive {tab[row, :, 5]} != {ref[:, 5]}'
        live = ref[:, 5] == 1
        assert (tab[row][live] == ref[live]).all(), f'{where} env row {row}: table\n{tab[row]}\n!=\n{ref}'


SMALL_CASES = sorted(c for c, (_, _, N, _) in gp.CASES.items() if N <= 4096)


@pytest.mark.parametrize('case', SMALL_CASES)
def test_policy_rollout_matches_oracle(oracle, case, request):
    from marlenv import SnakeVecEnv
    if case.startswith('fused_'):
        request.getfixturevalue('fused_on')
    kw, S, N, T = gp.CASES[case]
    if case in plan_cases.PLAN:
        plan_cases.check(case, kw, S, N)
    v = SnakeVecEnv(N, num_snakes=S, seed=gp.SEED, **kw)
    obs0 = _np(v.reset())
    refs = [oracle.OracleEnv(seed=gp.SEED + i, num_snakes=S, **gp.oracle_kwargs(kw)) for i in range(N)]
    np.testing.assert_array_equal(obs0, np.stack([r.reset() for r in refs]))
    for t in range(T):
        a = gp.batch_actions(refs)
        obs, rew, done, info = v.step(torch.from_numpy(a))
        where = f'{case} step {t}'
        compare_step(refs, range(N), a, _np(obs), _np(rew), _np(done), _np(info),
                     grids=_np(v.grids()), where=where)
        _compare_tables(_np(v.snake_table()), refs, where)
    v.close()


def test_policy_rollout_full_size(oracle):
    """16 384 envs, 4 lanes per env and 16 envs per k_logic wave: the sampled
    envs play the policy against their oracle twins, the others play seeded
    random actions; whole-batch invariants every 10th step."""
    from marlenv import SnakeVecEnv
    case = 'grow_12_s4_16384'
    kw, S, N, T = gp.CASES[case]
    plan_cases.check(case, kw, S, N)
    vr = kw['vision_range']
    v = SnakeVecEnv(N, num_snakes=S, seed=gp.SEED, **kw)
    obs = v.reset()
    idx = gp.sampled_envs(N)
    refs = [oracle.OracleEnv(seed=gp.SEED + int(i), num_snakes=S, **kw) for i in idx]
    sel = torch.from_numpy(idx).cuda()
    np.testing.assert_array_equal(_np(obs[sel]), np.stack([r.reset() for r in refs]))
    g = torch.Generator(device='cuda').manual_seed(4321)
    deaths34 = grow16 = 0
    for t in range(T):
        a = torch.randint(0, 3, (N, S), generator=g, device='cuda', dtype=torch.int8)
        pa = gp.batch_actions(refs)
        a[sel] = torch.from_numpy(pa).to(a)
        before = [r.snakes() for r in refs]
        obs, rew, done, info = v.step(a)
        sub = {k: x[sel].cpu().numpy() for k, x in info.items()}
        d = _np(done[sel])
        where = f'{case} step {t}'
        compare_step(refs, range(len(idx)), pa, _np(obs[sel]), _np(rew[sel]), d, sub,
                     grids=_np(v.grids()[sel]), where=where)
        _compare_tables(_np(v.snake_table()[sel]), refs, where)
        for row, (i, r) in enumerate(zip(idx, refs)):   # what this batch is for, seen on the GPU's dones
            b = before[row]
            deaths34 += int(((b[:, 5] == 1) & d[row] & (b[:, 6] >= 34)).sum())
            if i % 16 and not d[row].all():
                grow16 += int(((b[:, 6] == 15) & (r.snakes()[:, 6] == 16)).sum())
        if t % 10:
            continue
        tab = v.snake_table()
        alive = tab[..., 5].bool()
        centre = obs[:, :, vr, vr, 5]
        heads = obs[..., 5].sum(dim=(2, 3))
        assert torch.equal(centre.bool() | ~alive, torch.ones_like(alive))
        assert torch.equal(heads[alive], torch.ones_like(heads[alive]))
        assert int(heads[~alive].sum()) == 0
        assert not bool(info['error'].any())
    assert deaths34 >= 1 and grow16 >= 1, (deaths34, grow16)
    v.close()


def _ring_batch(oracle, kind, S):
    """The injected (L, t) batch in a SnakeVecEnv and its oracle twins."""
    from marlenv import SnakeVecEnv
    cases = gp.ring_cases(kind)
    H, W = gp.RING_BOARD['height'], gp.RING_BOARD['width']
    v = SnakeVecEnv(len(cases), num_snakes=S, seed=3, autoreset=False, **gp.RING_BOARD)
    v.reset()
    refs = []
    for i, (L, t) in enumerate(cases):
        r = oracle.OracleEnv(seed=3 + i, num_snakes=S, **gp.RING_BOARD)
        r.reset()
        grid, snakes, alive = gp.ring_state(L, i % S, S, H, W)
        v.inject(i, grid, snakes, alive)
        r.inject(grid, snakes, alive)
        refs.append(r)
    return v, refs, cases


def _run_ring(oracle, kind, S):
    v, refs, cases = _ring_batch(oracle, kind, S)
    N = len(cases)
    slot = np.arange(N) % S
    death = np.array([gp.ring_death_step(kind, t) for _, t in cases])
    rd = gp.RING_BOARD['reward_dict']
    for step in range(int(death.max()) + 2):   # (one step past the last death: dead snakes stay dead)
        a = np.zeros((N, S), np.int64)
        a[np.arange(N), slot] = [gp.ring_action(kind, t, step) for _, t in cases]
        obs, rew, done, info = v.step(torch.from_numpy(a))
        obs, rew, done, info = _np(obs), _np(rew), _np(done), _np(info)
        grids, tab, alive_n = _np(v.grids()), _np(v.snake_table()), _np(v.alive_counters())
        for i, r in enumerate(refs):
            L, t = cases[i]
            where = f'{kind} S={S} L={L} t={t} step {step}'
            if step > death[i]:   # the episode is over: nothing of the snake comes back
                assert (grids[i] <= gp.WALL).all() and not tab[i, :, 5].any(), where
                continue
            ro, rr, rdone, rinfo = r.step(a[i])
            assert (grids[i] == r.grid).all(), f'{where}: grid\n{grids[i]}\n!=\n{r.grid}'
            assert rr.tobytes() == rew[i].tobytes(), f'{where}: rew {rew[i]} != {rr}'
            assert (rdone == done[i]).all(), f'{where}: done {done[i]} != {rdone}'
            assert bool(info['episode_done'][i]) == bool(rinfo), where
            assert int(alive_n[i]) == r.alive_snakes, where
            if rinfo:
                assert list(info['rank'][i]) == [int(x) for x in rinfo['rank']], where
                for k in ('episode_scores', 'episode_steps', 'episode_fruits', 'episode_kills'):
                    assert info[k][i].tobytes() == rinfo[k].tobytes(), (where, k)
            assert (ro == obs[i]).all(), f'{where}: obs'
            ref = r.snakes()
            assert (tab[i, :, 5] == ref[:, 5]).all(), where
            live = ref[:, 5] == 1
            assert (tab[i][live] == ref[live]).all(), f'{where}: table {tab[i]} != {ref}'
            if step == death[i]:
                assert rdone[slot[i]] and bool(rinfo), where
                assert (grids[i] <= gp.WALL).all(), f'{where}: cells of the dead snake remain\n{grids[i]}'
                if kind == 'self':   # the kill goes to the owner of the cell: the snake itself
                    assert rew[i, slot[i]] == rd['lose'] + rd['kill'], where
            else:
                assert not rdone[slot[i]] and ref[slot[i], 6] == L, where
    v.close()


@pytest.mark.parametrize('S', [1, 4])
def test_death_at_every_ring_phase(oracle, S):
    _run_ring(oracle, 'wall', S)


@pytest.mark.parametrize('S', [1, 4])
def test_self_collision_of_long_snakes(oracle, S):
    _run_ring(oracle, 'self', S)


def test_tour_on_a_nearly_full_16_byte_ring(oracle):
    """Snakes of 12 to 15 cells walk a closed tour of the 16 interior cells of a
    6x6 board for three turns of their 16-byte rings: every tail refill comes
    from a chunk that also holds the head word, the deque's end wrapped in
    right behind the head. The policy never reaches this on that board."""
    from marlenv import SnakeVecEnv
    cases = gp.cycle_cases()
    N = len(cases)
    v = SnakeVecEnv(N, num_snakes=1, seed=5, autoreset=False, **gp.CYCLE_BOARD)
    assert v.layout.ring_cap == 16
    v.reset()
    refs = []
    for i, (L, start) in enumerate(cases):
        r = oracle.OracleEnv(seed=5 + i, num_snakes=1, **gp.CYCLE_BOARD)
        r.reset()
        state = gp.cycle_state(L, start)
        v.inject(i, *state)
        r.inject(*state)
        refs.append(r)
    for step in range(gp.CYCLE_STEPS):
        a = np.array([[gp.cycle_action(start, step)] for _, start in cases])
        obs, rew, done, info = v.step(torch.from_numpy(a))
        obs, rew, done, grids = _np(obs), _np(rew), _np(done), _np(v.grids())
        where = f'tour step {step}'
        assert not done.any() and not _np(info['episode_done']).any(), where
        for i, r in enumerate(refs):
            ro, rr, rdone, _ = r.step(a[i])
            assert (grids[i] == r.grid).all(), f'{where} {cases[i]}: grid\n{grids[i]}\n!=\n{r.grid}'
            assert rr.tobytes() == rew[i].tobytes() and not rdone.any(), (where, cases[i])
            assert (ro == obs[i]).all(), (where, cases[i])
        _compare_tables(_np(v.snake_table()), refs, where)
    v.close()


def test_snapshot_with_long_snakes(oracle):
    """state_dict() with snakes past the whole tail queue alive (ring words,
    pending head bits and refilled queues in the snapshot) -> 40 steps ->
    load_state_dict() -> the same 40 actions: bit-identical, in the same env
    and in a fresh one."""
    from marlenv import SnakeVecEnv
    case, T0, K = 'grow_12_s4', 150, 40
    kw, S, N, _ = gp.CASES[case]
    plan_cases.check(case, kw, S, N)
    v = SnakeVecEnv(N, num_snakes=S, seed=gp.SEED, **kw)
    v.reset()
    refs = [oracle.OracleEnv(seed=gp.SEED + i, num_snakes=S, **kw) for i in range(N)]
    for r in refs:
        r.reset()

    def play(where):
        a = gp.batch_actions(refs)
        obs, rew, done, info = v.step(torch.from_numpy(a))
        compare_step(refs, range(N), a, _np(obs), _np(rew), _np(done), _np(info), grids=_np(v.grids()), where=where)
        return a, (obs.clone(), rew.clone(), done.clone(), info['episode_done'].clone(), v.grids().clone(),
                   v.snake_table().clone())

    for t in range(T0):
        play(f'snapshot warm-up step {t}')
    tabs = np.stack([r.snakes() for r in refs])
    long_live = int(((tabs[..., 5] == 1) & (tabs[..., 6] >= 16)).sum())
    assert long_live >= 1, 'no live snake of 16 cells at the snapshot'
    snap, snap_cpu = v.state_dict(), v.state_dict(device='cpu')
    acts, ref_out = zip(*[play(f'snapshot step {T0 + t}') for t in range(K)])

    def replay(env):
        outs = []
        for a in acts:
            o, r, d, i = env.step(torch.from_numpy(a))
            outs.append((o.clone(), r.clone(), d.clone(), i['episode_done'].clone(), env.grids().clone(),
                         env.snake_table().clone()))
        return outs

    v.load_state_dict(snap)
    again = replay(v)
    fresh = SnakeVecEnv(N, num_snakes=S, seed=999, **kw)
    fresh.load_state_dict(snap_cpu)
    other = replay(fresh)
    for t, (a, b, c) in enumerate(zip(ref_out, again, other)):
        for x, y, z in zip(a, b, c):
            assert torch.equal(x, y) and torch.equal(x, z), f'step {T0 + t}'
    v.close()
    fresh.close()
