"""The long-snake cases (grow_policy.CASES) reach what they are for, asserted on
the CPU oracle alone with the seeds, batch sizes and step counts the GPU test
(test_long_snakes_gpu.py) runs: deaths of short, long and very long snakes, the
15 -> 16 growth past the whole tail queue off a wave's first lane group, long
tail moves, episodes longer than the body ring, several eaters in one step, and
respawns on a full board. Conditions, not measurements: a case that stops
reaching one of them no longer tests that code, so it fails here, without a GPU.
Also the policy rule itself on hand-made boards, and the injected ring-phase
scenarios (death by wall and by the own body at the planned step)."""
import numpy as np
import pytest

import grow_policy as gp


@pytest.mark.parametrize('name', sorted(gp.CASES))
def test_case_reaches_its_coverage(oracle, name):
    n = gp.coverage(oracle, name)
    print(name, n)
    missing = [k for k in gp.REQUIRED[name] if n[k] < 1]
    assert not missing, f'{name}: never reached {missing}: {n}'


def test_cases_and_requirements_agree():
    assert set(gp.CASES) == set(gp.REQUIRED)
    # the minimum ring and its 15 directions; rings of 64 and 128 bytes
    assert gp.ring_cap(gp.CASES['grow_6_s1_cap16'][0]) == 16
    assert gp.ring_cap(gp.CASES['grow_8_s2_full'][0]) == 64
    assert gp.ring_cap(gp.CASES['grow_12_s4'][0]) == 128
    # one frame of more than 64 16-byte chunks / of at most 64
    kw = gp.CASES['grow_36_s4'][0]
    assert kw['height'] * kw['width'] > 64 * 16 and kw.get('frame_stack', 1) == 1
    kw = gp.CASES['grow_12_s4'][0]
    assert kw['height'] * kw['width'] <= 64 * 16 and kw.get('frame_stack', 1) == 1
    assert gp.CASES['grow_16_s8_fs2'][0]['frame_stack'] == 2
    kw = gp.CASES['grow_rect_10x20_s3'][0]
    assert kw['height'] != kw['width']
    assert [gp.logic_lanes(S, N) for _, S, N, _ in (gp.CASES[c] for c in (
        'grow_12_s4', 'grow_12_s4_16384', 'grow_24_s16'))] == [8, 4, 16]


def _board(rows):
    """'#' wall, '.' empty, 'o' fruit, 'x' a body cell."""
    code = {'#': 1, '.': 0, 'o': 2, 'x': 4}
    return np.array([[code[ch] for ch in row] for row in rows])


def _snake(hr, hc, d, alive=1):
    return [hr, hc, 0, 0, d, alive, 3]


def test_policy_rule_on_small_boards():
    # nearest fruit: heading UP at (3, 2); keep -> (2, 2) is 1 from the fruit at
    # (1, 2), left -> (3, 1) is 3, right -> (3, 3) is 3
    g = _board(['#####', '#.o.#', '#...#', '#.x.#', '#####'])
    g[3, 2] = 3
    assert gp.actions(g, [_snake(3, 2, 0)]).tolist() == [0]
    # a tie in distance goes to the earlier action: fruit straight behind the
    # walls of a symmetric board, left (1) before right (2), keep blocked
    g = _board(['#####', '#.x.#', '#.x.#', '#o.o#', '#####'])
    g[2, 2] = 3
    assert gp.actions(g, [_snake(2, 2, 0)]).tolist() == [1]
    # a dead end loses to a farther open cell: keep -> (1, 1), whose neighbours
    # are walls and bodies, holds the fruit; right -> (2, 2) is open
    g = _board(['####', '#ox#', '#..#', '#..#', '####'])
    g[2, 1] = 3
    assert gp.actions(g, [_snake(2, 1, 0)]).tolist() == [2]
    # ... but a dead end is taken when it is the only candidate
    g = _board(['####', '#ox#', '#.x#', '####'])
    g[2, 1] = 3
    assert gp.actions(g, [_snake(2, 1, 0)]).tolist() == [0]
    # no candidate: 0; dead snakes: 0 whatever surrounds them
    g = _board(['#####', '#x.x#', '#.x.#', '#####'])
    g[1, 2] = 3
    assert gp.actions(g, [_snake(1, 2, 0), _snake(2, 1, 1, alive=0)]).tolist() == [0, 0]
    # a claimed cell is no candidate for a later slot: both heads next to the
    # fruit at (2, 2); slot 0 takes it, slot 1 (heading LEFT at (2, 3)) may not
    # keep and turns: left of LEFT is DOWN -> (3, 3), right is UP -> (1, 3);
    # equal distances, so left
    g = _board(['#####', '#...#', '#.o.#', '#...#', '#####'])
    g[2, 1], g[2, 3] = 3, 13
    assert gp.actions(g, [_snake(2, 1, 1), _snake(2, 3, 3)]).tolist() == [0, 1]
    # no fruit on the board: distance 0 everywhere, the first candidate
    g = _board(['#####', '#...#', '#...#', '#...#', '#####'])
    g[2, 2] = 3
    assert gp.actions(g, [_snake(2, 2, 2)]).tolist() == [0]


# ------------------------------------------------------ would the cases bite?
# ring_model.RingSnake, a host copy of the kernel's ring bookkeeping, follows the
# oracle through the cases: each live snake's new tail cell and each dying
# snake's erased cells are what a GPU run compares through the grid and the
# snake table. Without faults the copy never leaves the oracle; with one
# deliberate fault the named case leaves it in the named kind of step.
def _fresh_coords(grid, row, k):
    hr, hc, tr, tc, _, _, L = (int(x) for x in row)
    if L == 2:
        return [(hr, hc), (tr, tc)]
    assert L == 3
    (br, bc), = np.argwhere(grid == 4 + 10 * k)
    return [(hr, hc), (int(br), int(bc)), (tr, tc)]


def _follow_step(models, t0, g0, t1):
    """Advance one env's models by the oracle's step t0 -> t1; the first
    (kind, length) that differs from the oracle, or None."""
    for k, m in enumerate(models):
        if not t0[k, 5]:
            continue
        if t1[k, 5]:
            m.move(int(t1[k, 4]), bool(t1[k, 6] == t0[k, 6] + 1))
            assert m.head == (t1[k, 0], t1[k, 1])
            if m.tail != (t1[k, 2], t1[k, 3]):
                return 'tail', int(t0[k, 6])
        else:
            want = sorted(map(tuple, np.argwhere((g0 == 3 + 10 * k) | (g0 == 4 + 10 * k)).tolist()))
            if sorted(m.death_cells()) != want:
                return 'death', int(t0[k, 6])
    return None


def _follow_case(oracle, name, faults=()):
    from ring_model import RingSnake
    kw, S, N, T = gp.CASES[name]
    idx = gp.sampled_envs(N) if N > 4096 else np.arange(N)
    envs = [oracle.OracleEnv(seed=gp.SEED + int(i), num_snakes=S, **gp.oracle_kwargs(kw)) for i in idx]
    rings = [[bytearray(gp.ring_cap(kw)) for _ in range(S)] for _ in envs]

    def fresh(e, rg):
        e.reset()
        g, tab = e.grid, e.snakes()
        return [RingSnake(rg[k], _fresh_coords(g, tab[k], k), True, faults) for k in range(S)]

    models = [fresh(e, rg) for e, rg in zip(envs, rings)]
    for step in range(T):
        for j, e in enumerate(envs):
            g0, t0 = e.grid, e.snakes()
            done = e.step(gp.actions(g0, t0))[2]
            bad = _follow_step(models[j], t0, g0, e.snakes())
            if bad:
                return bad
            if done.all():
                models[j] = fresh(e, rings[j])
    return None


def _follow_ring(oracle, kind, faults=()):
    from ring_model import RingSnake
    H, W = gp.RING_BOARD['height'], gp.RING_BOARD['width']
    for L, t in gp.ring_cases(kind):
        e = oracle.OracleEnv(seed=0, num_snakes=1, **gp.RING_BOARD)
        e.reset()
        grid, snakes, alive = gp.ring_state(L, 0, 1, H, W)
        e.inject(grid, snakes, alive)
        models = [RingSnake(bytearray(gp.ring_cap(gp.RING_BOARD)), snakes[0][0], False, faults)]
        for step in range(gp.ring_death_step(kind, t) + 1):
            g0, t0 = e.grid, e.snakes()
            e.step([gp.ring_action(kind, t, step)])
            bad = _follow_step(models, t0, g0, e.snakes())
            if bad:
                return bad
    return None


def _follow_cycle(oracle, faults=()):
    from ring_model import RingSnake
    for L, start in gp.cycle_cases():
        e = oracle.OracleEnv(seed=0, num_snakes=1, **gp.CYCLE_BOARD)
        e.reset()
        grid, snakes, alive = gp.cycle_state(L, start)
        e.inject(grid, snakes, alive)
        models = [RingSnake(bytearray(gp.ring_cap(gp.CYCLE_BOARD)), snakes[0][0], False, faults)]
        for step in range(gp.CYCLE_STEPS):
            g0, t0 = e.grid, e.snakes()
            done = e.step([gp.cycle_action(start, step)])[2]
            assert not done.any(), (L, start, step)   # the tour never ends
            bad = _follow_step(models, t0, g0, e.snakes())
            if bad:
                return bad
    return None


def _follow(oracle, case, faults=()):
    if case == 'ring:cycle':
        return _follow_cycle(oracle, faults)
    if case.startswith('ring:'):
        return _follow_ring(oracle, case[5:], faults)
    return _follow_case(oracle, case, faults)


@pytest.mark.parametrize('name', sorted(gp.CASES) + ['ring:wall', 'ring:self', 'ring:cycle'])
def test_ring_copy_follows_the_oracle(oracle, name):
    assert _follow(oracle, name) is None


# fault -> the (case, kind of step) pairs that must see it; a case is a name of
# gp.CASES or the injected batch 'ring:wall' / 'ring:self'
BITES = {
    # short un-whole snakes exist only after inject: the refill of a snake of
    # fewer directions than the chunk holds reads below its head
    'refill_below_head': [('ring:wall', 'tail')],
    # the tail's chunk holds the head word: a snake of a few directions (the
    # policy's snakes refill only past 14 directions, and on the 16-byte ring a
    # snake that long fills the board and never moves its tail 14 times)
    'refill_no_pending': [('ring:wall', 'tail')],
    # a deque that fills its ring: only the tour on the 16-byte ring
    'refill_patch_tail': [('ring:cycle', 'tail')],
    'death_no_pending': [('ring:wall', 'death'), ('ring:self', 'death'), ('grow_12_s4', 'death'),
                         ('grow_6_s1_cap16', 'death'), ('grow_rect_10x20_s3', 'death')],
    'death_round_short': [('ring:wall', 'death'), ('ring:self', 'death'), ('grow_12_s4', 'death'),
                          ('grow_36_s4', 'death'), ('grow_12_s4_16384', 'death')],
    'death_no_wrap': [('ring:wall', 'death'), ('grow_12_s4', 'death'), ('grow_8_s2_full', 'death')],
    'handover_15th': [('grow_12_s4', 'tail'), ('grow_24_s16', 'tail'), ('grow_16_s8_fs2', 'tail')],
}


@pytest.mark.parametrize('fault', sorted(BITES))
def test_deliberate_fault_is_seen(oracle, fault):
    import ring_model
    assert set(BITES) == set(ring_model.FAULTS)
    for case, kind in BITES[fault]:
        got = _follow(oracle, case, (fault,))
        print(fault, case, got)
        assert got is not None and got[0] == kind, f'{fault}: {case} saw {got}, expected a wrong {kind} step'


@pytest.mark.parametrize('kind', ['wall', 'self'])
@pytest.mark.parametrize('S', [1, 4])
def test_ring_scenarios_on_the_oracle(oracle, kind, S):
    """Every (L, t) scenario does on the oracle what it is built for: the snake
    lives until its planned step, dies there (by its own body: with the kill
    credited to itself), and no cell of it remains."""
    H, W = gp.RING_BOARD['height'], gp.RING_BOARD['width']
    rd = gp.RING_BOARD['reward_dict']
    for i, (L, t) in enumerate(gp.ring_cases(kind)):
        slot = i % S
        e = oracle.OracleEnv(seed=i, num_snakes=S, **gp.RING_BOARD)
        e.reset()
        grid, snakes, alive = gp.ring_state(L, slot, S, H, W)
        e.inject(grid, snakes, alive)
        np.testing.assert_array_equal(e.grid, grid)
        assert e.snakes()[slot].tolist() == [1, 3, *gp.ring_path(L, H, W)[-1], 1, 1, L]
        for step in range(gp.ring_death_step(kind, t) + 1):
            a = np.zeros(S, np.int64)
            a[slot] = gp.ring_action(kind, t, step)
            _, rew, done, info = e.step(a)
            dies = step == gp.ring_death_step(kind, t)
            assert bool(done[slot]) == dies, (kind, L, t, step)
            if not dies:
                assert e.snakes()[slot, 6] == L and (e.grid % 10 == 3).sum() == 1
        assert rew[slot] == rd['lose'] + (rd['kill'] if kind == 'self' else 0.0), (kind, L, t, rew)
        assert info and info['episode_kills'][slot] == 0.0   # (a dying snake's step adds nothing)
        assert (e.grid <= gp.WALL).all(), (kind, L, t)
