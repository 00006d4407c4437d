"""CPU checks of the greedy opponent's rule (no GPU needed): the numpy
restatement (tests/greedy_ref.py) reproduces every record of the reference's
own GreedyEnemy.get_action (tests/golden/greedy_calls.npz), the fixture covers
every category of the rule, and the host-side argument checks of
snake_greedy_actions and GreedyActions reject what they should."""
import ctypes
import os

import numpy as np
import pytest

import greedy_ref as R


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


def test_restatement_reproduces_the_reference(calls):
    assert sorted(calls) == ['b10x14', 'b12', 'crafted', 'full20', 'vr5']
    for name, c in calls.items():
        act, dout, _ = R.greedy_actions(c['obs'], c['rnd'], c['skip'], c['din'])
        np.testing.assert_array_equal(act, c['act'], err_msg=name)
        np.testing.assert_array_equal(dout, c['dout'], err_msg=name)


def test_fixture_covers_every_category(calls):
    """Every category of greedy_ref occurs, the rollouts' own ones (all but a
    missing head) outside the crafted records too; unknown directions, both
    extremes of the random bits and a non-square board occur."""
    seen = {k: 0 for k in R.CATEGORY_NAMES}
    rolled = dict(seen)
    unknown, rnd = 0, set()
    for name, c in calls.items():
        cat = R.greedy_actions(c['obs'], c['rnd'], c['skip'], c['din'])[2]
        for k in seen:
            seen[k] += int(((cat & k) != 0).sum())
            if name != 'crafted':
                rolled[k] += int(((cat & k) != 0).sum())
        unknown += int(((c['din'] == R.UNKNOWN).all(axis=2) & (c['skip'] == 0)).sum())
        rnd |= set(c['rnd'][(cat & (R.N2 | R.N3)) != 0].tolist())
    print({R.CATEGORY_NAMES[k]: n for k, n in seen.items()}, 'unknown', unknown)
    for k, n in seen.items():
        assert n >= 1, R.CATEGORY_NAMES[k]
    for k, n in rolled.items():
        assert n >= 10 or k == R.NOHEAD, (R.CATEGORY_NAMES[k], n)
    assert unknown >= 20
    assert 0 in rnd and 0xFFFFFFFF in rnd              # (where the choice is among several moves)
    shapes = {c['obs'].shape[1:4] for c in calls.values()}
    assert any(h != w for _, h, w in shapes)


def test_pick_is_the_multiply_shift_rule():
    assert [R.pick(u, 3) for u in (0, 0x55555555, 0x55555556, 0xAAAAAAAA, 0xAAAAAAAB, 0xFFFFFFFF)] == [0, 0, 1, 1, 2, 2]
    assert [R.pick(u, 2) for u in (0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)] == [0, 0, 1, 1]
    assert R.pick(0xFFFFFFFF, 1) == 0


def test_neighbour_order_differs_from_the_evaluator():
    """A head with body above and below: the greedy rule asks the cell above
    first (direction (1, 0)), the evaluator's rule the cell below ((-1, 0))."""
    import policy_ref
    o = np.zeros((1, 1, 5, 5, 8), np.uint8)
    o[0, 0, 2, 2, 5] = 1
    o[0, 0, 1, 2, 6] = o[0, 0, 3, 2, 6] = 1
    din = np.full((1, 1, 2), R.UNKNOWN, np.int8)
    # heading (1, 0), forward (3, 2) is dead: the first best move is 1 = (-dx, dy) = (0, 1)
    assert R.greedy_actions(o, None, None, din)[1].tolist() == [[[0, 1]]]
    # heading (-1, 0), forward (1, 2) is masked: the first maximum is move 1 = (0, -1)
    q = np.array([[[1.0, 0.0, 0.0]]], np.float32)
    assert policy_ref.safe_actions(o, q, None, din)[1].tolist() == [[[0, -1]]]


def test_call_rejects_bad_arguments_on_the_host(native):
    """Bad arguments return before any device work, so this runs without a GPU."""
    L = native.lib()
    buf = (ctypes.c_uint8 * 64)()
    P = ctypes.c_void_p
    a = ctypes.addressof(buf)
    a16 = (a + 15) & ~15
    ok = native.PolicyCfg(2, 2, 8, 1, 60)
    for cfg, obs, dirs, act, n, rc, msg in [
        (native.PolicyCfg(2, 2, 16, 1, 60), a16, a, a, 1, -1, 'obs_c'),
        (native.PolicyCfg(65, 2, 8, 1, 60), a16, a, a, 1, -1, 'obs_h'),
        (native.PolicyCfg(2, 2, 8, 17, 60), a16, a, a, 1, -1, 'num_snakes'),
        (native.PolicyCfg(2, 2, 8, 1, 0), a16, a, a, 1, -1, 'fill_limit'),
        (ok, None, a, a, 1, -2, 'NULL'), (ok, a16, None, a, 1, -2, 'NULL'), (ok, a16, a, None, 1, -2, 'NULL'),
        (ok, a16 + 8, a, a, 1, -2, 'aligned'), (ok, a16, a, a, -1, -2, 'num_envs'),
        (ok, a16, a, a, (1 << 26) + 1, -2, 'num_envs'),
    ]:
        got = L.snake_greedy_actions(ctypes.byref(cfg), P(obs) if obs else None, None, None,
                                     P(dirs) if dirs else None, P(act) if act else None, n, None)
        assert got == rc, (msg, got)
        assert msg in L.snake_last_error().decode()
    assert L.snake_greedy_actions(ctypes.byref(ok), P(a16), None, None, P(a), P(a), 0, None) == 0   # no envs: no launch


def test_greedy_actions_rejects_before_any_device_work(native):
    import torch
    from marlenv import GreedyActions
    for shape in ((4, 20, 20, 16), (4, 65, 20, 8), (17, 20, 20, 8), (20, 20, 8)):
        with pytest.raises(ValueError):
            GreedyActions(shape)
    ga = GreedyActions((2, 5, 5, 8))
    with pytest.raises(TypeError):
        ga(torch.zeros((3, 2, 5, 5, 8), dtype=torch.float32))
    with pytest.raises(TypeError):
        ga(torch.zeros((3, 2, 5, 8, 5), dtype=torch.uint8).transpose(3, 4))
    with pytest.raises(ValueError):
        ga(torch.zeros((3, 2, 5, 6, 8), dtype=torch.uint8))
    with pytest.raises(ValueError, match='no CPU fallback'):
        ga(torch.zeros((3, 2, 5, 5, 8), dtype=torch.uint8))


def test_battle_rejects_a_wrong_controller_count():
    from marlenv import battle

    class Env:
        num_envs, num_snakes = 3, 4

    with pytest.raises(ValueError, match='one controller per snake slot'):
        battle(Env(), [None] * 3, 1)
