"""CPU checks of the safe-action rule (no GPU needed): the numpy restatement
(tests/policy_ref.py) reproduces every record of the reference's own
DQN_Evaluator.get_action (tests/golden/policy_calls.npz), the fixture covers
every rule, and the host-side plan check accepts and rejects what it should."""
import ctypes
import os

import numpy as np
import pytest

import policy_ref as R


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
    assert sorted(calls) == ['b10x14', 'b12', 'full20', 'vr5']
    for name, c in calls.items():
        act, dout, _ = R.safe_actions(c['obs'], c['q'], c['skip'], c['din'])
        np.testing.assert_array_equal(act, c['act'], err_msg=name)
        np.testing.assert_array_equal(dout, c['dout'], err_msg=name)


def test_fixture_covers_every_rule(calls):
    """Each of the rules a reference rollout reaches (occupied, deadly, beside a
    head, fill) decides in at least 20 records, and at least 20 records hold a
    snake whose direction is unknown."""
    decided = {r: 0 for r in (R.OCCUPIED, R.DEADLY_CELL, R.NEAR_HEAD, R.FILL)}
    unknown = 0
    for c in calls.values():
        rule = R.safe_actions(c['obs'], c['q'], c['skip'], c['din'])[2]
        for r in decided:
            decided[r] += int((rule == r).any(axis=1).sum())
        unknown += int(((c['din'] == R.UNKNOWN).all(axis=2) & (c['skip'] == 0)).any(axis=1).sum())
    print({R.RULE_NAMES[r]: n for r, n in decided.items()}, 'unknown', unknown)
    for r, n in decided.items():
        assert n >= 20, (R.RULE_NAMES[r], n)
    assert unknown >= 20
    shapes = {c['obs'].shape[1:4] for c in calls.values()}
    assert any(h != w for _, h, w in shapes)            # one non-square board


def plan(native, h, w, c, S, limit=60):
    cfg = native.PolicyCfg(h, w, c, S, limit)
    rc = native.lib().snake_policy_plan(ctypes.byref(cfg))
    return rc, native.lib().snake_last_error().decode()


def test_plan_accepts(native):
    assert plan(native, 20, 20, 8, 4)[0] == 0
    assert plan(native, 64, 64, 8, 16)[0] == 0
    assert plan(native, 1, 1, 8, 1, limit=1)[0] == 0


@pytest.mark.parametrize('args,msg', [
    ((20, 20, 16, 4), 'obs_c'), ((65, 20, 8, 4), 'obs_h'), ((20, 65, 8, 4), 'obs_w'), ((20, 20, 8, 17), 'num_snakes'),
    ((20, 20, 8, 0), 'num_snakes'), ((0, 20, 8, 4), 'obs_h'), ((20, 20, 8, 4, 0), 'fill_limit'),
])
def test_plan_rejects(native, args, msg):
    rc, err = plan(native, *args)
    assert rc == -1
    assert msg in err
    with pytest.raises(ValueError):
        native.check(rc)


def test_call_rejects_bad_arguments_on_the_host(native):
    """Bad arguments return before any device work, so this runs without a GPU."""
    L = native.lib()
    buf = (ctypes.c_uint8 * 64)()
    P = ctypes.c_void_p
    a = ctypes.addressof(buf)
    a16 = (a + 15) & ~15
    ok = native.PolicyCfg(2, 2, 8, 1, 60)
    for cfg, obs, q, dirs, act, n, rc, msg in [
        (native.PolicyCfg(2, 2, 16, 1, 60), a16, a, a, a, 1, -1, 'obs_c'),
        (native.PolicyCfg(65, 2, 8, 1, 60), a16, a, a, a, 1, -1, 'obs_h'),
        (native.PolicyCfg(2, 2, 8, 17, 60), a16, a, a, a, 1, -1, 'num_snakes'),
        (native.PolicyCfg(2, 2, 8, 1, 0), a16, a, a, a, 1, -1, 'fill_limit'),
        (ok, None, a, a, a, 1, -2, 'NULL'), (ok, a16, None, a, a, 1, -2, 'NULL'),
        (ok, a16, a, None, a, 1, -2, 'NULL'), (ok, a16, a, a, None, 1, -2, 'NULL'),
        (ok, a16 + 8, a, a, a, 1, -2, 'aligned'), (ok, a16, a, a, a, -1, -2, 'num_envs'),
        (ok, a16, a, a, a, (1 << 26) + 1, -2, 'num_envs'),
    ]:
        got = L.snake_safe_actions(ctypes.byref(cfg), P(obs) if obs else None, P(q) if q else None, None,
                                   P(dirs) if dirs else None, P(act) if act else None, n, None)
        assert got == rc, (msg, got)
        assert msg in L.snake_last_error().decode()
        assert 'snake_safe_actions' in L.snake_last_error().decode() or rc == -1
    assert L.snake_safe_actions(ctypes.byref(ok), P(a16), P(a), None, P(a), P(a), 0, None) == 0   # no envs: no launch


def test_safe_actions_rejects_a_shape_before_any_device_work(native):
    """No GPU here: the constructor raises from the host-side plan check."""
    from marlenv import SafeActions
    for shape in ((4, 20, 20, 16), (4, 65, 20, 8), (17, 20, 20, 8), (20, 20, 8)):
        with pytest.raises(ValueError):
            SafeActions(shape)
    SafeActions((4, 20, 20, 8))
    SafeActions((16, 64, 64, 8), fill_limit=60)
