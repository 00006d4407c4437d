"""snake_plan_paths (include/snake_env.h), the host-only description of the
kernel variants snake_step takes: every shape the GPU tests name for a path
(tests/plan_cases.py, expectations written down from the planner's rules) still
plans that path. No GPU needed."""
import ctypes
import os

import pytest

import plan_cases as P


@pytest.fixture(scope='module')
def native():
    from marlenv import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _native


@pytest.mark.parametrize('name', sorted(P.PLAN))
def test_case_plans_its_path(native, name):
    got = P.check(name)
    # the fields are consistent with each other whatever the shape
    kw, S, N, _ = P.PLAN[name]
    vr, fs = kw.get('vision_range'), kw.get('frame_stack', 1)
    oh, ow = (2 * vr + 1, 2 * vr + 1) if vr else (kw['height'], kw['width'])
    assert got['units'] == S * oh * ow * fs
    if got['encode'] in (P.DIRECT, P.ROWS):
        assert (got['enc_group'] == 0) == (got['encode'] == P.DIRECT)
    assert 0 <= got['enc_group'] <= S
    assert got['logic_lanes'] in (4, 8, 16) and got['logic_lanes'] >= min(S, 16) and got['logic_wpb'] in (1, 4)
    assert not (got['fused'] and got['background'])


def test_every_encode_and_link_is_named():
    """The table holds at least one shape per encode, per link record, and a
    staged encode with a partial last group."""
    exp = [e for _, _, _, e in P.PLAN.values()]
    assert {e['encode'] for e in exp if 'encode' in e} == {P.DIRECT, P.ROWS, P.TABLE, P.LEAN, P.LEAN_TABLE}
    assert {e['link'] for e in exp if 'link' in e} == {0, 1, 2}
    assert any(e.get('encode') == P.ROWS and 0 < e['enc_group'] < S and S % e['enc_group']
               for _, S, _, e in P.PLAN.values())
    assert any(e.get('units', 0) % 2 for e in exp)


def test_fused_needs_instep_spawn(native):
    """The one-launch step is eligible only with the spawn-ahead attempts in the
    step: the same board with the default background kernel is not."""
    kw, S, N, _ = P.PLAN['fused_vr5_s4']
    assert native.plan_paths(N, num_snakes=S, **kw)['fused'] == 1
    bg = native.plan_paths(N, num_snakes=S, **dict(kw, spawn_background=0))
    assert (bg['fused'], bg['background']) == (0, 1)


@pytest.mark.parametrize('kw,S,expect', [
    # the compat env of the golden replays (autoreset off): 20x20 full map plans the
    # table for the auto-reset step, k_encode stages two groups of two snakes
    (dict(height=20, width=20, autoreset=False), 4, dict(encode=P.ROWS, enc_group=2)),
    (dict(height=23, width=25, autoreset=False), 2, dict(encode=P.DIRECT, enc_group=0)),
    # a lean + table board under every-step auto-reset: P = 3872, groups of two
    (dict(height=40, width=40, vision_range=5, frame_stack=4, autoreset='every_step'), 8,
     dict(encode=P.ROWS, enc_group=2)),
    (dict(height=9, width=14, vision_range=3, autoreset='every_step'), 3, dict(encode=P.ROWS, enc_group=3)),
])
def test_k_encode_modes_stage_or_encode_directly(native, kw, S, expect):
    """Without the all-done auto-reset the step encodes in k_encode: staged rows
    or direct, whatever the auto-reset step of the same board plans."""
    got = native.plan_paths(1, num_snakes=S, **kw)
    assert {k: got[k] for k in expect} == expect
    assert (got['enc_per_wave'], got['enc_wpb'], got['desc_in_lds'], got['fused']) == (1, 1, 0, 0)


def test_plan_paths_errors(native):
    with pytest.raises(ValueError):
        native.plan_paths(16, num_snakes=17)
    c = native.SnakeCfg()
    assert native.lib().snake_plan_paths(ctypes.byref(c), 16, None) == -2
    assert native.ENCODE_PATHS[P.LEAN_TABLE] == 'lean_table' and len(native.ENCODE_PATHS) == 5


def test_rows_are_the_shapes_the_gpu_tests_run():
    """A row of the table and the GPU case of the same name are one shape."""
    import grow_policy
    import test_encode_blocks as eb
    import test_gpu_parity as gp
    for name, (kw, S, N, _) in P.PLAN.items():
        if name in grow_policy.CASES:
            assert grow_policy.CASES[name][:3] == (kw, S, N), name
        elif name in gp.BATCH_CASES:
            assert gp.BATCH_CASES[name][:3] == (kw, S, N), name
        elif name in gp.FULL_SIZE_CASES:
            assert gp.FULL_SIZE_CASES[name][:2] + (gp.FULL_SIZE_CASES[name][3],) == (N, S, kw), name
        else:
            assert name.startswith('geom_') and eb.GEOMETRIES[name[5:]] == (kw, S), name
