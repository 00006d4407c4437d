"""The plan of snake_plan and snake_plan_paths (include/snake_env.h) agrees with
itself: relations between its fields that hold because the planner
(snake_capi.cpp build_kcfg's stages) and the launchers read one statement of
each rule (snake_internal.h), asserted for every row of tests/plan_cases.py and
on a grid of shapes on both sides of every threshold. No GPU needed."""
import ctypes
import itertools
import os

import pytest

import plan_cases as P

NS = (1, 8192, 8193, 16384, 32768, 32769, 65536, 65537)
SS = (1, 4, 5, 8, 9, 16)
AUTORESET = (False, True, 'every_step')
BACKGROUND = (-1, 0, 1)
# a board of each encode kind: name -> (kwargs, (num_snakes at which it is that kind, the kind))
BOARDS = {
    'direct': (dict(height=23, width=25), (4, P.DIRECT)),
    'rows': (dict(height=14, width=14, vision_range=3), (4, P.ROWS)),
    'table': (dict(height=12, width=20, vision_range=5), (4, P.TABLE)),
    'lean': (dict(height=40, width=24, vision_range=8, frame_stack=4), (8, P.LEAN)),
    'lean_table': (dict(height=24, width=40, vision_range=5, frame_stack=4), (8, P.LEAN_TABLE)),
    # 20 168 spawn poses: no draw record in LDS (more than 18 368)
    'big': (dict(height=44, width=44, vision_range=4), (4, P.TABLE)),
}
Q_SETS, SPAWN_RECORD_BYTES = 4, 672 * 4   # kQSets, kSpawnStride words


@pytest.fixture(scope='module')
def plans():
    """(label, kwargs, S, N, snake_layout, snake_plan_paths dict) of every shape, planned once."""
    from marlenv import _native
    from marlenv.config import build_cfg
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = _native.lib()

    def plan(label, kw, S, N):
        c = build_cfg(num_snakes=S, **kw)[0]
        lay = _native.SnakeLayout()
        assert L.snake_plan(ctypes.byref(c), N, ctypes.byref(lay)) == 0, (label, S, N, L.snake_last_error())
        return label, kw, S, N, lay, _native.plan_paths(N, num_snakes=S, **kw)

    out = [plan(name, kw, S, N) for name, (kw, S, N, _) in P.PLAN.items()]
    for (name, (kw, _)), N, S, ar, bg in itertools.product(BOARDS.items(), NS, SS, AUTORESET, BACKGROUND):
        out.append(plan(name, dict(kw, autoreset=ar, spawn_background=bg), S, N))
    return out


def each(plans):
    for label, kw, S, N, lay, got in plans:
        yield (label, kw, S, N), kw, S, N, lay, got


def test_boards_are_their_kind(plans):
    kinds = {(label, S): got['encode'] for label, kw, S, N, _, got in plans
             if label in BOARDS and N == 1 and kw['autoreset'] is True and kw['spawn_background'] == 0}
    for name, (_, (S, kind)) in BOARDS.items():
        assert kinds[name, S] == kind, name
    big = [lay.n_cand for label, _, _, _, lay, _ in plans if label == 'big']
    assert min(big) > 18368


def test_jscratch_iff_global_link_tables(plans):
    for what, _, _, _, lay, got in each(plans):
        assert (lay.jscratch > 0) == (got['link'] == 0), what


def test_fused_implies_its_path(plans):
    for what, _, _, _, _, got in each(plans):
        if got['fused']:
            assert got['encode'] == P.TABLE and got['link'] in (1, 2) and got['background'] == 0, what
            assert got['enc_per_wave'] == 4, what


def test_background_keeps_the_draw_record(plans):
    """... in LDS (link 1); k_post_lean's auto-reset workers keep no record in
    LDS whatever fits (link 0)."""
    for what, kw, _, _, _, got in each(plans):
        if got['background']:
            assert kw.get('autoreset', True) is True, what
            lean = got['encode'] in (P.LEAN, P.LEAN_TABLE)
            assert got['link'] == (0 if lean else 1), what


def test_descriptors_and_encode_blocks_are_the_table_encodes(plans):
    for what, _, _, _, _, got in each(plans):
        if got['desc_in_lds']:
            assert got['encode'] in (P.TABLE, P.LEAN_TABLE), what
        if got['enc_wpb'] > 1:
            assert got['encode'] == P.TABLE, what


def test_logic_lanes_hold_the_snakes(plans):
    for what, _, S, _, _, got in each(plans):
        assert got['logic_lanes'] >= min(16, max(4, 1 << (S - 1).bit_length())), what


def test_spawn_records_per_queue_set_iff_background(plans):
    for what, _, _, N, lay, got in each(plans):
        assert lay.spawn == (Q_SETS if got['background'] else 1) * N * SPAWN_RECORD_BYTES, what


def test_units(plans):
    for what, kw, S, _, lay, got in each(plans):
        vr = kw.get('vision_range')
        oh, ow = (2 * vr + 1, 2 * vr + 1) if vr else (kw['height'], kw['width'])
        assert (lay.obs_h, lay.obs_w) == (oh, ow), what
        assert got['units'] == S * oh * ow * kw.get('frame_stack', 1), what


def test_grid_reaches_both_sides(plans):
    """Every field the relations speak of takes each of its values somewhere on the grid."""
    seen = {k: {got[k] for *_, got in plans} for k in ('encode', 'link', 'fused', 'background', 'desc_in_lds')}
    assert seen == dict(encode={0, 1, 2, 3, 4}, link={0, 1, 2}, fused={0, 1}, background={0, 1}, desc_in_lds={0, 1})
    assert {got['enc_wpb'] > 1 for *_, got in plans} == {False, True}
    assert {got['logic_lanes'] for *_, got in plans} == {4, 8, 16}
    assert {lay.jscratch > 0 for _, _, _, _, lay, _ in plans} == {False, True}
