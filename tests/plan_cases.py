"""Which kernel path each named test shape is meant to take: the expected fields
of snake_plan_paths (include/snake_env.h), written down by hand from the rules
of the planner (snake_capi.cpp build_kcfg's stages, and the shared predicates of
snake_internal.h) -- never read back from the library. The CPU test
tests/test_plan_paths.py asserts the whole table; the GPU tests assert a case's
row (check) before they step it, so a retuned threshold fails loudly instead of
silently dropping a path's coverage. tests/test_plan_consistency.py holds the
plan's fields to each other over a grid of shapes around every threshold.

Rows: name -> (board kwargs, num_snakes, num_envs, expected fields). Only the
fields that make the case what it is are listed.

How the expected values follow from the shape (P = obs bytes per snake =
oh * ow * 8 * frame_stack; fdw = frame_stack * H * W / 4 ring dwords,
frame_dwords), and the function that states each rule:
  lean    W % 4 == 0, an even unit count and 512 < fdw <= 2048 (lean_geom;
          kTblDwordsMax, kLeanDwordsMax)
  table   W % 4 == 0, an even unit count, fdw <= 512 and the carve (image,
          window origins, 1280 * S pattern bytes, 4 * units descriptor bytes)
          within 40 KB; on a lean board within 48 KB (plan_encode)
  rows    otherwise, where at least one snake's P fits 8 KB: groups of
          min(S, 8192 // P) snakes, an even number where P % 16 != 0
          (plan_staged_encode)
  direct  otherwise
  desc_in_lds   table encode with more than 256 unit pairs, or lean
          (tbl_desc_in_lds)
  background    batches of at most 8192 envs and 64 MiB of observations, or more
          than 8192 spawn poses; never with spawn_background=-1 or a draw
          record over 36 KB (more than 18 368 spawn poses: link 0) (bg_of,
          draw_record_fits)
  link    2 (u32 table in LDS) without the background kernel up to 32 768
          envs, else 1 (plan_worker_lds, link_record); 0 on lean boards
          (k_post_lean's workers) and over 18 368 poses (workers_global_links)
  logic_lanes   4 / 8 / 16 for S <= 4 / 8 / 16 (lanes_per_env), at least 8 up
          to 8192 envs (plan_logic)
  logic_wpb     1 where four waves' frames (64 / lanes envs each) exceed 160 KB
          (plan_logic)
"""
DIRECT, ROWS, TABLE, LEAN, LEAN_TABLE = range(5)

INSTEP = dict(spawn_background=-1)
_W12x20 = dict(height=12, width=20)
_T20x12 = dict(height=20, width=12, vision_range=5)
_F8x36 = dict(height=8, width=36, vision_range=5)
_FUSED = dict(encode=TABLE, fused=1, background=0, link=2, enc_per_wave=4)
_GROW12 = dict(height=12, width=12, snake_length=3, num_fruits=10, vision_range=3)

PLAN = {
    # ---- existing cases of test_gpu_parity whose comments claim a path
    'lean_40_s8_vr8_fs4': (dict(height=40, width=40, vision_range=8, frame_stack=4), 8, 16, dict(encode=LEAN)),
    'big_44_s4_global_links': (dict(height=44, width=44, snake_length=3, vision_range=4, spawn_ahead=4), 4, 16,
                               dict(encode=TABLE, link=0)),
    'big_100_l2': (dict(height=100, width=100, snake_length=2, vision_range=3), 4, 16, dict(logic_wpb=1)),
    's16': (dict(height=24, width=24, snake_length=2, vision_range=3), 16, 16, dict(logic_lanes=16)),
    'fused_vr5_s4': (dict(height=20, width=20, snake_length=3, vision_range=5, spawn_background=-1), 4, 128, _FUSED),
    'fused_full20_s4': (dict(height=20, width=20, snake_length=3, spawn_background=-1), 4, 96, _FUSED),
    'fused_coop_vr5_s4': (dict(height=20, width=20, vision_range=5, coop=True, spawn_background=-1), 4, 96, _FUSED),
    'fused_human_12_vr3': (dict(height=12, width=12, vision_range=3, observer='human', spawn_background=-1), 4, 64,
                           _FUSED),
    'fused_trunc_12_s2': (dict(height=12, width=12, max_episode_steps=7, spawn_background=-1), 2, 64, _FUSED),
    'fused_s2_vr4': (dict(height=12, width=12, vision_range=4, num_fruits=6, spawn_background=-1), 2, 64, _FUSED),
    'fused_24_vr3': (dict(height=24, width=24, vision_range=3, spawn_background=-1), 4, 64, _FUSED),
    # ---- FULL_SIZE_CASES
    'odd14_16384': (dict(height=14, width=14, vision_range=3), 4, 16384,
                    dict(encode=ROWS, enc_group=4, enc_per_wave=2)),
    'odd34_16384': (dict(height=34, width=34, vision_range=3), 4, 16384,
                    dict(encode=ROWS, enc_group=4, enc_per_wave=2)),
    'rect_12x20_vr5_16384': (dict(height=12, width=20, snake_length=3, vision_range=5), 4, 16384,
                             dict(encode=TABLE, logic_lanes=4, background=0)),
    'rect_14x22_vr3_16384': (dict(height=14, width=22, vision_range=3), 4, 16384,
                             dict(encode=ROWS, enc_group=4, enc_per_wave=2)),
    # ---- rectangular batches (BATCH_CASES): one per path and orientation
    # 960 units, 480 pairs: descriptors in LDS
    'rect_wide_12x20': (_W12x20, 4, 64, dict(encode=TABLE, desc_in_lds=1, units=960, background=1, link=1)),
    # 484 units: descriptors in registers, four encode waves per workgroup
    'rect_tall_20x12_vr5': (_T20x12, 4, 64, dict(encode=TABLE, desc_in_lds=0, units=484, enc_wpb=4, background=1)),
    # an 11x11 crop on a board 8 rows high
    'rect_flat_8x36_vr5': (_F8x36, 4, 64, dict(encode=TABLE, desc_in_lds=0, units=484, background=1)),
    'fused_rect_12x20': (dict(_W12x20, **INSTEP), 4, 64, dict(_FUSED, desc_in_lds=1)),
    'fused_rect_20x12_vr5': (dict(_T20x12, **INSTEP), 4, 64, dict(_FUSED, desc_in_lds=0)),
    'fused_rect_8x36_vr5': (dict(_F8x36, **INSTEP), 4, 64, dict(_FUSED, desc_in_lds=0)),
    # fdw = 960; carve 8128 + 10 240 + 15 488 bytes: lean with the table
    'rect_lean_24x40_fs4': (dict(height=24, width=40, vision_range=5, frame_stack=4, max_episode_steps=60), 8, 16,
                            dict(encode=LEAN_TABLE, units=3872, background=1, link=0)),
    # fdw = 960; 9248 units: the descriptors alone take 36 992 bytes, no table
    'rect_lean_40x24_vr8_fs4': (dict(height=40, width=24, vision_range=8, frame_stack=4, max_episode_steps=60), 8, 16,
                                dict(encode=LEAN, units=9248)),
    # fdw = 768, full map: oh = 32, ow = 48; 12 288 units, no table
    'rect_lean_32x48_fs2_full': (dict(height=32, width=48, frame_stack=2, max_episode_steps=60), 4, 16,
                                 dict(encode=LEAN, units=12288)),
    'rect_rows_14x9': (dict(height=14, width=9), 3, 64, dict(encode=ROWS, enc_group=3, units=378)),
    'rect_rows_9x14_vr3_fs2': (dict(height=9, width=14, vision_range=3, frame_stack=2), 3, 64,
                               dict(encode=ROWS, enc_group=3, units=294)),
    # 189 units: 8-byte stores
    'rect_rows_9x7_l2': (dict(height=9, width=7, snake_length=2), 3, 64, dict(encode=ROWS, enc_group=3, units=189)),
    'rect_rows_7x22_human_vr2': (dict(height=7, width=22, vision_range=2, observer='human'), 2, 64,
                                 dict(encode=ROWS, enc_group=2, units=50)),
    # P = 2464: three of the four snakes fit 8 KB, the last group is one snake
    'rect_rows_14x22_groups': (dict(height=14, width=22), 4, 64, dict(encode=ROWS, enc_group=3, units=1232)),
    'rect_rows_22x14_groups': (dict(height=22, width=14), 4, 64, dict(encode=ROWS, enc_group=3, units=1232)),
    # P = 4600 (8 mod 16): one snake fits, but a group must be even -> direct
    'direct_23x25': (dict(height=23, width=25), 2, 32, dict(encode=DIRECT, enc_group=0, units=1150)),
    'direct_25x23_s3': (dict(height=25, width=23), 3, 32, dict(encode=DIRECT, enc_group=0, units=1725)),
    # P = 4680 (8 mod 16)
    'direct_13x15_fs3': (dict(height=13, width=15, frame_stack=3), 2, 32, dict(encode=DIRECT, enc_group=0, units=1170)),
    # P = 12 800 > 8 KB; W % 4 == 0 but the table carve is 63 168 bytes
    'direct_40x40_s8_full': (dict(height=40, width=40, max_episode_steps=60), 8, 16,
                             dict(encode=DIRECT, enc_group=0, units=12800)),
    'rect_thin_5x255_vr4': (dict(height=5, width=255, vision_range=4), 2, 32, dict(encode=ROWS, enc_group=2, units=162)),
    'rect_thin_255x5_vr3_fs2': (dict(height=255, width=5, vision_range=3, frame_stack=2), 2, 32,
                                dict(encode=ROWS, enc_group=2, units=196)),
    # 22 352 spawn poses: global link tables; fdw = 540: lean, with the table
    'rect_big_30x72_vr4': (dict(height=30, width=72, vision_range=4, spawn_ahead=4, max_episode_steps=60), 4, 16,
                           dict(encode=LEAN_TABLE, link=0, background=0)),
    'rect_big_72x30_vr4': (dict(height=72, width=30, vision_range=4, spawn_ahead=4, max_episode_steps=60), 4, 16,
                           dict(encode=ROWS, enc_group=4, link=0, background=0)),
    # 8 envs of 9600 bytes per k_logic wave: 78 080 bytes, one wave per workgroup
    'rect_big_64x150_l2': (dict(height=64, width=150, snake_length=2, vision_range=3, max_episode_steps=60), 4, 16,
                           dict(encode=ROWS, logic_lanes=8, logic_wpb=1, link=0)),
    # ---- test_encode_blocks.GEOMETRIES (37 envs; both spawn paths plan the same encode)
    'geom_rect_12x20_s4': (_W12x20, 4, 37, dict(encode=TABLE, desc_in_lds=1)),
    'geom_rect_20x12_vr5_s4': (_T20x12, 4, 37, dict(encode=TABLE, desc_in_lds=0)),
    'geom_rect_14x22_s4': (dict(height=14, width=22), 4, 37, dict(encode=ROWS, enc_group=3)),
    'geom_rect_23x25_s2': (dict(height=23, width=25), 2, 37, dict(encode=DIRECT)),
    # ---- long snakes under the growing policy (grow_policy.CASES): the k_logic
    # instantiations whose body-ring code they are for
    # 32 envs: at least 8 lanes, and a small batch runs the background kernel
    'grow_12_s4': (_GROW12, 4, 32, dict(logic_lanes=8, background=1)),
    'fused_grow_12_s4': (dict(_GROW12, **INSTEP), 4, 32, _FUSED),
    # past 8192 envs S <= 4 runs 4 lanes per env, 16 envs per wave
    'grow_12_s4_16384': (_GROW12, 4, 16384, dict(logic_lanes=4)),
    'grow_24_s16': (dict(height=24, width=24, snake_length=2, num_fruits=40, vision_range=3), 16, 16,
                    dict(logic_lanes=16)),
}


def check(name, kw=None, S=None, N=None, **more):
    """Assert that shape `name` still plans the path of its row. kw / S / N, when
    given, are the shape the caller is about to run: they must be the row's
    (`more` = kwargs on top of the row's, e.g. the spawn path)."""
    from marlenv import _native
    pkw, pS, pN, expect = PLAN[name]
    if kw is not None:
        assert (dict(pkw, **more), pS, pN) == (kw, S, N), f'{name}: the shape run is not the shape planned'
    got = _native.plan_paths(pN, num_snakes=pS, **dict(pkw, **more))
    bad = {k: (got[k], v) for k, v in expect.items() if got[k] != v}
    assert not bad, f'{name}: plan differs from the path this case is for, (got, expected): {bad}'
    return got
