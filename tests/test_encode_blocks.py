"""The table encode's env-to-wave mapping (k_post runs several independent
encode waves per workgroup, four envs per wave; k_post_lean one workgroup per
two envs): seeded batches whose size is no multiple of a wave's or a
workgroup's envs, stepped against the CPU oracle and compared at every step
(bit-exact, as test_gpu_parity.test_batch_matches_oracle)."""
import numpy as np
import pytest

import plan_cases
from parity_util import compare_step, oracle_batch

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

ENVS_PER_WAVE = 4
WPB = (2, 3, 4)   # every workgroup width the plan may choose (snake_internal.h kEncWpbMax = 4)

# a last wave with fewer than four envs, a last workgroup with fewer live waves
# than it has, fewer envs than one wave
SIZES = sorted({1, 3, 67} | {ENVS_PER_WAVE * w + d for w in WPB for d in (-1, 1)})

# spawn_background=-1: k_post with the in-step workers (the path of the large
# batches); the default gives these small batches the background spawn kernel
# and the resets-only k_post
PATHS = {'instep': dict(spawn_background=-1), 'background': {}}

BOARD = dict(height=20, width=20, snake_length=3, vision_range=5)

GEOMETRIES = {
    # compact pattern stride 10 * S, unit counts that are no multiple of 128
    **{f's{s}_vr{vr}': (dict(height=20, width=20, vision_range=vr), s) for s in (1, 2, 3) for vr in (1, 4)},
    # the largest one-pass chunk count
    'full20_s4': (dict(height=20, width=20), 4),
    # more than four chunks per lane (descriptors in LDS) / three frame dwords per lane
    'fs2_12_vr3': (dict(height=12, width=12, vision_range=3, frame_stack=2), 4),
    'b24_vr3': (dict(height=24, width=24, vision_range=3), 4),
    # height != width (paths in plan_cases.PLAN under 'geom_' + name): table
    # encode in both orientations, a staged encode in groups of 3 of 4 snakes,
    # the direct encode
    **{k: plan_cases.PLAN['geom_' + k][:2] for k in ('rect_12x20_s4', 'rect_20x12_vr5_s4', 'rect_14x22_s4',
                                                     'rect_23x25_s2')},
}


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    from marlenv import _native
    _native.lib()


def _np(x):
    return {k: v.cpu().numpy() for k, v in x.items()} if isinstance(x, dict) else x.cpu().numpy()


def _run(oracle, kw, S, N, T, seed, where):
    from marlenv import SnakeVecEnv
    v = SnakeVecEnv(N, num_snakes=S, seed=seed, **kw)
    obs0 = _np(v.reset())
    okw = {k: x for k, x in kw.items() if k not in ('spawn_ahead', 'spawn_background')}   # GPU scheduling knobs only
    refs, robs = oracle_batch(oracle, N, seed, S, **okw)
    np.testing.assert_array_equal(obs0, robs)
    rs = np.random.RandomState(seed)
    resets = 0
    for t in range(T):
        a = rs.randint(0, 3, size=(N, S))
        obs, rew, done, info = v.step(torch.from_numpy(a))
        info = _np(info)
        resets += int(info['episode_done'].sum())
        compare_step(refs, range(N), a, _np(obs), _np(rew), _np(done), info,
                     grids=_np(v.grids()), where=f'{where} step {t}')
    return resets


@pytest.mark.parametrize('path', sorted(PATHS))
@pytest.mark.parametrize('N', SIZES)
def test_odd_batch_sizes(oracle, N, path):
    resets = _run(oracle, dict(BOARD, **PATHS[path]), 4, N, 60, 4000 + N, f'N={N} {path}')
    assert N < 8 or resets > 0, 'no episode ended: the reset-flag path was not taken'


@pytest.mark.parametrize('path', sorted(PATHS))
@pytest.mark.parametrize('geom', sorted(GEOMETRIES))
def test_geometries(oracle, geom, path):
    kw, S = GEOMETRIES[geom]
    if 'geom_' + geom in plan_cases.PLAN:
        plan_cases.check('geom_' + geom, dict(kw, **PATHS[path]), S, 37, **PATHS[path])
    _run(oracle, dict(kw, **PATHS[path]), S, 37, 40, 5000 + len(geom) + 7 * S, f'{geom} {path}')


@pytest.mark.parametrize('path', sorted(PATHS))
@pytest.mark.parametrize('wpb', WPB)
def test_all_envs_reset_in_one_step(oracle, wpb, path):
    """Truncation after five steps: every env resets in the same step, so the
    reset flag skips the encode of a wave's first and last env and of whole
    waves."""
    N = ENVS_PER_WAVE * wpb + 1
    resets = _run(oracle, dict(BOARD, max_episode_steps=5, **PATHS[path]), 4, N, 17, 6000 + N, f'trunc N={N} {path}')
    assert resets >= 3 * N


def test_lean_workgroups(oracle):
    """40x40 x 4 frames: k_post_lean's 256-thread table encode, two envs per workgroup."""
    _run(oracle, dict(height=40, width=40, vision_range=5, frame_stack=4), 8, 9, 30, 7009, 'lean N=9')
