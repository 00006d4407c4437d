"""bench.py's plain run, --full and --dump-outputs.

A plain run leaves the CPU baseline out (`cpu_baseline` null) and --full brings
it back; --dump-outputs writes what the last timed step returned as float32 /
float64 .npy files within 64 MB, the same bytes from run to run, equal to a
SnakeVecEnv stepped by hand with the benchmark's seeds and actions."""
import json
import sys

import numpy as np
import pytest

import bench

SMALL = ['--num-envs', '300', '--height', '12', '--width', '12', '--num-snakes', '3', '--vision-range', '3']


def _main(monkeypatch, capsys, argv):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.delenv('LOCAL_WORLD_SIZE', raising=False)
    monkeypatch.setattr(sys, 'argv', ['bench.py'] + argv)
    bench.main()
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith('{"metric"')]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_sample_rows_is_fixed_and_within_budget():
    assert bench.sample_rows(100, 8, 800) is None
    a, b = bench.sample_rows(65536, 15488, 32 << 20), bench.sample_rows(65536, 15488, 32 << 20)
    assert a.tobytes() == b.tobytes()
    assert len(a) == (32 << 20) // 15488 and len(a) * 15488 <= 32 << 20
    assert len(np.unique(a)) == len(a) and (np.diff(a) > 0).all() and 0 <= a[0] and a[-1] < 65536
    assert bench.DUMP_OBS_BYTES + bench.DUMP_REST_BYTES + 2 * 8 * 65536 <= 64 * 10**6


def test_dump_outputs_needs_a_timed_step(monkeypatch, capsys):
    with pytest.raises(SystemExit) as ex:
        _main(monkeypatch, capsys, ['--steps', '0', '--dump-outputs', 'x'])
    assert ex.value.code == 2


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(monkeypatch, capsys, tmp_path):
    import torch
    from marlenv import SnakeVecEnv
    steps, warmup = 23, 6
    argv = ['--gpus', '1', '--steps', str(steps), '--warmup', str(warmup)] + SMALL
    monkeypatch.setattr(bench, 'cpu_baseline', lambda *a, **k: pytest.fail('a plain run ran the CPU baseline'))
    monkeypatch.setattr(bench, 'DUMP_OBS_BYTES', 100 * 3 * 7 * 7 * 8 * 4)   # a sample of 100 of the 300 envs
    lines = [_main(monkeypatch, capsys, argv + ['--dump-outputs', str(tmp_path / d)]) for d in 'ab']
    line = lines[0]
    assert line['cpu_baseline'] is None and line['steps'] == steps and line['warmup'] == warmup
    assert line['ms_per_step'] > 0 and line['unit'] == 'env-steps/s' and line['higher_is_better'] is True
    assert line['value'] == pytest.approx(300 / (line['ms_per_step'] * 1e-3), rel=1e-2)   # (ms_per_step is rounded to 1e-4 ms)
    a, b = ({p.stem: np.load(p) for p in (tmp_path / d).glob('*.npy')} for d in 'ab')
    assert sorted(a) == sorted(b) == sorted(
        ['obs', 'obs_env_index', 'rewards', 'dones', 'episode_done', 'rank', 'error', 'episode_scores',
         'episode_steps', 'episode_fruits', 'episode_kills'])
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 * 10**6
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k

    # the same rollout by hand: env i seeded i, the actions of generator 12345
    dev = torch.device('cuda', torch.cuda.current_device())
    venv = SnakeVecEnv(300, num_snakes=3, device=dev, seed=0, height=12, width=12, snake_length=3,
                       vision_range=3, frame_stack=1)
    venv.reset()
    gen = torch.Generator(device=dev)
    gen.manual_seed(12345)
    actions = torch.randint(0, 3, (warmup + steps, 300, 3), generator=gen, device=dev, dtype=torch.int8)
    for t in range(warmup + steps):
        obs, rew, done, info = venv.step(actions[t])
    idx = a['obs_env_index'].astype(np.int64)
    assert len(idx) == 100 and a['obs'].shape == (100, 3, 7, 7, 8)
    assert (a['obs'] == obs.cpu().numpy()[idx]).all()
    assert a['rewards'].tobytes() == rew.cpu().numpy().tobytes()
    assert (a['dones'] == done.cpu().numpy()).all()
    for k in ('episode_done', 'rank', 'error', 'episode_scores', 'episode_steps', 'episode_fruits', 'episode_kills'):
        assert (a[k] == info[k].cpu().numpy()).all(), k
    assert rew.abs().sum() > 0


@pytest.mark.gpu
def test_full_run_adds_the_cpu_baseline(monkeypatch, capsys):
    """(the baseline itself is stood in for: it forks one worker per core, which
    a process that already holds the GPU should not do)"""
    seen = []

    def fake(env_kw, num_snakes, seconds, ratio_key):
        seen.append((env_kw['height'], num_snakes, seconds))
        return {'value': 1.0, 'unit': 'env-steps/s'}
    monkeypatch.setattr(bench, 'cpu_baseline', fake)
    argv = ['--gpus', '1', '--steps', '8', '--warmup', '4', '--cpu-seconds', '0.5'] + SMALL
    line = _main(monkeypatch, capsys, argv + ['--full'])
    assert seen == [(12, 3, 0.5)] and line['cpu_baseline'] == {'value': 1.0, 'unit': 'env-steps/s'}
    assert line['ms_per_step'] > 0
    assert _main(monkeypatch, capsys, argv + ['--full', '--no-cpu-baseline'])['cpu_baseline'] is None
    assert _main(monkeypatch, capsys, argv)['cpu_baseline'] is None and len(seen) == 1
