"""Device time of the greedy-opponent kernel (snake_greedy_actions,
greedy_kernels.hip) in its two layouts, beside k_safe_actions and one plain
read of the same observations. The method is scripts/policy_bench.py's.

Per geometry -- cfg2: 4 096 envs x 4 snakes x 20x20x8 (full map), cfg3: 65 536
envs x 4 x 11x11x8 (vision_range 5) -- the env is stepped with the greedy
kernel's own actions, and K consecutive steps' inputs (observations, skip
masks, random bits, the directions going in) are kept, K chosen so that
together they exceed twice the 256 MiB Infinity Cache: the timed launches walk
round them, so every launch reads its observations from HBM as a step of a real
loop does. Each launch is timed by its own pair of HIP events, all enqueued
behind ~30 ms of filler work; the directions (updated in place) are put back
outside the timed span.

Timed in one process on the same tensors, `--reps` times in turn (read pass,
k_safe_actions, rows on 64 lanes, four snakes per wave, and again): the read
pass obs.view(int64).sum(), k_safe_actions on random Q-values with the same
directions, k_greedy<1> and, where the map has at most 16 rows, k_greedy<4>, the layout
such maps take (both through snake_debug_greedy_actions, the library's testing
aid that takes the layout as an argument).

Prints one JSON record and writes it to --out: per geometry and kernel the
median microseconds of every repetition, the median of those as a fraction of
the 8 TB/s the project's rooflines use, and the two conditions of DESIGN 4g:
greedy <= safe at each shape, and the packed layout's slowest median below the
rows layout's fastest. The record is written either way; the exit status is 1
when a condition does not hold.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'marl-snake_amd'))

import torch  # noqa: E402

from launch_timer import per_launch_us  # noqa: E402

HBM_PEAK = 8.0e12
L3_BYTES = 256 << 20
GEOMETRIES = {
    'cfg2': dict(num_envs=4096, num_snakes=4, height=20, width=20, snake_length=5, vision_range=None),
    'cfg3': dict(num_envs=65536, num_snakes=4, height=20, width=20, snake_length=3, vision_range=5),
}


def greedy_call(ga, x, rows_only):
    """snake_debug_greedy_actions: rows_only = 1 is the rows-on-64-lanes layout
    whatever the height, 0 the layout snake_greedy_actions takes."""
    from marlenv import _native
    P = ctypes.c_void_p
    N = x['obs'].shape[0]
    _native.check(_native.lib().snake_debug_greedy_actions(
        ctypes.byref(ga.cfg), P(x['obs'].data_ptr()), P(x['rnd'].data_ptr()), P(x['skip'].data_ptr()),
        P(x['dirs'].data_ptr()), P(x['actions'].data_ptr()), ctypes.c_int64(N),
        P(torch.cuda.current_stream().cuda_stream), ctypes.c_int(rows_only)))


def measure(name, launches, warmup, settle, reps):
    from marlenv import GreedyActions, SafeActions, SnakeVecEnv
    kw = dict(GEOMETRIES[name])
    N = kw.pop('num_envs')
    env = SnakeVecEnv(N, seed=0, **kw)
    S, h = env.num_snakes, env.obs_shape[1]
    ga, sa = GreedyActions(env.obs_shape), SafeActions(env.obs_shape)
    g = torch.Generator(device='cuda').manual_seed(0)
    obs = env.reset()
    obs_bytes = obs.numel()
    K = max(3, -(-2 * L3_BYTES // obs_bytes))
    skip, inputs = None, []
    settle = max(1, settle)      # (the first call allocates ga.dirs)
    for t in range(settle + K):
        rnd = torch.randint(-2 ** 31, 2 ** 31, (N, S), dtype=torch.int32, device='cuda', generator=g)
        if t >= settle:
            z = torch.zeros((N, S), dtype=torch.uint8, device='cuda')
            inputs.append(dict(obs=obs, rnd=rnd, q=torch.randn((N, S, 3), generator=g, device='cuda'),
                               skip=z if skip is None else skip.to(torch.uint8),
                               dirs_in=ga.dirs.clone(), dirs=torch.empty_like(ga.dirs),
                               actions=torch.empty((N, S), dtype=torch.int8, device='cuda')))
        a = ga(obs, skip=skip, rnd=rnd)
        obs, _, done, info = env.step(a)
        ga.forget(info['episode_done'])
        skip = done & ~info['episode_done'][:, None]
    env.close()

    def restore(x):
        x['dirs'].copy_(x['dirs_in'])

    kernels = [('read_pass', lambda x: x['obs'].view(torch.int64).sum(), lambda x: None),
               ('safe_actions', lambda x: sa(x['obs'], x['q'], skip=x['skip'], dirs=x['dirs']), restore),
               ('greedy_rows', lambda x: greedy_call(ga, x, 1), restore)]
    if h <= 16:
        kernels.append(('greedy_packed', lambda x: greedy_call(ga, x, 0), restore))
    medians = {k[0]: [] for k in kernels}
    for _ in range(reps):
        for key, fn, before in kernels:
            medians[key].append(per_launch_us(fn, inputs, launches, warmup, before)[0])
    out = {'num_envs': N, 'obs_shape': list(env.obs_shape), 'obs_bytes': obs_bytes, 'inputs_in_rotation': K,
           'skipped_snakes_frac': float(torch.stack([x['skip'].float().mean() for x in inputs]).mean()),
           'unknown_dirs_frac': float(torch.stack([(x['dirs_in'][..., 0] == -128).float().mean()
                                                   for x in inputs]).mean())}
    for key, us in medians.items():
        mid = sorted(us)[len(us) // 2]
        out[key] = {'us_median_per_rep': us, 'us_median': mid,
                    'frac_of_8TBs': obs_bytes / (mid * 1e-6) / HBM_PEAK}
    used = 'greedy_packed' if h <= 16 else 'greedy_rows'
    out['layout_used'] = used
    out['greedy_not_slower_than_safe_actions'] = out[used]['us_median'] <= out['safe_actions']['us_median']
    if h <= 16:
        out['packed_slowest_below_rows_fastest'] = max(medians['greedy_packed']) < min(medians['greedy_rows'])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--settle', type=int, default=30, help='env steps before the kept inputs')
    ap.add_argument('--reps', type=int, default=3, help='interleaved repetitions of every kernel')
    ap.add_argument('--geometries', default='cfg2,cfg3')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'greedy_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('greedy_bench.py needs the GPU: a CPU run cannot give a time')
    rec = {'metric': 'greedy_actions_kernel_us', 'device': torch.cuda.get_device_name(0),
           'launches': args.launches, 'warmup': args.warmup, 'reps': args.reps,
           'timing': 'one HIP event pair per launch; inputs rotate over more than twice the Infinity Cache',
           'read_pass': 'obs.view(torch.int64).sum()'}
    for name in args.geometries.split(','):
        rec[name] = measure(name, args.launches, args.warmup, args.settle, args.reps)
    print(json.dumps(rec), flush=True)
    with open(args.out, 'w') as fp:
        fp.write(json.dumps(rec, indent=1) + '\n')
    failed = [name + ': ' + k for name in args.geometries.split(',')
              for k in ('greedy_not_slower_than_safe_actions', 'packed_slowest_below_rows_fastest')
              if rec[name].get(k) is False]
    if failed:
        sys.exit('conditions of DESIGN 4g that do not hold: ' + ', '.join(failed))


if __name__ == '__main__':
    main()
