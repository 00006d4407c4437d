"""Device time of the safe-action kernel (snake_safe_actions, policy_kernels.hip)
alone, beside one plain read of the same observations.

Per geometry -- cfg2: 4 096 envs x 4 snakes x 20x20x8 (full map), cfg3: 65 536
envs x 4 x 11x11x8 (vision_range 5) -- the env is stepped with the kernel's own
actions on random Q-values, and K consecutive steps' inputs (observations, skip
masks, the directions going in) are kept, K chosen so that together they
exceed twice the 256 MiB Infinity Cache: the timed launches walk round them, so
every launch reads its observations from HBM as a step of a real loop does.
Each launch is timed by its own pair of HIP events, all enqueued behind ~30 ms
of filler work so that the GPU never waits for the host inside a timed span;
the directions (updated in place by the kernel) are put back outside it. The yardstick, timed
the same way in the same process on the same tensors, is one torch pass that
reads the observation tensor once: obs.view(int64).sum().

Prints one JSON record: per geometry the kernel's and the read pass's median
and mean microseconds, the observation bytes, both as a fraction of the 8 TB/s
the project's rooflines use, and kernel / read pass.
"""
import argparse
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


def measure(name, launches, warmup, settle):
    from marlenv import SafeActions, SnakeVecEnv
    kw = dict(GEOMETRIES[name])
    N = kw.pop('num_envs')
    env = SnakeVecEnv(N, seed=0, **kw)
    S = env.num_snakes
    sa = SafeActions(env.obs_shape)
    g = torch.Generator(device='cuda').manual_seed(0)
    obs = env.reset()
    obs_bytes = obs.numel()
    K = max(3, -(-2 * L3_BYTES // obs_bytes))
    skip, inputs = None, []
    settle = max(1, settle)      # (the first call allocates sa.dirs)
    for t in range(settle + K):
        q = torch.randn((N, S, 3), generator=g, device='cuda')
        if t >= settle:
            z = torch.zeros((N, S), dtype=torch.uint8, device='cuda')
            inputs.append(dict(obs=obs, q=q, skip=z if skip is None else skip.to(torch.uint8),
                               dirs_in=sa.dirs.clone(), dirs=torch.empty_like(sa.dirs)))
        a = sa(obs, q, skip=skip)
        obs, _, done, info = env.step(a)
        sa.forget(info['episode_done'])
        skip = done & ~info['episode_done'][:, None]
    env.close()

    def restore(x):
        x['dirs'].copy_(x['dirs_in'])

    k_med, k_mean = per_launch_us(lambda x: sa(x['obs'], x['q'], skip=x['skip'], dirs=x['dirs']),
                                  inputs, launches, warmup, restore)
    r_med, r_mean = per_launch_us(lambda x: x['obs'].view(torch.int64).sum(), inputs, launches, warmup)
    return {'num_envs': N, 'obs_shape': list(env.obs_shape), 'obs_bytes': obs_bytes, 'inputs_in_rotation': K,
            'skipped_snakes_frac': float(torch.stack([x['skip'].float().mean() for x in inputs]).mean()),
            'kernel_us_median': k_med, 'kernel_us_mean': k_mean,
            'read_pass_us_median': r_med, 'read_pass_us_mean': r_mean,
            'kernel_frac_of_8TBs': obs_bytes / (k_med * 1e-6) / HBM_PEAK,
            'read_pass_frac_of_8TBs': obs_bytes / (r_med * 1e-6) / HBM_PEAK,
            'kernel_over_read_pass': k_med / r_med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--settle', type=int, default=30, help='env steps before the kept inputs')
    ap.add_argument('--geometries', default='cfg2,cfg3')
    ap.add_argument('--out', default=None, help='also write the record to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('policy_bench.py needs the GPU: a CPU run cannot give a time')
    rec = {'metric': 'safe_actions_kernel_us', 'device': torch.cuda.get_device_name(0),
           'launches': args.launches, 'warmup': args.warmup,
           'timing': 'one HIP event pair per launch; inputs rotate over more than twice the Infinity Cache',
           'read_pass': 'obs.view(torch.int64).sum()'}
    for name in args.geometries.split(','):
        rec[name] = measure(name, args.launches, args.warmup, args.settle)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(json.dumps(rec, indent=1) + '\n')


if __name__ == '__main__':
    main()
