"""Device time of the graph-observation kernel (snake_graph_obs,
graph_kernels.hip) beside a straightforward torch-indexing version of the same
rule on the same GPU and one plain read of the same observations. The method
is scripts/greedy_bench.py's.

The benchmark's configuration -- 65 536 envs x 4 snakes, 20x20, vision_range 5
(11x11x8 observations) -- is stepped with random actions, and K consecutive
steps' inputs (the observations and a copy of the snake records) are kept, K
chosen so that together they exceed twice the 256 MiB Infinity Cache: the
timed launches walk round them, so every launch reads its observations from
HBM as a step of a real loop does. Each call is timed by its own pair of HIP
events, all enqueued behind ~30 ms of filler work. k_graph_obs writes into one
output tensor allocated beforehand; the torch version allocates what it needs
from the caching allocator (no device allocation after the warm-up).

The torch version (torch_graph_obs below) is the yardstick: per ray step one
gather of the five rays' cells for every snake, a compare, a masked add and
the wall test, about a dozen launches per step of the ray. Its result is
checked against the kernel's, exactly, before anything is timed.

Prints one JSON record and writes it to --out: per variant the median
microseconds of every repetition and the median of those; for the kernel also
the bytes it has to move -- the output, the records, and one 8-byte cell per
ray step (an upper bound: a ray stops at a wall) -- over that time.
"""
import argparse
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'marl-snake_amd'))

import torch  # noqa: E402

from launch_timer import per_launch_us  # noqa: E402

HBM_PEAK = 8.0e12
L3_BYTES = 256 << 20
CONFIG = dict(num_envs=65536, num_snakes=4, height=20, width=20, snake_length=3, vision_range=5)
# the five rays' steps per direction code (0 UP, 1 RIGHT, 2 DOWN, 3 LEFT): F, L, R, F + L, F + R
UNIT = ((-1, 0), (0, 1), (1, 0), (0, -1))
RAY_STEPS = [[(dr, dc), (-dc, dr), (dc, -dr), (dr - dc, dc + dr), (dr + dc, dc - dr)] for dr, dc in UNIT]


def weights(n, float32_quotient):
    """The rule's weights (include/snake_env.h): (5, n) float64, one row per ray."""
    i = torch.arange(1, n + 1, dtype=torch.float64)
    diag = i * math.sqrt(2.0)
    if float32_quotient:
        axis, diag = (1.0 / i.float()).double(), (1.0 / diag.float()).double()
    else:
        axis, diag = 1.0 / i, 1.0 / diag
    return torch.stack([axis, axis, axis, diag, diag]).cuda()


def torch_graph_obs(obs, rec, vr, wt, steps_table):
    """source='own' of the rule with torch indexing: obs uint8 (N, S, h, w, C), rec
    int32 (N, S, 4). Returns float64 (N, S, 5, C)."""
    N, S, h, w, C = obs.shape
    n = wt.shape[1]
    x, y = rec[..., 0], rec[..., 1]
    alive = ((y >> 8) & 1).bool()
    steps = steps_table[(y & 3).long()]                     # (N, S, 5, 2)
    if vr:
        r0 = c0 = torch.full((N, S, 1), vr, dtype=torch.int64, device=obs.device)
    else:
        r0, c0 = (x & 255).long()[..., None], ((x >> 8) & 255).long()[..., None]
    flat = obs.view(N * S, h * w, C)
    snake = torch.arange(N * S, device=obs.device).view(N, S, 1)
    out = torch.zeros((N, S, 5, C), dtype=torch.float64, device=obs.device)
    going = alive[..., None].expand(N, S, 5).clone()
    zero = torch.zeros((), dtype=torch.float64, device=obs.device)
    for i in range(n):
        r, c = r0 + (i + 1) * steps[..., 0], c0 + (i + 1) * steps[..., 1]
        going &= (r >= 0) & (r < h) & (c >= 0) & (c < w)
        cell = flat[snake, r.clamp(0, h - 1) * w + c.clamp(0, w - 1)]      # (N, S, 5, C)
        out += torch.where(going[..., None] & (cell == 1), wt[:, i].view(1, 1, 5, 1), zero)
        going &= cell[..., 0] != 1
    return out


def kernel_call(cfg, x, out):
    from marlenv import _native
    P = ctypes.c_void_p
    _native.check(_native.lib().snake_graph_obs(
        ctypes.byref(cfg), P(x['obs'].data_ptr()), P(x['rec'].data_ptr()), P(out.data_ptr()),
        ctypes.c_int64(x['obs'].shape[0]), P(torch.cuda.current_stream().cuda_stream)))


def measure(launches, warmup, settle, reps, num_envs):
    from marlenv import GraphObs, SnakeVecEnv
    kw = dict(CONFIG)
    N = num_envs or kw.pop('num_envs')
    kw.pop('num_envs', None)
    env = SnakeVecEnv(N, seed=0, **kw)
    S, h, w, C = env.obs_shape
    vr = int(env.cfg.vision_range)
    graph = GraphObs(env)
    g = torch.Generator(device='cuda').manual_seed(0)
    obs = env.reset()
    obs_bytes = obs.numel()
    K = max(3, -(-2 * L3_BYTES // obs_bytes))
    inputs = []
    for t in range(settle + K):
        if t >= settle:
            inputs.append(dict(obs=obs, rec=env.snake.view(N, S, 4).clone()))
        obs = env.step(torch.randint(0, 3, (N, S), dtype=torch.int8, device='cuda', generator=g))[0]
    env.close()
    n = vr or 5
    wt = weights(n, vr == 0)
    steps_table = torch.tensor(RAY_STEPS, dtype=torch.int64, device='cuda')
    out = torch.empty((N, S, 5, C), dtype=torch.float64, device='cuda')
    for x in inputs:            # the yardstick computes what the kernel computes
        kernel_call(graph.cfg, x, out)
        assert torch.equal(out, torch_graph_obs(x['obs'], x['rec'], vr, wt, steps_table))
    variants = [('read_pass', lambda x: x['obs'].view(torch.int64).sum()),
                ('torch_indexing', lambda x: torch_graph_obs(x['obs'], x['rec'], vr, wt, steps_table)),
                ('k_graph_obs', lambda x: kernel_call(graph.cfg, x, out))]
    medians = {k: [] for k, _ in variants}
    for _ in range(reps):
        for key, fn in variants:
            medians[key].append(per_launch_us(fn, inputs, launches, warmup)[0])
    alive = torch.stack([((x['rec'][..., 1] >> 8) & 1).float().mean() for x in inputs]).mean()
    moved = out.numel() * 8 + N * S * 16 + N * S * 5 * n * C
    rec = {'num_envs': N, 'obs_shape': [S, h, w, C], 'obs_bytes': obs_bytes, 'out_bytes': out.numel() * 8,
           'bytes_moved_upper_bound': moved, 'inputs_in_rotation': K, 'alive_snakes_frac': float(alive)}
    for key, us in medians.items():
        rec[key] = {'us_median_per_rep': us, 'us_median': sorted(us)[len(us) // 2]}
    t = rec['k_graph_obs']['us_median'] * 1e-6
    rec['k_graph_obs']['bytes_per_s'] = moved / t
    rec['k_graph_obs']['frac_of_8TBs'] = moved / t / HBM_PEAK
    rec['torch_over_kernel'] = rec['torch_indexing']['us_median'] / rec['k_graph_obs']['us_median']
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--settle', type=int, default=30, help='env steps before the kept inputs')
    ap.add_argument('--reps', type=int, default=3, help='interleaved repetitions of every variant')
    ap.add_argument('--num-envs', type=int, default=0, help='0: the benchmark\'s 65 536')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'graph_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('graph_bench.py needs the GPU: a CPU run cannot give a time')
    rec = {'metric': 'graph_obs_kernel_us', 'device': torch.cuda.get_device_name(0),
           'launches': args.launches, 'warmup': args.warmup, 'reps': args.reps,
           'timing': 'one HIP event pair per call; inputs rotate over more than twice the Infinity Cache',
           'read_pass': 'obs.view(torch.int64).sum()'}
    rec['cfg3'] = measure(args.launches, args.warmup, args.settle, args.reps, args.num_envs)
    print(json.dumps(rec), flush=True)
    with open(args.out, 'w') as fp:
        fp.write(json.dumps(rec, indent=1) + '\n')


if __name__ == '__main__':
    main()
