"""Device time of the genome-head kernel (snake_genome_actions,
genome_kernels.hip) alone, beside the feature extractor it follows.

Two batches of 128-feature rows -- one generation of train_ga.py, 100 genomes x
1 env x 4 snakes, and 4 096 envs x 4 snakes over the same 100 genomes -- and two
populations: `linear`, every genome the head of fc3_to_genome (3 output nodes x
128 links, GenomeHeads.from_linear's program with weights of its own), and
`random`, feed-forward genomes of 24 to 48 nodes with up to 16 links each and
mixed activations. The features are random float32 (a third of them zero, as
after a relu); K feature tensors rotate, but at 8 MiB a batch they stay in the
caches, as they do in a rollout where the extractor has just written them. Each
launch is timed by its own pair of HIP events, all enqueued behind ~30 ms of
filler work so that the GPU never waits for the host inside a timed span.

For scale, timed the same way in the same process: DQNForward.forward_features
(random weights, observations of random 0/1 bytes) on the same number of rows
-- fp32 and the bf16 map path on train_ga.py's 20x20x8 full map, and the bf16
window path on the 11x11x8 crop -- and one SnakeVecEnv.step of the same batch
(20x20 board, full-map observations).

Prints one JSON record and writes it to profiles/genome_bench.json.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'marl-snake_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from launch_timer import per_launch_us  # noqa: E402

I, A, S, G = 128, 3, 4, 100
BATCHES = {'generation_100x4': 100, 'envs_4096x4': 4096}


class Net:
    def __init__(self, node_evals):
        self.input_nodes = [-i - 1 for i in range(I)]
        self.output_nodes = list(range(A))
        self.node_evals = node_evals


def linear_population(rs):
    from marlenv.neat_head import LinearNetwork
    return [LinearNetwork(rs.randn(A, I).astype(np.float32) * 0.1, rs.randn(A).astype(np.float32)) for _ in range(G)]


def random_population(rs):
    nets = []
    for _ in range(G):
        hidden = int(rs.randint(24 - A, 48 - A + 1))
        order = [A + i for i in range(hidden)] + list(range(A))     # hidden nodes, then the outputs
        evals, seen = [], []
        for node in order:
            avail = [-i - 1 for i in range(I)] + seen
            k = int(rs.randint(1, 17))
            links = [(avail[int(j)], float(rs.uniform(-1, 1))) for j in rs.choice(len(avail), k, replace=False)]
            evals.append((node, ('relu', 'sigmoid', 'tanh')[int(rs.randint(3))], 'sum', float(rs.uniform(-1, 1)),
                          float(rs.uniform(-1, 1)), links))
            seen.append(node)
        nets.append(Net(evals))
    return nets


def random_dqn(precision, side):
    from marlenv import DQNForward
    g = torch.Generator().manual_seed(3)
    shapes = {'conv1.weight': (32, 8, 3, 3), 'conv1.bias': (32,), 'conv2.weight': (64, 32, 3, 3),
              'conv2.bias': (64,), 'conv3.weight': (64, 64, 3, 3), 'conv3.bias': (64,),
              'fc1.weight': (256, 64 * side * side), 'fc1.bias': (256,), 'fc2.weight': (128, 256),
              'fc2.bias': (128,), 'fc3.weight': (3, 128), 'fc3.bias': (3,)}
    state = {k: torch.randn(s, generator=g) * 0.05 for k, s in shapes.items()}
    return DQNForward(state, side, side, 8, num_actions=3, precision=precision)


def measure(N, populations, launches, warmup):
    from marlenv import GenomeHeads, SnakeVecEnv
    gen = torch.Generator(device='cuda').manual_seed(0)
    feats = []
    for _ in range(4):
        f = torch.randn((N * S, I), generator=gen, device='cuda')
        feats.append(torch.where(torch.rand((N * S, I), generator=gen, device='cuda') < 0.33, torch.zeros_like(f), f.abs()))
    rec = {'num_envs': N, 'rows': N * S}
    for name, nets in populations.items():
        heads = GenomeHeads(nets, num_inputs=I, genome_of_env=np.arange(N) % G)
        lay, tiles, _ = heads.tiles(S)
        med, mean = per_launch_us(lambda x: heads(x), feats, launches, warmup)
        sizes = np.diff(heads.program['node_off'])
        rec[name] = {'kernel_us_median': med, 'kernel_us_mean': mean, 'tiles': int(len(tiles)),
                     'scratch_tiles': int((tiles[:, 3] >= 0).sum()), 'lds_bytes': int(lay.lds_bytes),
                     'nodes_per_genome': [int(sizes.min()), int(sizes.max())],
                     'links': int(heads.cfg.num_links)}
    for precision, side in (('fp32', 20), ('bf16', 20), ('bf16', 11)):
        obs = [torch.randint(0, 2, (N * S, side, side, 8), generator=gen, device='cuda', dtype=torch.uint8)
               for _ in range(4)]
        net = random_dqn(precision, side)
        med, mean = per_launch_us(net.forward_features, obs, max(launches // 4, 10), max(warmup // 4, 3))
        rec['forward_features_%s_%dx%d_us_median' % (precision, side, side)] = med
        del obs, net
    env = SnakeVecEnv(N, num_snakes=S, height=20, width=20, snake_length=5, seed=0)
    env.reset()
    acts = [torch.randint(0, 3, (N, S), generator=gen, device='cuda').to(torch.int8) for _ in range(4)]
    rec['env_step_us_median'], _ = per_launch_us(env.step, acts, launches, warmup)
    env.close()
    step = rec['env_step_us_median'] + rec['forward_features_fp32_20x20_us_median']
    for name in populations:
        rec[name]['share_of_rollout_step'] = rec[name]['kernel_us_median'] / (step + rec[name]['kernel_us_median'])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'genome_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('genome_bench.py needs the GPU: a CPU run cannot give a time')
    rs = np.random.RandomState(0)
    populations = {'linear': linear_population(rs), 'random': random_population(rs)}
    rec = {'metric': 'genome_actions_kernel_us', 'device': torch.cuda.get_device_name(0),
           'launches': args.launches, 'warmup': args.warmup, 'inputs': I, 'outputs': A, 'genomes': G,
           'timing': 'one HIP event pair per launch behind ~30 ms of filler work; 4 inputs rotate (cache resident)',
           'rollout_step': 'env_step + forward_features_fp32_20x20 + the head kernel, device medians'}
    for name, N in BATCHES.items():
        rec[name] = measure(N, populations, args.launches, args.warmup)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(json.dumps(rec, indent=1) + '\n')


if __name__ == '__main__':
    main()
