"""Device time of the `random` streams (snake_pyrandom_act and
snake_pyrandom_sample, pyrandom_kernels.hip) beside the torch glue they can
replace, which stays the default path.

The method is scripts/replay_bench.py's: each call is timed by its own pair of
HIP events, all enqueued behind ~30 ms of filler work so that the GPU never
waits for the host inside a timed span; 100 calls, three repeats, each repeat's
median kept; inputs rotate. Both paths of a comparison run in the same process
on the same tensors.

  sample     ReplayBuffer.sample(512), draw plus gather, on a full ring (count
             = 3 * capacity + 7) of pushed random observations: capacities
             10 000 (the reference's BUFFER_SIZE) and 1 048 576, observations
             11x11x8 and 20x20x8.
               torch  sample(512): rand(capacity), arange, compare, masked_fill_,
                      topk(capacity, 512), then the gather
               hip    sample(512, rng=r): snake_pyrandom_sample, then the gather
             and each draw alone (the torch draw as the same five ops).
  act        Q-values to actions at 4 096 x 4 and 65 536 x 4 snakes, 3 actions,
             epsilon 0.1 and 1.0 (every snake draws randrange), over 8 rotating
             Q tensors and skip masks with a quarter of the snakes done.
               torch  argmax, rand, randint, where, masked_fill, to(int8)
               hip    PyRandom.act: one launch
  iteration  scripts/actor_bench.py's training iteration (4 096 envs x 4 snakes,
             Collector.run(actor, 1, 0.1) then update(*buf.sample(512)), ring of
             131 072) without and with rng.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'marl-snake_amd'))

import torch  # noqa: E402

BATCH = 512
SHAPES = {'vision5_11x11x8': (11, 11, 8, 5), 'config_20x20x8': (20, 20, 8, None)}      # h, w, c, vision_range
CAPACITIES = (10000, 1 << 20)
ACT_ENVS = (4096, 65536)
SNAKES, ACTIONS = 4, 3
ITER_ENVS, ITER_CAPACITY = 4096, 1 << 17


def medians_us(fn, inputs, launches, warmup, repeats):
    out = []
    for _ in range(repeats):
        for i in range(warmup):
            fn(inputs[i % len(inputs)])
        torch.cuda.synchronize()
        filler = torch.empty(1 << 28, dtype=torch.float32, device='cuda')
        for _ in range(60):
            filler.add_(1.0)
        evs = []
        for i in range(launches):
            x = inputs[i % len(inputs)]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(x)
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
        del filler
        us = sorted(a.elapsed_time(b) * 1e3 for a, b in evs)
        out.append(us[len(us) // 2])
    return out


def spread(v):
    return {'median_us': sorted(v)[len(v) // 2], 'repeats_us': v}


def compare(rec, key, hip, tor):
    rec[key + '_hip'], rec[key + '_torch'] = spread(hip), spread(tor)
    rec[key + '_hip_over_torch'] = rec[key + '_hip']['median_us'] / rec[key + '_torch']['median_us']


def full_buffer(h, w, c, capacity, g):
    """A ring that has wrapped, filled by pushes of random 0/1 observations."""
    from marlenv import ReplayBuffer
    buf = ReplayBuffer((SNAKES, h, w, c), capacity)
    N = 4096
    obs = (torch.rand((N, SNAKES, h, w, c), device='cuda', generator=g) < 0.25).to(torch.uint8)
    nxt = (torch.rand((N, SNAKES, h, w, c), device='cuda', generator=g) < 0.25).to(torch.uint8)
    act = torch.randint(0, 3, (N, SNAKES), device='cuda', generator=g).to(torch.int8)
    rew = torch.randn((N, SNAKES), device='cuda', generator=g, dtype=torch.float64)
    done = torch.rand((N, SNAKES), device='cuda', generator=g) < 0.1
    for _ in range(-(-capacity // (N * SNAKES))):
        buf.push(obs, nxt, act, rew, done)
    buf.count.fill_(3 * capacity + 7)
    torch.cuda.synchronize()
    return buf


def measure_sample(args, g):
    from marlenv import PyRandom
    rec = {}
    for shape, (h, w, c, _) in SHAPES.items():
        for capacity in CAPACITIES:
            buf = full_buffer(h, w, c, capacity, g)
            rng = PyRandom(0)
            e = {'obs_shape': [h, w, c], 'capacity': capacity, 'batch': BATCH}

            def torch_draw(_):
                keys = torch.rand(capacity, device='cuda', generator=g)
                held = torch.arange(capacity, device='cuda') < buf.size()
                return torch.topk(keys.masked_fill_(~held, -1.0), BATCH).indices

            m = (args.launches, args.warmup, args.repeats)
            compare(e, 'sample', medians_us(lambda _: buf.sample(BATCH, rng=rng), (None,), *m),
                    medians_us(lambda _: buf.sample(BATCH, generator=g), (None,), *m))
            compare(e, 'draw', medians_us(lambda _: rng.sample(buf.count, capacity, BATCH), (None,), *m),
                    medians_us(torch_draw, (None,), *m))
            idx = rng.sample(buf.count, capacity, BATCH)
            e['gather'] = spread(medians_us(lambda _: buf.sample(idx=idx), (None,), *m))
            assert int(rng.err.item()) == 0
            rec['%s_cap%d' % (shape, capacity)] = e
            del buf
            torch.cuda.empty_cache()
    return rec


def measure_act(args, g):
    from marlenv import PyRandom
    rec = {}
    for N in ACT_ENVS:
        rng = PyRandom(list(range(N)))
        inputs = [(torch.randn((N * SNAKES, ACTIONS), device='cuda', generator=g),
                   torch.rand((N, SNAKES), device='cuda', generator=g) < 0.25) for _ in range(8)]
        e = {'envs': N, 'snakes': SNAKES, 'actions': ACTIONS, 'key_bytes': N * 624 * 4}
        for eps in (0.1, 1.0):
            def torch_act(x):
                q, mask = x
                greedy = q.reshape(N, SNAKES, -1).argmax(dim=2)
                u = torch.rand((N, SNAKES), device='cuda', generator=g)
                rnd = torch.randint(0, 3, (N, SNAKES), device='cuda', generator=g)
                greedy = torch.where(u < eps, rnd, greedy)
                return greedy.masked_fill(mask, 0).to(torch.int8)

            compare(e, 'act_eps%g' % eps,
                    medians_us(lambda x: rng.act(x[0], SNAKES, eps, skip=x[1]), inputs, args.launches, args.warmup,
                               args.repeats),
                    medians_us(torch_act, inputs, args.launches, args.warmup, args.repeats))
        assert int(rng.err.item()) == 0
        rec['envs%d' % N] = e
    return rec


def measure_iteration(args):
    from marlenv import Collector, DQNLearner, PyRandom, ReplayBuffer, SnakeVecEnv
    nn = torch.nn

    class TorchDQN(nn.Module):
        def __init__(self, h, w, c, A):
            super().__init__()
            self.conv1, self.conv2 = nn.Conv2d(c, 32, 3, padding=1), nn.Conv2d(32, 64, 3, padding=1)
            self.conv3 = nn.Conv2d(64, 64, 3, padding=1)
            self.fc1, self.fc2, self.fc3 = nn.Linear(64 * h * w, 256), nn.Linear(256, 128), nn.Linear(128, A)

    rec = {}
    for shape, (h, w, c, vr) in SHAPES.items():
        torch.manual_seed(0)
        state = TorchDQN(h, w, c, ACTIONS).cuda().state_dict()
        e = {'obs_shape': [h, w, c], 'envs': ITER_ENVS, 'snakes': SNAKES, 'capacity': ITER_CAPACITY}
        runs = {}
        for name, use_rng in (('torch', False), ('hip', True)):
            kw = dict(height=20, width=20) if vr is None else dict(height=20, width=20, vision_range=vr)
            env = SnakeVecEnv(ITER_ENVS, num_snakes=SNAKES, seed=1, **kw)
            buf = ReplayBuffer(env.obs_shape, ITER_CAPACITY)
            lrn = DQNLearner(state, h, w, c, num_actions=ACTIONS)
            policy = lrn.actor()
            collector = Collector(env, buf)
            rng = PyRandom(list(range(ITER_ENVS + 1))) if use_rng else None
            collector.run(policy, steps=2, epsilon=0.5, rng=rng)

            def iteration(_=None):
                collector.run(policy, steps=1, epsilon=0.1, rng=rng)
                if rng is None:
                    lrn.update(*buf.sample(BATCH))
                else:
                    lrn.update(*buf.sample(BATCH, rng=rng, stream=ITER_ENVS))

            runs[name] = medians_us(iteration, (None,), args.launches, args.warmup, args.repeats)
            if rng is not None:
                assert int(rng.err.item()) == 0
            env.close()
            del env, buf, lrn, policy, collector
            torch.cuda.empty_cache()
        compare(e, 'iteration', runs['hip'], runs['torch'])
        rec[shape] = e
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--parts', default='sample,act,iteration')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pyrandom_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('pyrandom_bench.py needs the GPU: a CPU run cannot give a time')
    g = torch.Generator(device='cuda').manual_seed(0)
    rec = {'metric': 'pyrandom_us', 'device': torch.cuda.get_device_name(0), 'launches': args.launches,
           'warmup': args.warmup, 'repeats': args.repeats,
           'timing': 'one HIP event pair per call, enqueued behind ~30 ms of filler work; medians of each repeat',
           'torch': 'the default path: torch ops on a torch generator', 'hip': 'the same call with rng=PyRandom'}
    for part, fn in (('sample', lambda: measure_sample(args, g)), ('act', lambda: measure_act(args, g)),
                     ('iteration', lambda: measure_iteration(args))):
        if part in args.parts.split(','):
            rec[part] = fn()
            print('%s done' % part, file=sys.stderr, flush=True)
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(json.dumps(rec, indent=1) + '\n')


if __name__ == '__main__':
    main()
