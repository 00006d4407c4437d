"""What the device-side pack (dqn_pack_kernels.hip) buys a training loop that
collects with the policy it is training.

Shapes: 20x20x8 (train_dqn.py's Config, the map plan) and 11x11x8 (vision range
5, the window plan). The method is scripts/learner_bench.py's: each call is
timed by its own pair of HIP events, all enqueued behind ~30 ms of filler work
so that the GPU never waits for the host inside a timed span; 100 calls, three
repeats, each repeat's median kept. Recorded per shape:

  pack            one snake_dqn_pack32 (actor.sync()), beside the least bytes it
                  moves -- every fp32 source read once, every destination
                  written once -- over the 8 TB/s HBM peak
  refresh_old     the same refresh without it: DQNForward(learner.state_dict(),
                  ...). It syncs with the host, so this one is wall-clock time
                  between two device synchronisations, host time included
  update_fp32 / update_bf16_target
                  DQNLearner.update at B = 512 with target_precision 'fp32'
                  (profiles/learner_bench.json's update_hip is its yardstick)
                  and 'bf16', and the target forward alone in both modes
  iteration_*     one training iteration at 4 096 envs x 4 snakes:
                  Collector.run(policy, steps=1) then update(*buf.sample(512)),
                  acting with the learner itself (fp32) against acting with
                  learner.actor() (bf16, repacked by every update); also as
                  wall-clock time per iteration of a 100-iteration loop
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'marl-snake_amd'))

HBM_PEAK = 8e12
SHAPES = {'config_20x20x8': (20, 20, 8, None), 'vision5_11x11x8': (11, 11, 8, 5)}      # h, w, c, vision_range
BATCH = 512
ENVS, SNAKES = 4096, 4
CAPACITY = 1 << 17


def pack_bytes(lay, h, w, c, A=3):
    """Least bytes of one pack: the fp32 sources read, the destinations written."""
    small = 32 + 64 + 64 + 256 + 128 + A * 128 + A
    src = 32 * 9 * c + 64 * 288 + 64 * 576 + 256 * 64 * h * w + 128 * 256 + small
    dst16 = lay.conv1_w + lay.conv2_w + lay.conv3_w + lay.fc1_w + lay.fc2_w
    return 4 * src + 2 * dst16 + 4 * small


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--shapes', default=','.join(SHAPES))
    ap.add_argument('--out', default=None, help='also write the record to this file')
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit('actor_bench.py needs the GPU: a CPU run cannot give a time')
    from marlenv import Collector, DQNLearner, ReplayBuffer, SnakeVecEnv
    from marlenv.dqn import DQNForward

    class TorchDQN(torch.nn.Module):
        def __init__(self, h, w, c, A):
            super().__init__()
            nn = torch.nn
            self.conv1, self.conv2 = nn.Conv2d(c, 32, 3, padding=1), nn.Conv2d(32, 64, 3, padding=1)
            self.conv3 = nn.Conv2d(64, 64, 3, padding=1)
            self.fc1, self.fc2, self.fc3 = nn.Linear(64 * h * w, 256), nn.Linear(256, 128), nn.Linear(128, A)

    def batch(h, w, c, seed):
        g = torch.Generator(device='cuda').manual_seed(seed)
        s = (torch.rand((BATCH, h, w, c), device='cuda', generator=g) < 0.25).to(torch.uint8)
        ns = (torch.rand((BATCH, h, w, c), device='cuda', generator=g) < 0.25).to(torch.uint8)
        a = torch.randint(0, 3, (BATCH,), device='cuda', generator=g)
        r = torch.randn(BATCH, device='cuda', generator=g)
        d = (torch.rand(BATCH, device='cuda', generator=g) < 0.1).float()
        return s, a, r, ns, d

    def medians_us(fn, inputs=(None,)):
        out = []
        for _ in range(args.repeats):
            for i in range(args.warmup):
                fn(inputs[i % len(inputs)])
            torch.cuda.synchronize()
            filler = torch.empty(1 << 28, dtype=torch.float32, device='cuda')
            for _ in range(60):
                filler.add_(1.0)
            evs = []
            for i in range(args.launches):
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

    def wall_us(fn, calls):
        """Per call, between two device synchronisations (host time included)."""
        out = []
        for _ in range(args.repeats):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) / calls * 1e6)
        return out

    def spread(v):
        return {'median_us': sorted(v)[len(v) // 2], 'repeats_us': v}

    rec = {'metric': 'dqn_actor_us', 'device': torch.cuda.get_device_name(0), 'batch': BATCH,
           'envs': ENVS, 'snakes': SNAKES, 'launches': args.launches, 'warmup': args.warmup,
           'repeats': args.repeats,
           'timing': 'one HIP event pair per call, enqueued behind ~30 ms of filler work; *_wall: wall-clock '
                     'time per call between two device synchronisations'}
    for shape in args.shapes.split(','):
        h, w, c, vr = SHAPES[shape]
        torch.manual_seed(0)
        state = TorchDQN(h, w, c, 3).cuda().state_dict()
        learner = DQNLearner(state, h, w, c, num_actions=3)
        learner16 = DQNLearner(state, h, w, c, num_actions=3, target_precision='bf16')
        batches = [batch(h, w, c, s) for s in range(4)]
        e = {'obs_shape': [h, w, c], 'parameters': learner.numel}

        # (a) the pack, (b) the refresh it replaces
        actor = learner.actor(auto_sync=False)
        e['plan'] = actor.plan
        e['pack_bytes_least'] = int(pack_bytes(actor.layout, h, w, c))
        e['pack_bound_us'] = e['pack_bytes_least'] / HBM_PEAK * 1e6
        e['pack'] = spread(medians_us(lambda _: actor.sync()))
        e['pack_over_bound'] = e['pack']['median_us'] / e['pack_bound_us']
        e['refresh_old_wall'] = spread(wall_us(lambda: DQNForward(learner.state_dict(), h, w, c), 20))
        e['pack_wall'] = spread(wall_us(actor.sync, 20))

        # (c) the update in both target precisions
        e['update_fp32'] = spread(medians_us(lambda b: learner.update(*b), batches))
        e['update_bf16_target'] = spread(medians_us(lambda b: learner16.update(*b), batches))
        e['target_forward_fp32'] = spread(medians_us(lambda b: learner.target_q(b[3]), batches))
        e['target_forward_bf16'] = spread(medians_us(lambda b: learner16.target_q(b[3]), batches))
        del learner16

        # (d) one training iteration, acting in fp32 against acting through the actor
        for name, bf16 in (('iteration_fp32_acting', False), ('iteration_actor', True)):
            kw = dict(height=20, width=20) if vr is None else dict(height=20, width=20, vision_range=vr)
            env = SnakeVecEnv(ENVS, num_snakes=SNAKES, seed=1, **kw)
            assert tuple(env.obs_shape) == (SNAKES, h, w, c), env.obs_shape
            buf = ReplayBuffer(env.obs_shape, CAPACITY)
            lrn = DQNLearner(state, h, w, c, num_actions=3)
            policy = lrn.actor() if bf16 else lrn
            collector = Collector(env, buf)
            collector.run(policy, steps=2, epsilon=0.5)

            def iteration(_=None):
                collector.run(policy, steps=1, epsilon=0.1)
                lrn.update(*buf.sample(BATCH))

            e[name] = spread(medians_us(iteration))
            e[name + '_wall'] = spread(wall_us(iteration, args.launches))
            e[name.replace('iteration', 'acting_forward')] = spread(
                medians_us(lambda _: policy(collector.obs.view(ENVS * SNAKES, h, w, c))))
            del env, buf, lrn, policy, collector
        e['iteration_actor_over_fp32'] = e['iteration_actor']['median_us'] / e['iteration_fp32_acting']['median_us']
        rec[shape] = e
        del learner, actor
        torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(json.dumps(rec, indent=1) + '\n')


if __name__ == '__main__':
    main()
