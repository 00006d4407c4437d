"""Device time of the replay buffer's kernels (snake_replay_push and
snake_replay_gather, replay_kernels.hip) beside the same work in torch ops.

Per geometry -- cfg2: 4 096 envs x 4 snakes x 20x20x8 (full map), cfg3: 65 536
envs x 4 x 11x11x8 (vision_range 5) -- the env is stepped with random actions,
and K consecutive steps' tensors (observations before and after, actions,
rewards, dones, the "already done" masks, the episode steps) are kept, K chosen
so that the observations exceed twice the 256 MiB Infinity Cache: the timed
pushes walk round them, so every push reads its observations from HBM as a step
of a real loop does. The rings hold 1 048 576 transitions. Each call is timed by
its own pair of HIP events, all enqueued behind ~30 ms of filler work so that
the GPU never waits for the host inside a timed span; every timing is repeated
and the record keeps each repeat's median.

Yardsticks, timed the same way in the same process on the same tensors:
  read pass     one plain read of obs and next_obs: .view(int64).sum() of each;
  torch push    the same push in sync-free torch ops on an unpacked uint8 ring:
                cumsum of the stored flags, slots from a device counter, and a
                masked scatter (index_copy_, the skipped snakes into a spare row);
  torch gather  index_select on that unpacked ring plus the small tensors; for
                the float32 format followed by the learner's
                permute(0, 3, 1, 2).float().
The gathers (B = 512 and B = 32 768, both formats) draw fresh random indices per
call over rings filled by the pushes.

Prints one JSON record: per geometry and measurement the medians in
microseconds, the algorithmic bytes, the bytes/s as a fraction of the 8 TB/s the
project's rooflines use, and HIP / torch for the push and for each gather.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'marl-snake_amd'))

import torch  # noqa: E402

HBM_PEAK = 8.0e12
L3_BYTES = 256 << 20
CAPACITY = 1 << 20
EARLY_DEATH = (10, -1.0)
GEOMETRIES = {
    'cfg2': dict(num_envs=4096, num_snakes=4, height=20, width=20, snake_length=5, vision_range=None),
    'cfg3': dict(num_envs=65536, num_snakes=4, height=20, width=20, snake_length=3, vision_range=5),
}


def medians_us(fn, inputs, launches, warmup, repeats):
    """The median device microseconds of fn(input) over `launches` calls walking
    round `inputs`, `repeats` times."""
    out = []
    for _ in range(repeats):
        for i in range(warmup):
            fn(inputs[i % len(inputs)])
        torch.cuda.synchronize()
        # ~30 ms of other work first: the host enqueues every timed call while the
        # GPU is busy, so no span between two events waits for the host
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


class TorchReplay:
    """The push and the gather in sync-free torch ops, on unpacked uint8 rings
    (row `capacity` is the spare row the skipped snakes are scattered into)."""

    def __init__(self, obs_shape, capacity, early_death, device):
        S, h, w, c = obs_shape
        self.capacity, self.row = capacity, h * w * c
        self.shape = (h, w, c)
        self.steps, self.penalty = early_death
        self.state = torch.zeros((capacity + 1, self.row), dtype=torch.uint8, device=device)
        self.next_state = torch.zeros_like(self.state)
        self.action = torch.zeros(capacity + 1, dtype=torch.int8, device=device)
        self.reward = torch.zeros(capacity + 1, dtype=torch.float32, device=device)
        self.done = torch.zeros(capacity + 1, dtype=torch.uint8, device=device)
        self.count = torch.zeros(1, dtype=torch.int64, device=device)

    def push(self, obs, next_obs, actions, rewards, done, skip, step):
        stored = ~skip.reshape(-1)
        seq = torch.cumsum(stored, 0)
        slot = torch.where(stored, (self.count + seq - 1) % self.capacity, self.capacity)
        r = rewards + torch.where(done & (step < self.steps)[:, None], self.penalty, 0.0)
        self.state.index_copy_(0, slot, obs.view(-1, self.row))
        self.next_state.index_copy_(0, slot, next_obs.view(-1, self.row))
        self.action.index_copy_(0, slot, actions.reshape(-1))
        self.reward.index_copy_(0, slot, r.reshape(-1).float())
        self.done.index_copy_(0, slot, done.reshape(-1).to(torch.uint8))
        self.count += seq[-1]

    def gather(self, idx, format):
        head = torch.where(self.count > self.capacity, self.count % self.capacity, 0)
        slot = (head + idx) % self.capacity
        state = self.state.index_select(0, slot).view((-1,) + self.shape)
        next_state = self.next_state.index_select(0, slot).view((-1,) + self.shape)
        if format == 'float32':
            state = state.permute(0, 3, 1, 2).float()
            next_state = next_state.permute(0, 3, 1, 2).float()
        return (state, self.action.index_select(0, slot).long(), self.reward.index_select(0, slot), next_state,
                self.done.index_select(0, slot).float())


def spread(v):
    return {'median_us': sorted(v)[len(v) // 2], 'repeats_us': v}


def measure(name, launches, warmup, settle, repeats):
    from marlenv import ReplayBuffer, SnakeVecEnv
    kw = dict(GEOMETRIES[name])
    N = kw.pop('num_envs')
    env = SnakeVecEnv(N, seed=0, **kw)
    S, h, w, c = env.obs_shape
    g = torch.Generator(device='cuda').manual_seed(0)
    obs = env.reset()
    obs_bytes = obs.numel()
    K = max(3, -(-2 * L3_BYTES // obs_bytes))      # (K + 1 observation tensors: a step's next_obs is the next one's obs)
    mask = torch.zeros((N, S), dtype=torch.bool, device='cuda')
    counter = torch.zeros(N, dtype=torch.int32, device='cuda')
    inputs = []
    for t in range(settle + K):
        actions = torch.randint(0, 3, (N, S), device='cuda', generator=g).masked_fill(mask, 0).to(torch.int8)
        next_obs, rewards, done, info = env.step(actions)
        ended = info['episode_done']
        if t >= settle:
            inputs.append(dict(obs=obs, next_obs=next_obs, actions=actions, rewards=rewards, done=done, skip=mask,
                               step=counter))
        obs, mask = next_obs, done & ~ended[:, None]
        counter = torch.where(ended, torch.zeros_like(counter), counter + 1)
    env.close()
    stored = float(torch.stack([(~x['skip']).sum() for x in inputs]).float().mean())

    buf = ReplayBuffer((S, h, w, c), CAPACITY, early_death=EARLY_DEATH)
    ref = TorchReplay((S, h, w, c), CAPACITY, EARLY_DEATH, 'cuda')
    P, pitch = buf.layout.packed_row, buf.layout.pitch
    rec = {'num_envs': N, 'obs_shape': [S, h, w, c], 'obs_bytes': obs_bytes, 'inputs_in_rotation': K,
           'capacity': CAPACITY, 'packed_row_bytes': P, 'ring_pitch_bytes': pitch,
           'stored_per_push_mean': stored, 'skipped_snakes_frac': 1 - stored / (N * S)}

    def entry(v, nbytes):
        e = spread(v)
        e['bytes'] = nbytes
        e['frac_of_8TBs'] = nbytes / (e['median_us'] * 1e-6) / HBM_PEAK
        return e

    # ---- push: the stored rows read once (8 bytes per cell) and written packed
    small = N * S * (1 + 8 + 1 + 1) + N * 4 + stored * (1 + 4 + 1)
    push_bytes = 2 * stored * (P * 8 + P) + small
    torch_push_bytes = 2 * N * S * (P * 8) * 2 + small       # index_copy_ reads and writes every row
    rec['push_hip'] = entry(medians_us(lambda x: buf.push(**x), inputs, launches, warmup, repeats), push_bytes)
    rec['push_torch'] = entry(medians_us(lambda x: ref.push(**x), inputs, launches, warmup, repeats), torch_push_bytes)
    rec['read_pass'] = entry(medians_us(lambda x: (x['obs'].view(torch.int64).sum(), x['next_obs'].view(torch.int64).sum()),
                                        inputs, launches, warmup, repeats), 2 * obs_bytes)
    rec['push_hip_over_torch'] = rec['push_hip']['median_us'] / rec['push_torch']['median_us']
    rec['push_hip_over_read_pass'] = rec['push_hip']['median_us'] / rec['read_pass']['median_us']
    rec['transitions_pushed'] = int(buf.count.item())

    # ---- gather: fresh indices per call over the full rings
    for B in (512, 32768):
        idxs = [torch.randint(0, CAPACITY, (B,), device='cuda', generator=g) for _ in range(8)]
        for fmt, out_bytes in (('uint8', 8 * P), ('float32', 32 * P)):
            small = B * (8 + 8 + 4 + 4 + 1 + 4 + 1)
            key = 'gather_%d_%s' % (B, fmt)
            hip = medians_us(lambda i: buf.sample(idx=i, format=fmt), idxs, launches, warmup, repeats)
            tor = medians_us(lambda i: ref.gather(i, fmt), idxs, launches, warmup, repeats)
            rec[key + '_hip'] = entry(hip, 2 * B * (out_bytes + P) + small)
            # index_select reads and writes unpacked rows; the float32 format then reads them and writes floats
            rec[key + '_torch'] = entry(tor, 2 * B * (16 * P + (40 * P if fmt == 'float32' else 0)) + small)
            rec[key + '_hip_over_torch'] = rec[key + '_hip']['median_us'] / rec[key + '_torch']['median_us']
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--settle', type=int, default=30, help='env steps before the kept inputs')
    ap.add_argument('--geometries', default='cfg2,cfg3')
    ap.add_argument('--out', default=None, help='also write the record to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('replay_bench.py needs the GPU: a CPU run cannot give a time')
    rec = {'metric': 'replay_push_gather_us', 'device': torch.cuda.get_device_name(0),
           'launches': args.launches, 'warmup': args.warmup, 'repeats': args.repeats,
           'timing': 'one HIP event pair per call; pushed inputs rotate over more than twice the Infinity Cache',
           'read_pass': 'obs.view(torch.int64).sum() and next_obs.view(torch.int64).sum()',
           'push_torch': 'cumsum of the stored flags, index_copy_ into unpacked uint8 rings',
           'gather_torch': 'index_select on the unpacked rings (+ permute(0,3,1,2).float() for float32)'}
    for name in args.geometries.split(','):
        rec[name] = measure(name, args.launches, args.warmup, args.settle, args.repeats)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(json.dumps(rec, indent=1) + '\n')


if __name__ == '__main__':
    main()
