"""Device time of one DQNLearner.update (dqn_train_kernels.hip + the fp32
forward) beside the same update in PyTorch eager fp32.

Shapes: B = 512 at 20x20x8 (train_dqn.py's Config) and at 11x11x8 (vision range
5). The yardstick runs in the same process on the same tensors: a torch
restatement of the network (train_dqn.py:104-151), smooth_l1_loss, backward,
clip_grad_norm_(10) and optim.Adam -- Trainer.update_model (:243-257) without
its .item(). Each call is timed by its own pair of HIP events, all enqueued
behind ~30 ms of filler work so that the GPU never waits for the host inside a
timed span; 100 calls, three repeats, each repeat's median kept. The learner's
stages (target forward, policy forward, TD loss, backward, clip + Adam) are
timed the same way one by one.

Per-kernel times come from a kernel trace taken in a run of its own:

    rocprofv3 --kernel-trace -f csv -d DIR -o trace -- python scripts/learner_bench.py --trace-loop 30
    python scripts/learner_bench.py --fold-trace DIR/trace_kernel_trace.csv --updates 30 --record REC.json

--fold-trace needs no GPU: it labels every dispatch of an update by its kernel
name and its ordinal among that name's dispatches in the update (the backward
launches its GEMMs in a fixed order: fc2, fc1, conv3, conv2, conv1), takes the
median duration per label and adds, for the GEMMs, the algorithmic FLOPs and
their fraction of the 157.3 TF fp32 matrix peak.

--backward-precision bf16 builds the learner with backward_precision='bf16'
(also for --trace-loop; --fold-trace knows the bf16 kernels' names and adds
their fraction of the 2.5 PF bf16 peak). --backward-precision both times
backward and update of an fp32-mode and a bf16-mode learner in one process on
the same batches, by the same method, and writes the record to
profiles/learner_bf16_bench.json (or --out).

--forward-precision bf16 builds the learner with forward_precision='bf16' and
target_precision='mixed' (also for --trace-loop; --fold-trace labels the
k_fwd16 dispatches of an update by layer, target forward first, and adds their
FLOPs). --forward-precision both times the policy forward, the target forward
(fp32 against 'mixed') and update of an fp32-forward and a bf16-forward learner
in one process on the same batches, by the same method, with
--backward-precision fp32 or bf16 for both, and writes the record to
profiles/learner_fwd16_bench.json (or --out).
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'marl-snake_amd'))

FP32_MATRIX_PEAK = 157.3e12
BF16_MATRIX_PEAK = 2.5e15
BF16_RECORD = os.path.join(ROOT, 'profiles', 'learner_bf16_bench.json')
FWD16_RECORD = os.path.join(ROOT, 'profiles', 'learner_fwd16_bench.json')
SHAPES = {'config_20x20x8': (20, 20, 8), 'vision5_11x11x8': (11, 11, 8)}
BATCH = 512


def gemm_flops(h, w, c, A=3, B=BATCH):
    """Algorithmic FLOPs (2 per multiply-add) of the backward's GEMMs, by label."""
    P = h * w
    M = B * P
    return {
        'wgrad fc2': 2 * B * 128 * 256, 'dgrad fc2': 2 * B * 128 * 256,
        'wgrad fc1': 2 * B * 256 * 64 * P, 'dgrad fc1': 2 * B * 256 * 64 * P,
        'wgrad conv3': 2 * M * 64 * 576, 'dgrad conv3': 2 * M * 64 * 576,
        'wgrad conv2': 2 * M * 64 * 288, 'dgrad conv2': 2 * M * 32 * 576,
        'wgrad conv1': 2 * M * 32 * 9 * c,
    }


def forward_gemm_flops(h, w, c, B=BATCH):
    """Algorithmic FLOPs of one forward's five matrix-core GEMMs, by layer."""
    M = B * h * w
    return {'conv1': 2 * M * 32 * 9 * c, 'conv2': 2 * M * 64 * 288, 'conv3': 2 * M * 64 * 576,
            'fc1': 2 * B * 256 * 64 * h * w, 'fc2': 2 * B * 128 * 256}


def update_bytes(h, w, c, A=3, B=BATCH):
    """Least bytes one update moves: both observation batches, the policy
    forward's pre-activations written and read back, the dY buffers written and
    read, the weights read three times (two forwards, the input gradients) and
    parameters, gradients, m and v read and written by clip + Adam."""
    P = h * w
    n = 32 * 9 * c + 64 * 288 + 64 * 576 + 256 * 64 * P + 128 * 256 + A * 128 + 32 + 64 + 64 + 256 + 128 + A
    acts = B * (P * (32 + 64 + 64) + 256 + 128)
    return 2 * B * P * c + 4 * (2 * acts + acts + 2 * acts) + 4 * n * (3 + 1 + 2 + 1 + 6)


def fold_trace(path, updates, shape):
    h, w, c = SHAPES[shape]
    rows = []
    with open(path) as fp:
        for r in csv.DictReader(fp):
            rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']))
    rows.sort()
    by_name = {}
    for s, e, name in rows:
        by_name.setdefault(name, []).append(e - s)
    order = {'k_wgrad': ('fc2', 'fc1', 'conv3', 'conv2', 'conv1'), 'k_dgrad': ('fc2', 'fc1', 'conv3', 'conv2')}
    # k_wgrad<2> (dense) runs fc2, fc1; <1> conv3, conv2; <0> conv1 -- the template argument is in the name
    out, flops = {}, gemm_flops(h, w, c)
    for name, durs in sorted(by_name.items()):
        if len(durs) % updates:
            continue                          # not a kernel of the update loop (set-up work)
        per = len(durs) // updates
        short = name.split('(')[0].split('::')[-1]
        for j in range(per):
            d = sorted(durs[j::per])
            label = '%s #%d' % (short, j) if per > 1 else short
            out[label] = {'median_us': d[len(d) // 2] / 1e3, 'calls_per_update': 1}
    # the GEMMs: label -> layer by template argument and ordinal
    gemms = {}
    for label, e in out.items():
        base = label.split(' #')[0]
        is16 = base.startswith('k_wgrad16') or base.startswith('k_dgrad16')
        base = base.replace('k_wgrad16', 'k_wgrad').replace('k_dgrad16', 'k_dgrad')
        j = int(label.split('#')[1]) if '#' in label else 0
        layer = None
        if base.startswith('k_wgrad<2>') or base.startswith('k_wgrad<(int)2>'):
            layer = 'wgrad ' + ('fc2', 'fc1')[j]
        elif base.startswith('k_wgrad<1>') or base.startswith('k_wgrad<(int)1>'):
            layer = 'wgrad ' + ('conv3', 'conv2')[j]
        elif base.startswith('k_wgrad<0>') or base.startswith('k_wgrad<(int)0>'):
            layer = 'wgrad conv1'
        elif base.startswith('k_dgrad<false>') or base.startswith('k_dgrad<(bool)0>'):
            layer = 'dgrad ' + ('fc2', 'fc1')[j]
        elif base.startswith('k_dgrad<true>') or base.startswith('k_dgrad<(bool)1>'):
            layer = 'dgrad ' + ('conv3', 'conv2')[j]
        if layer:
            f = flops[layer]
            gemms[layer] = {'median_us': e['median_us'], 'flops': f,
                            'frac_of_fp32_matrix_peak': f / (e['median_us'] * 1e-6) / FP32_MATRIX_PEAK}
            if is16:
                gemms[layer]['frac_of_bf16_matrix_peak'] = f / (e['median_us'] * 1e-6) / BF16_MATRIX_PEAK
    # the bf16 forward's GEMMs: k_fwd16<0> conv1, <1> conv2, conv3, <2> fc1, fc2; with a 'mixed' target an
    # update runs them twice, the target forward first
    fwd, fflops = {}, forward_gemm_flops(h, w, c)
    for label, e in out.items():
        base = label.split(' #')[0]
        j = int(label.split('#')[1]) if '#' in label else 0
        for arg, layers in (('0', ('conv1',)), ('1', ('conv2', 'conv3')), ('2', ('fc1', 'fc2'))):
            if base.startswith('k_fwd16<%s>' % arg) or base.startswith('k_fwd16<(int)%s>' % arg):
                per = sum(1 for x in out if x.split(' #')[0] == base)
                who = ('target', 'policy')[j // len(layers)] if per == 2 * len(layers) else 'policy'
                f = fflops[layers[j % len(layers)]]
                fwd['%s %s' % (who, layers[j % len(layers)])] = {
                    'median_us': e['median_us'], 'flops': f, 'tflops': f / (e['median_us'] * 1e-6) / 1e12,
                    'frac_of_bf16_matrix_peak': f / (e['median_us'] * 1e-6) / BF16_MATRIX_PEAK}
    return {'shape': shape, 'updates_traced': updates, 'kernels_us': out, 'backward_gemms': gemms,
            'forward_gemms': fwd, 'order_in_backward': order}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--shapes', default=','.join(SHAPES))
    ap.add_argument('--out', default=None, help='also write the record to this file')
    ap.add_argument('--trace-loop', type=int, default=0, help='only run this many updates at --trace-shape')
    ap.add_argument('--trace-shape', default='config_20x20x8')
    ap.add_argument('--fold-trace', default=None, help='a rocprofv3 kernel trace CSV of a --trace-loop run')
    ap.add_argument('--updates', type=int, default=30, help='--fold-trace: the updates the trace holds')
    ap.add_argument('--record', default=None, help='--fold-trace: the JSON record to add the kernels to')
    ap.add_argument('--backward-precision', default='fp32', choices=('fp32', 'bf16', 'both'),
                    help="the learner's backward_precision; both: backward and update in each mode, side by side")
    ap.add_argument('--forward-precision', default='fp32', choices=('fp32', 'bf16', 'both'),
                    help="the learner's forward_precision (bf16: with target_precision='mixed'); both: the two "
                         'forwards and update in each mode, side by side')
    args = ap.parse_args()
    if args.fold_trace:
        rec = fold_trace(args.fold_trace, args.updates, args.trace_shape)
        if args.record:
            with open(args.record) as fp:
                whole = json.load(fp)
            if whole.get('metric') in ('dqn_backward_bf16_us', 'dqn_forward_bf16_us'):  # one trace per shape, of the bf16 mode
                whole.setdefault('kernel_traces', {})[args.trace_shape] = rec
            else:
                whole['kernel_trace'] = rec
            with open(args.record, 'w') as fp:
                fp.write(json.dumps(whole, indent=1) + '\n')
        print(json.dumps(rec))
        return

    import torch
    F = torch.nn.functional
    if not torch.cuda.is_available():
        sys.exit('learner_bench.py needs the GPU: a CPU run cannot give a time')
    from marlenv import DQNLearner

    class TorchDQN(torch.nn.Module):
        def __init__(self, h, w, c, A):
            super().__init__()
            nn = torch.nn
            self.conv1, self.conv2 = nn.Conv2d(c, 32, 3, padding=1), nn.Conv2d(32, 64, 3, padding=1)
            self.conv3 = nn.Conv2d(64, 64, 3, padding=1)
            self.fc1, self.fc2, self.fc3 = nn.Linear(64 * h * w, 256), nn.Linear(256, 128), nn.Linear(128, A)

        def forward(self, obs):
            x = obs.permute(0, 3, 1, 2).float()
            x = F.relu(self.conv1(x))
            x = F.relu(self.conv2(x))
            x = F.relu(self.conv3(x))
            x = F.relu(self.fc1(x.reshape(x.size(0), -1)))
            return self.fc3(F.relu(self.fc2(x)))

    def batch(h, w, c, seed):
        g = torch.Generator(device='cuda').manual_seed(seed)
        s = (torch.rand((BATCH, h, w, c), device='cuda', generator=g) < 0.25).to(torch.uint8)
        ns = (torch.rand((BATCH, h, w, c), device='cuda', generator=g) < 0.25).to(torch.uint8)
        a = torch.randint(0, 3, (BATCH,), device='cuda', generator=g)
        r = torch.randn(BATCH, device='cuda', generator=g)
        d = (torch.rand(BATCH, device='cuda', generator=g) < 0.1).float()
        return s, a, r, ns, d

    def medians_us(fn, inputs):
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

    def spread(v):
        return {'median_us': sorted(v)[len(v) // 2], 'repeats_us': v}

    def setup(shape, precision=None, forward=None):
        forward = forward or args.forward_precision
        h, w, c = SHAPES[shape]
        torch.manual_seed(0)
        policy, target = TorchDQN(h, w, c, 3).cuda(), TorchDQN(h, w, c, 3).cuda()
        target.load_state_dict(policy.state_dict())
        learner = DQNLearner(policy.state_dict(), h, w, c, num_actions=3,
                             backward_precision=precision or args.backward_precision, forward_precision=forward,
                             target_precision='mixed' if forward == 'bf16' else 'fp32')
        return h, w, c, policy, target, learner, [batch(h, w, c, s) for s in range(4)]

    if args.forward_precision == 'both' and args.backward_precision == 'both':
        sys.exit('--forward-precision both compares the forwards under one --backward-precision: fp32 or bf16')
    if args.trace_loop:
        if 'both' in (args.backward_precision, args.forward_precision):
            sys.exit('--trace-loop traces one mode: --backward-precision and --forward-precision fp32 or bf16')
        h, w, c, _, _, learner, batches = setup(args.trace_shape)
        for i in range(args.trace_loop):
            learner.update(*batches[i % len(batches)])
        torch.cuda.synchronize()
        return

    if args.forward_precision == 'both':
        rec = {'metric': 'dqn_forward_bf16_us', 'device': torch.cuda.get_device_name(0), 'batch': BATCH,
               'launches': args.launches, 'warmup': args.warmup, 'repeats': args.repeats,
               'backward_precision': args.backward_precision,
               'timing': 'one HIP event pair per call, enqueued behind ~30 ms of filler work',
               'yardstick': "the fp32-forward learner (forward_precision='fp32', target_precision='fp32') timed in "
                            "the same process on the same batches; the bf16 one has target_precision='mixed'"}
        for shape in args.shapes.split(','):
            e = {}
            for mode in ('fp32', 'bf16'):
                h, w, c, _, _, learner, batches = setup(shape, forward=mode)
                e[mode] = {'policy_forward': spread(medians_us(lambda b: learner(b[0]), batches)),
                           'target_forward': spread(medians_us(lambda b: learner.target_q(b[3]), batches)),
                           'update': spread(medians_us(lambda b: learner.update(*b), batches))}
                del learner
            e['obs_shape'] = [h, w, c]
            e['forward_gemm_flops'] = sum(forward_gemm_flops(h, w, c).values())
            for stage in ('policy_forward', 'target_forward', 'update'):
                e['%s_bf16_over_fp32' % stage] = e['bf16'][stage]['median_us'] / e['fp32'][stage]['median_us']
            rec[shape] = e
        print(json.dumps(rec), flush=True)
        out = args.out or FWD16_RECORD
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, 'w') as fp:
            fp.write(json.dumps(rec, indent=1) + '\n')
        return

    if args.backward_precision == 'both':
        rec = {'metric': 'dqn_backward_bf16_us', 'device': torch.cuda.get_device_name(0), 'batch': BATCH,
               'launches': args.launches, 'warmup': args.warmup, 'repeats': args.repeats,
               'timing': 'one HIP event pair per call, enqueued behind ~30 ms of filler work',
               'yardstick': "the fp32-mode learner (backward_precision='fp32') timed in the same process on the "
                            'same batches'}
        for shape in args.shapes.split(','):
            e = {}
            for mode in ('fp32', 'bf16'):
                h, w, c, _, _, learner, batches = setup(shape, mode)
                s, a, r, ns, d = batches[0]
                m = {'update': spread(medians_us(lambda b: learner.update(*b), batches))}
                nq, q = learner.target_q(ns), learner(s)
                loss, dq = learner.td_loss(q, a, r, d, nq)
                m['backward'] = spread(medians_us(lambda b: learner.backward(s, dq), batches))
                e[mode] = m
                del learner
            e['obs_shape'] = [h, w, c]
            e['backward_gemm_flops'] = sum(gemm_flops(h, w, c).values())
            for stage in ('backward', 'update'):
                e['%s_bf16_over_fp32' % stage] = e['bf16'][stage]['median_us'] / e['fp32'][stage]['median_us']
            rec[shape] = e
        print(json.dumps(rec), flush=True)
        out = args.out or BF16_RECORD
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, 'w') as fp:
            fp.write(json.dumps(rec, indent=1) + '\n')
        return

    rec = {'metric': 'dqn_update_us', 'device': torch.cuda.get_device_name(0), 'batch': BATCH,
           'launches': args.launches, 'warmup': args.warmup, 'repeats': args.repeats,
           'timing': 'one HIP event pair per call, enqueued behind ~30 ms of filler work',
           'yardstick': 'PyTorch eager fp32 on the same tensors: nn.Module forward x2, smooth_l1_loss, backward, '
                        'clip_grad_norm_(10), optim.Adam(lr=5e-4).step()'}
    for shape in args.shapes.split(','):
        h, w, c, policy, target, learner, batches = setup(shape)
        opt = torch.optim.Adam(policy.parameters(), lr=5e-4)

        def torch_update(b):
            s, a, r, ns, d = b
            q = policy(s).gather(1, a[:, None])
            with torch.no_grad():
                tq = r + (1 - d) * 0.99 * target(ns).max(1)[0]
            loss = F.smooth_l1_loss(q.squeeze(), tq)
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(policy.parameters(), 10)
            opt.step()
            return loss

        e = {'obs_shape': [h, w, c], 'parameters': learner.numel,
             'backward_gemm_flops': sum(gemm_flops(h, w, c).values()), 'update_bytes_least': update_bytes(h, w, c)}
        e['update_hip'] = spread(medians_us(lambda b: learner.update(*b), batches))
        e['update_torch'] = spread(medians_us(torch_update, batches))
        e['hip_over_torch'] = e['update_hip']['median_us'] / e['update_torch']['median_us']
        # the stages, one by one (backward and apply reuse what the earlier stages left)
        e['target_forward'] = spread(medians_us(lambda b: learner.target_q(b[3]), batches))
        e['policy_forward'] = spread(medians_us(lambda b: learner(b[0]), batches))
        s, a, r, ns, d = batches[0]
        nq, q = learner.target_q(ns), learner(s)
        loss, dq = learner.td_loss(q, a, r, d, nq)
        e['td_loss'] = spread(medians_us(lambda b: learner.td_loss(q, a, r, d, nq), batches))
        e['backward'] = spread(medians_us(lambda b: learner.backward(s, dq), batches))
        e['clip_adam'] = spread(medians_us(lambda b: learner.apply(), batches))
        e['backward_gemm_frac_of_fp32_matrix_peak'] = (
            e['backward_gemm_flops'] / (e['backward']['median_us'] * 1e-6) / FP32_MATRIX_PEAK)
        # torch's phases the same way
        e['torch_forward_x2'] = spread(medians_us(lambda b: (policy(b[0]), target(b[3])), batches))
        rec[shape] = e
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(json.dumps(rec, indent=1) + '\n')


if __name__ == '__main__':
    main()
