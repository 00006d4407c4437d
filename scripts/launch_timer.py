"""The per-launch device timer of policy_bench.py, greedy_bench.py and
genome_bench.py: one HIP event pair per launch, all enqueued behind ~30 ms of
filler work."""
import torch

_filler = []


def per_launch_us(fn, inputs, launches, warmup, before=None):
    """Median and mean device microseconds of fn(input) over `launches` launches
    walking round `inputs`; before(input), if any, runs outside the timed span."""
    before = before or (lambda x: None)
    for i in range(warmup):
        before(inputs[i % len(inputs)])
        fn(inputs[i % len(inputs)])
    torch.cuda.synchronize()
    # ~30 ms of other work first: the host enqueues every timed launch while the
    # GPU is busy, so no span between two events waits for the host
    if not _filler:
        _filler.append(torch.empty(1 << 28, dtype=torch.float32, device='cuda'))
    for _ in range(60):
        _filler[0].add_(1.0)
    evs = []
    for i in range(launches):
        x = inputs[i % len(inputs)]
        before(x)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(x)
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in evs)
    return us[len(us) // 2], sum(us) / len(us)
