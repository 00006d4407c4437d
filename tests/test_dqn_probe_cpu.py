"""The integer probes of tests/dqn_probe.py are valid and sharp (no GPU): every
probe that tests/test_dqn_exact.py runs keeps the arithmetic of the kernels
exact, exercises every weight column and input byte, and notices a single
zeroed weight. Conditions on the probes, not on the kernels."""
import pytest

torch = pytest.importorskip('torch')

import dqn_probe as dp

# Coverage over a batch (every byte position set in one observation and clear in
# another, the share of live units) is a statement about a batch: a position is
# never 1 in B observations with probability 0.75^B, 2e-8 at B = 64, times at
# most 15 488 positions. The one smaller probe is train_dqn.py's 20x20x8 at
# B = 5; the tail batches 1..513 and 1/127/129 are prefixes of larger probes.
COVER_MIN_B = 64
BF16_KEYS = dp.bf16_probe_keys()
FP32_KEYS = dp.fp32_probe_keys()


def _ids(keys):
    return ['%dx%dx%d-a%d-s%d-b%d' % k for k in keys]


def _is_int(t):
    return bool((t == t.round()).all())


def _exact_bound(p):
    """Largest |partial sum| any summation order can meet in each layer:
    max|input| * max row sum of |W| + max|b|."""
    worst = 0.0
    for name, src in zip(dp.LAYERS + ('fc3',), dp.ROUNDED + ('h2',)):
        w = p.state[name + '.weight'].double()
        worst = max(worst, float(p.acts[src].abs().max()) * float(w.abs().reshape(w.size(0), -1).sum(1).max())
                    + float(p.state[name + '.bias'].abs().max()))
    return worst


@pytest.mark.parametrize('key', BF16_KEYS, ids=_ids(BF16_KEYS))
def test_bf16_probe_valid(key):
    p = dp.probe(*key)
    for name, t in p.state.items():
        assert _is_int(t) and float(t.abs().max()) <= 256, name
        assert torch.equal(t.to(torch.bfloat16).float(), t), name
    for name in dp.ROUNDED:
        t = p.acts[name]
        assert _is_int(t) and float(t.min()) >= 0 and float(t.max()) <= 256, (name, float(t.max()))
        assert torch.equal(t.to(torch.bfloat16).double(), t), name
    assert _is_int(p.acts['h2']) and _is_int(p.q)
    assert float(p.q.abs().max()) < 2 ** 24
    assert _exact_bound(p) < 2 ** 24
    assert int(p.obs.max()) == 1          # 0/1 bytes: no /255 anywhere


@pytest.mark.parametrize('key', FP32_KEYS, ids=_ids(FP32_KEYS))
def test_fp32_probe_valid(key):
    p = dp.probe(*key)
    for name, t in p.state.items():
        assert _is_int(t), name
    for name in dp.ROUNDED + ('h2',):
        assert _is_int(p.acts[name]), name
    assert _is_int(p.q) and float(p.q.abs().max()) < 2 ** 24
    assert _exact_bound(p) < 2 ** 24
    assert int(p.obs.max()) == 1          # the /255 branch is not taken


@pytest.mark.parametrize('key', BF16_KEYS + FP32_KEYS, ids=_ids(BF16_KEYS + FP32_KEYS))
def test_probe_coverage(key):
    h, w, c, a, seed, B = key
    p = dp.probe(*key)
    for name in dp.LAYERS:
        wt = p.state[name + '.weight']
        if wt.dim() == 4:
            wt = wt.permute(0, 2, 3, 1).reshape(wt.size(0), -1)      # columns (tap, input channel)
        assert bool((wt != 0).any(0).all()), name + ' has an all-zero column'
    if B < COVER_MIN_B:
        return
    assert bool((p.obs == 1).any(0).all()) and bool((p.obs == 0).any(0).all())
    for name in ('c1', 'c2', 'c3', 'h1', 'h2'):
        t = p.acts[name]
        if h * w == 1 and name == 'h1':
            continue        # 64 fc1 columns for 256 rows: the other 192 units are their bias
        # the share of the layer's unit activations over the batch that are
        # positive (units that fire on at least one row would be ~100 %)
        live = float((t > 0).double().mean())
        assert 0.25 <= live <= 0.90, (name, live)


def test_fp32_cases_sit_on_both_sides_of_the_dispatch():
    for h, w, c, a, B, mfma in dp.FP32_CASES:
        assert dp.fp32_conv_on_matrix_cores(h, w, c) == mfma, (h, w, c)
    assert dp.fp32_conv_on_matrix_cores(33, 33, 8) and not dp.fp32_conv_on_matrix_cores(34, 34, 8)
    sides = {(B * h * w) % 128 > 64 for h, w, c, a, B, _ in dp.FP32_CASES}
    assert sides == {True, False}


def sharpness(h, w, c, seeds, B, n=40):
    """Per layer: of n randomly chosen nonzero weights per seed, each zeroed
    alone, the share that changes the reference's features on at least one
    observation; (pooled over the seeds' nets, the lowest single net)."""
    pooled, lowest = {}, {}
    for name in dp.LAYERS:
        hit = tot = 0
        worst = 1.0
        for seed in seeds:
            p = dp.probe(h, w, c, 3, seed, B)
            g = torch.Generator().manual_seed(1000 + seed)
            wt = p.state[name + '.weight']
            nz = wt.reshape(-1).nonzero().reshape(-1)
            pick = nz[torch.randperm(nz.numel(), generator=g)[:n]]
            mine = 0
            for idx in pick.tolist():
                st = dict(p.state)
                w2 = wt.clone()
                w2.view(-1)[idx] = 0.0
                st[name + '.weight'] = w2
                # a change on the first observations is a change on the batch: try those first
                for rows in (slice(0, 12), slice(0, B)):
                    acts = {k: v[rows] for k, v in p.acts.items()}
                    feat = dp.ref64(st, None, start=name, acts=acts)[0]
                    if not torch.equal(feat, p.feat[rows]):
                        mine += 1
                        break
            hit += mine
            tot += len(pick)
            worst = min(worst, mine / len(pick))
        pooled[name], lowest[name] = hit / tot, worst
    return pooled, lowest


@pytest.mark.parametrize('geo', dp.SHARP_GEO, ids=['%dx%dx%d' % g for g in dp.SHARP_GEO])
def test_probe_sharpness(geo):
    """>= 90 % of single zeroed weights change the features, per layer. Asserted
    on the lowest single net of the case's seeds, which bounds the union over
    the seeds from below."""
    pooled, lowest = sharpness(*geo, seeds=dp.SEEDS, B=dp.GRID_B)
    print('sharpness %dx%dx%d pooled %s lowest %s' % (geo + (pooled, lowest)))
    for name in dp.LAYERS:
        assert lowest[name] >= 0.90, (name, lowest[name], pooled[name])
