"""The map path of the bf16 DQN forward on real weights and real full-map
observations, against the PyTorch restatement of the reference network
(tests/test_dqn.py's RefDQN) in fp32 and with its bf16 roundings.

The bounds are tests/test_dqn.py's, unchanged: |dq| <= 2e-2 * max|q| + 1e-3
against fp32, <= 2e-3 * max|q| + 1e-4 against the bf16 restatement, features <=
2e-2 * max + 1e-3, equal argmax where the reference's margin exceeds 5 % of the
scale. They carry over to the larger maps: measured on the CPU with the
restatement alone (random-init nets, dense and sparse 0/1 inputs; 20x20x8,
20x20x32, 22x22x8, 12x10x8, 4x33x16) the bf16 restatement differs from fp32 by
2.1e-4 to 1.1e-3 of the scale on q and at most 2.3e-3 on the features, and a
float64-accumulated bf16 restatement from the fp32-accumulated one (the order
of the sums) by at most 1.2e-4: the sizes seen at 11x11 (7.3e-4, 1.9e-3,
1.2e-4). Layout, border, tail and stale-state errors too small for these bounds
are held by tests/test_dqn_map_exact.py."""
import math

import pytest

torch = pytest.importorskip('torch')

from test_dqn import RefDQN, _obs_full

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('B,shape', [(1, (20, 20, 8)), (333, (20, 20, 8)), (1000, (20, 20, 8)),
                                     (333, (20, 20, 16)), (1000, (12, 10, 8)), (1, (12, 10, 8))])
def test_map_forward_matches_fp32_reference(B, shape):
    from marlenv.dqn import DQNForward
    torch.manual_seed(1)
    h, w, c = shape
    ref = RefDQN(h, w, c, 3).cuda()
    obs = _obs_full(B, fs=c // 8, H=h, W=w)
    assert obs.shape == (B, h, w, c)
    net = DQNForward(ref, h, w, c, 3)
    assert net.plan == 'map'
    q = net(obs)
    feat = net.forward_features(obs)
    torch.cuda.synchronize()
    with torch.no_grad():
        q32 = ref(obs)
        f32 = ref.forward_features(obs)
        qbf = ref(obs, bf16=True)
    assert q.shape == (B, 3) and feat.shape == (B, 128)
    assert torch.isfinite(q).all()
    scale = float(q32.abs().max())
    print('q vs fp32 %.3g, vs bf16 %.3g of scale %.3g' % (float((q - q32).abs().max()), float((q - qbf).abs().max()), scale))
    assert float((q - q32).abs().max()) <= 2e-2 * scale + 1e-3
    assert float((q - qbf).abs().max()) <= 2e-3 * scale + 1e-4
    fs_ = float(f32.abs().max())
    assert float((feat - f32).abs().max()) <= 2e-2 * fs_ + 1e-3
    top2 = q32.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 0.05 * scale
    assert bool((q.argmax(1)[clear] == q32.argmax(1)[clear]).all())


def test_map_large_batch_sampled():
    """81 923 observations of 20x20x8: the conv3 scratch passes 4 GiB, so every
    offset into it must be 64-bit. 256 sampled rows and the first and last two
    against the fp32 reference; every output finite."""
    from marlenv.dqn import DQNForward
    torch.manual_seed(3)
    B = 81923
    obs = _obs_full(B, seed=5)
    ref = RefDQN(20, 20, 8, 3).cuda()
    net = DQNForward(ref, 20, 20, 8, 3)
    assert net.plan == 'map' and B * net.layout.act_per_obs * 2 > 2 ** 32
    q = net(obs)
    torch.cuda.synchronize()
    g = torch.Generator(device='cuda').manual_seed(7)
    rows = torch.cat([torch.randint(0, B, (256,), generator=g, device='cuda'),
                      torch.tensor([0, 1, B - 2, B - 1], device='cuda')])
    with torch.no_grad():
        q32 = ref(obs[rows])
    scale = float(q32.abs().max())
    assert torch.isfinite(q).all()
    assert float((q[rows] - q32).abs().max()) <= 2e-2 * scale + 1e-3


def test_map_evaluate_runs_on_the_full_map():
    """One consumer: the evaluator loop on a 64-env full-map SnakeVecEnv."""
    from marlenv import SnakeVecEnv
    from marlenv.dqn import DQNForward
    from marlenv.policy import evaluate
    torch.manual_seed(5)
    env = SnakeVecEnv(64, num_snakes=4, seed=3, height=20, width=20)
    net = DQNForward(RefDQN(20, 20, 8, 3).cuda(), 20, 20, 8, 3)
    assert net.plan == 'map'
    episodes, score, life = evaluate(env, net, steps=20)
    torch.cuda.synchronize()
    assert episodes >= 0
    assert episodes == 0 or (math.isfinite(score) and math.isfinite(life))
    assert torch.isfinite(net(env.reset().view(-1, 20, 20, 8))).all()
