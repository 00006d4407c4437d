"""The genome-head kernel (snake_genome_actions, genome_kernels.hip) against the
restated FeedForwardNetwork (tests/genome_ref.py) on the same inputs copied to
the host. relu-only populations: outputs bitwise, actions equal. Mixed
populations: every output within the derived bound that genome_ref carries
along, the action the first maximum of the kernel's own outputs, and equal to
the reference's wherever its best output leads by more than the two bounds."""
import ctypes
import math

import numpy as np
import pytest

import genome_ref as R

pytestmark = pytest.mark.gpu

RELU_ONLY = (R.relu_activation,)


@pytest.fixture(scope='module')
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), 'needs the GPU'
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def lds_node_limit(I):
    from marlenv import _native
    lay = _native.GenomeLayout()
    cfg = _native.GenomeCfg(I, 1, 1, 0, 0, 0)
    assert _native.lib().snake_genome_plan(ctypes.byref(cfg), 64, ctypes.byref(lay)) == 0
    return lay.lds_nodes


def population(rs, N, I, A, acts):
    """Genomes of different sizes, one with no evaluated node, a hidden chain
    five deep, and one just over the LDS path's node limit; an unsorted,
    repeating env -> genome map that uses every genome and gives genome 0 about
    half of the envs (several tiles where N * S allows)."""
    limit = lds_node_limit(I)
    big = R.random_network(rs, I, A, hidden=limit + 1, acts=acts)
    assert len(big.node_evals) > limit
    nets = [R.random_network(rs, I, A, hidden=7, acts=acts), R.Network([-i - 1 for i in range(I)], range(A), []),
            R.chain_network(rs, I, A, 5, acts=acts), big]
    nets += [R.random_network(rs, I, A, hidden=h % 13, acts=acts) for h in range(min(N - 1, 9) - len(nets))]
    G = len(nets)
    g = np.concatenate([rs.permutation(G), rs.choice(G, N - G, p=[0.5] + [0.5 / (G - 1)] * (G - 1))])
    g = g[rs.permutation(N)]
    assert (np.diff(g) < 0).any() and np.bincount(g).max() > 1      # (not sorted, repeating)
    return nets, g.astype(np.int64)


def run_kernel(torch, nets, g, x, S, skip):
    from marlenv import GenomeHeads
    heads = GenomeHeads(nets, num_inputs=x.shape[-1], genome_of_env=g)
    f = torch.from_numpy(x).cuda()
    sk = None if skip is None else torch.from_numpy(skip).cuda()
    a, o = heads(f, skip=sk, return_outputs=True)
    assert a.dtype == torch.int8 and tuple(a.shape) == (len(g), S)
    assert o.dtype == torch.float64 and tuple(o.shape) == (len(g), S, len(nets[0].output_nodes))
    a2 = heads(f.view(len(g), S, -1), skip=sk)             # (without the outputs, 3-d features)
    assert torch.equal(a, a2)
    return heads, a.cpu().numpy(), o.cpu().numpy()


def compare(got_a, got_o, out, err, act, skip):
    """The assertions of the module docstring; returns how many actions were decided."""
    assert np.isfinite(out).all()
    exact = err == 0.0
    assert (bits(got_o)[exact] == bits(out)[exact]).all()
    assert (np.abs(got_o - out) <= err).all(), float((np.abs(got_o - out) - err).max())
    own = np.argmax(got_o, axis=-1).astype(np.int8)
    if skip is not None:
        own[skip != 0] = 0
    np.testing.assert_array_equal(got_a, own)
    # the reference's best output leads every other one by more than their two bounds
    best = np.take_along_axis(out, np.argmax(out, -1)[..., None], -1)
    ebest = np.take_along_axis(err, np.argmax(out, -1)[..., None], -1)
    lead = (out + err + ebest < best) | (np.arange(out.shape[-1]) == np.argmax(out, -1)[..., None])
    decided = lead.all(-1)
    if skip is not None:
        decided |= skip != 0
    np.testing.assert_array_equal(got_a[decided], act[decided])
    return int(decided.sum())


SHAPES = [(5, 3, 5, 1), (7, 4, 128, 3), (40, 2, 33, 4), (75, 4, 128, 3)]


@pytest.mark.parametrize('acts', [RELU_ONLY, R.ACTS], ids=['relu', 'mixed'])
@pytest.mark.parametrize('N,S,I,A', SHAPES)
def test_kernel_matches_restatement(torch_gpu, N, S, I, A, acts):
    rs = np.random.RandomState(1000 * N + len(acts))
    nets, g = population(rs, N, I, A, acts)
    x = R.random_features(rs, N * S, I)
    skip = (rs.rand(N, S) < 0.25).astype(np.uint8)
    heads, got_a, got_o = run_kernel(torch_gpu, nets, g, x, S, skip)
    lay, tiles, _ = heads.tiles(S)
    assert (tiles[:, 3] >= 0).any() and (tiles[:, 3] < 0).any()     # both the scratch and the LDS path ran
    if N * S > 2 * lay.tile_rows:
        assert np.bincount(tiles[:, 0]).max() > 1                   # a genome over several tiles
    out, err, act = R.reference(nets, g, x, S, skip)
    if acts is RELU_ONLY:
        assert (err == 0.0).all()
        assert (bits(got_o) == bits(out)).all()
        np.testing.assert_array_equal(got_a, act)
    decided = compare(got_a, got_o, out, err, act, skip)
    assert decided > N * S // 2
    # no skip mask: the same outputs, the plain first maximum
    _, a0, o0 = run_kernel(torch_gpu, nets, g, x, S, None)
    assert (bits(o0) == bits(got_o)).all()
    np.testing.assert_array_equal(a0, np.argmax(got_o, -1))


def test_ties_take_the_first_maximum(torch_gpu):
    """Ties at exactly 0.0 after relu, with a never-evaluated output among them."""
    ins, relu, agg = [-1, -2], R.relu_activation, R.sum_aggregation
    nets = [
        # out 0 = 0, out 1 = out 2 = relu(x0): x0 > 0 -> 1, else all 0.0 -> 0
        R.Network(ins, [0, 1, 2], [(0, relu, agg, -1.0, 1.0, []), (1, relu, agg, 0.0, 1.0, [(-1, 1.0)]),
                                   (2, relu, agg, 0.0, 1.0, [(-1, 1.0)])]),
        # out 0 = relu(-|..|) = 0.0, out 1 never evaluated (0.0), out 2 = relu(x1)
        R.Network(ins, [0, 1, 2], [(0, relu, agg, -0.5, 1.0, [(-1, 0.0)]), (2, relu, agg, 0.0, 2.0, [(-2, 1.0)])]),
    ]
    x = np.array([[1.5, 0], [-1, 0], [0, 0], [-0.0, 3],      # env 0, genome 0
                  [5, -1], [5, 0.25], [0, -0.0], [-7, 1e-30]], np.float32)
    _, got_a, got_o = run_kernel(torch_gpu, nets, [0, 1], x, 4, None)
    out, err, act = R.reference(nets, [0, 1], x, 4)
    assert (err == 0).all() and (bits(got_o) == bits(out)).all()
    np.testing.assert_array_equal(got_a, act)
    assert got_a.tolist() == [[1, 0, 0, 0], [0, 2, 0, 2]]


def test_clamps(torch_gpu):
    """Inputs that drive 5z and 2.5z far past +-60: both sides take exp and tanh
    of exactly +-60, so the outputs agree to the 4 ulp of the activation alone,
    and just inside the clamp the bound holds."""
    agg = R.sum_aggregation
    net = R.Network([-1, -2], [0, 1, 2, 3], [
        (0, R.sigmoid_activation, agg, 0.0, 1.0, [(-1, 3.0)]), (1, R.tanh_activation, agg, 0.0, 1.0, [(-1, 3.0)]),
        (2, R.sigmoid_activation, agg, 0.0, 1.0, [(-2, 1.0)]), (3, R.tanh_activation, agg, 0.0, 1.0, [(-2, 2.0)])])
    x = np.array([[100, 11.9], [-100, -11.9], [4.0001, 12], [-4.0001, -12.0001], [1e30, 0], [-1e30, 1]], np.float32)
    _, got_a, got_o = run_kernel(torch_gpu, [net], [0, 0, 0], x, 2, None)
    out, err, act = R.reference([net], [0, 0, 0], x, 2)
    compare(got_a, got_o, out, err, act, None)
    got, want = got_o.reshape(6, 4), out.reshape(6, 4)
    assert want[0, 0] == 1.0 / (1.0 + math.exp(-60.0)) and want[1, 0] == 1.0 / (1.0 + math.exp(60.0))
    assert want[0, 1] == math.tanh(60.0) == 1.0 and want[1, 1] == -1.0
    for r in (0, 1, 4, 5):
        for a in (0, 1):
            assert abs(got[r, a] - want[r, a]) <= 4 * math.ulp(want[r, a]), (r, a, got[r, a], want[r, a])


def test_from_linear(torch_gpu):
    """fc3_to_genome's head: relu(b + sum_i x_i w_i), the sum sequential in float64, bitwise."""
    from marlenv import GenomeHeads
    rs = np.random.RandomState(8)
    N, S = 9, 4
    W, b = rs.randn(3, 128).astype(np.float32), rs.randn(3).astype(np.float32)
    x = R.random_features(rs, N * S, 128)
    heads = GenomeHeads.from_linear(torch_gpu.from_numpy(W), torch_gpu.from_numpy(b), num_envs=N)
    a, o = heads(torch_gpu.from_numpy(x).cuda(), return_outputs=True)
    want = np.zeros((N * S, 3))
    for r in range(N * S):
        for k in range(3):
            s = 0.0
            for i in range(128):
                s = s + float(x[r, i]) * float(W[k, i])
            z = float(b[k]) + s
            want[r, k] = z if z > 0.0 else 0.0
    assert (bits(o.cpu().numpy().reshape(N * S, 3)) == bits(want)).all()
    np.testing.assert_array_equal(a.cpu().numpy().reshape(-1), np.argmax(want, -1))


# ---- end to end: 6 genomes x 2 envs, 2 snakes, 8x8 board, episodes of at most 25 steps

E2E = dict(N=12, S=2, I=16, steps=40, seed=21)


def e2e_env():
    from marlenv import SnakeVecEnv
    return SnakeVecEnv(E2E['N'], num_snakes=E2E['S'], height=8, width=8, snake_length=3, max_episode_steps=25,
                       seed=E2E['seed'])


def e2e_heads():
    from marlenv import GenomeHeads
    rs = np.random.RandomState(9)
    nets = [R.random_network(rs, E2E['I'], 3, hidden=h, acts=RELU_ONLY) for h in (0, 2, 4, 6, 9, 12)]
    g = [4, 0, 2, 5, 1, 3, 0, 5, 3, 4, 2, 1]
    return nets, g, GenomeHeads(nets, num_inputs=E2E['I'], genome_of_env=g)


def projection(torch, obs_shape):
    """A fixed projection with entries in -2 .. 2: sums of at most 512 bytes times
    them are small integers, exact in float32 in any order."""
    S, h, w, c = obs_shape
    P = np.random.RandomState(10).randint(-2, 3, size=(h * w * c, E2E['I'])).astype(np.float32)
    P = torch.from_numpy(P).cuda()
    return lambda obs: obs.reshape(obs.shape[0], -1).float() @ P


@pytest.fixture(scope='module')
def rollout(torch_gpu):
    """The loop of evaluate_population written out, checked step by step against
    the restatement and a host recomputation; returns the host's R."""
    torch = torch_gpu
    env = e2e_env()
    nets, g, heads = e2e_heads()
    N, S = E2E['N'], E2E['S']
    feat = projection(torch, env.obs_shape)
    obs = env.reset()
    R_dev = torch.zeros((N, S), dtype=torch.float64, device='cuda')
    fin_dev = torch.zeros(N, dtype=torch.bool, device='cuda')
    skip_dev = None
    R_host, fin, skip = np.zeros((N, S)), np.zeros(N, bool), np.zeros((N, S), bool)
    moved = set()
    for t in range(E2E['steps']):
        f = feat(obs.view(N * S, *env.obs_shape[1:]))
        fh = f.cpu().numpy()
        assert (fh == np.round(fh)).all()
        a = heads(f, skip=skip_dev)
        np.testing.assert_array_equal(a.cpu().numpy(), R.reference(nets, g, fh, S, skip)[2], err_msg='step %d' % t)
        moved |= set(a.cpu().numpy()[~skip].tolist())
        obs, rew, done, info = env.step(a)
        ended = info['episode_done']
        R_dev = torch.where(fin_dev[:, None], R_dev, R_dev + rew)
        fin_dev = fin_dev | ended
        skip_dev = (done & ~ended[:, None]) | fin_dev[:, None]
        rew_h, done_h, ended_h = rew.cpu().numpy(), done.cpu().numpy(), ended.cpu().numpy()
        for i in range(N):
            if not fin[i]:
                R_host[i] += rew_h[i]
        fin |= ended_h
        skip = (done_h & ~ended_h[:, None]) | fin[:, None]
        assert (bits(R_dev.cpu().numpy()) == bits(R_host)).all()
        np.testing.assert_array_equal(fin_dev.cpu().numpy(), fin)
        np.testing.assert_array_equal(skip_dev.cpu().numpy(), skip)
    env.close()
    assert fin.all() and len(moved) > 1
    return R_host


def test_end_to_end_rollout(rollout):
    assert np.isfinite(rollout).all() and (rollout != 0).any()


def test_evaluate_population(torch_gpu, rollout):
    from marlenv import evaluate_population
    nets, g, heads = e2e_heads()
    results = []
    for sync_every in (1, 1000, 1):
        env = e2e_env()
        results.append(evaluate_population(env, projection(torch_gpu, env.obs_shape), heads, steps=E2E['steps'],
                                           sync_every=sync_every))
        env.close()
    for Rv, fit, gfit in results:
        assert (bits(Rv) == bits(rollout)).all()
        assert [bits(v) for v in fit] == [bits(np.mean(rollout[i])) for i in range(E2E['N'])]
        for k in range(6):
            i, j = [e for e in range(E2E['N']) if g[e] == k]
            assert bits(gfit[k]) == bits(np.mean(np.array([fit[i], fit[j]])))


def test_with_the_dqn_features(torch_gpu):
    """forward_features of a random fp32 DQNForward on an 8x8 map into mixed
    genomes: finite fitnesses, and R is the sum of an env's rewards up to and
    including the step of its first episode_done."""
    torch = torch_gpu
    from marlenv import DQNForward, GenomeHeads, evaluate_population
    h = w = 8
    gen = torch.Generator().manual_seed(3)
    shapes = {'conv1.weight': (32, 8, 3, 3), 'conv1.bias': (32,), 'conv2.weight': (64, 32, 3, 3),
              'conv2.bias': (64,), 'conv3.weight': (64, 64, 3, 3), 'conv3.bias': (64,),
              'fc1.weight': (256, 64 * h * w), 'fc1.bias': (256,), 'fc2.weight': (128, 256),
              'fc2.bias': (128,), 'fc3.weight': (3, 128), 'fc3.bias': (3,)}
    state = {k: torch.randn(s, generator=gen) * 0.05 for k, s in shapes.items()}
    net = DQNForward(state, h, w, 8, num_actions=3, precision='fp32')
    rs = np.random.RandomState(11)
    nets = [R.random_network(rs, 128, 3) for _ in range(6)]
    heads = GenomeHeads(nets, genome_of_env=[0, 1, 2, 3, 4, 5, 5, 4, 3, 2, 1, 0])

    class Recording:                # the env, keeping every step's rewards and episode ends
        def __init__(self, env):
            self.env, self.rew, self.ended = env, [], []

        def __getattr__(self, k):
            return getattr(self.env, k)

        def step(self, a):
            out = self.env.step(a)
            self.rew.append(out[1].cpu().numpy())
            self.ended.append(out[3]['episode_done'].cpu().numpy())
            return out

    env = Recording(e2e_env())
    Rv, fit, gfit = evaluate_population(env, net.forward_features, heads, steps=E2E['steps'], sync_every=8)
    env.env.close()
    assert np.isfinite(fit).all() and np.isfinite(gfit).all()
    want, last = np.zeros_like(Rv), 0
    for i in range(E2E['N']):
        first = [t for t in range(len(env.ended)) if env.ended[t][i]][0]
        for t in range(first + 1):
            want[i] += env.rew[t][i]
        last = max(last, first + 1)
    assert len(env.rew) == -(-last // 8) * 8         # stopped at the first sync after the last episode's end
    assert (bits(Rv) == bits(want)).all()
