"""battle() and the controllers (marlenv/arena.py) on the GPU: a DQN behind the
safe-action rule, a NEAT head on the same net's features and two greedy
opponents share every env. A hand loop calls the same controllers, checks each
step's actions against the three numpy restatements (policy_ref, genome_ref,
greedy_ref) on the env's own observations and sums the results on the host;
battle() must return those sums.

The rewards are multiples of 1/8 far below 2^50, so every float64 sum of them
is exact whatever its order: the device's and the host's sums are compared for
equality."""
import numpy as np
import pytest

import genome_ref
import greedy_ref
import policy_ref

pytestmark = pytest.mark.gpu

N, S, STEPS, SIDE = 32, 4, 60, 12
REWARDS = dict(fruit=1.0, kill=0.5, lose=-1.0, win=2.0, time=0.125)
UNKNOWN = -128


@pytest.fixture(scope='module')
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), 'needs the GPU'
    return torch


def make_env():
    from marlenv import SnakeVecEnv
    return SnakeVecEnv(N, num_snakes=S, height=SIDE, width=SIDE, snake_length=3, max_episode_steps=40, seed=31,
                       reward_dict=REWARDS)


@pytest.fixture(scope='module')
def net(torch_gpu):
    """A small random fp32 DQNForward on the 12x12 full map (weights large
    enough that its features change with the observation), and the weights of
    a random linear NEAT head on its 128 features, each weight row made
    orthogonal to the mean feature vector of the first observations so that
    the head's choice follows what changes between observations."""
    torch = torch_gpu
    from marlenv import DQNForward
    g = torch.Generator().manual_seed(3)
    shapes = {'conv1.weight': (32, 8, 3, 3), 'conv1.bias': (32,), 'conv2.weight': (64, 32, 3, 3),
              'conv2.bias': (64,), 'conv3.weight': (64, 64, 3, 3), 'conv3.bias': (64,),
              'fc1.weight': (256, 64 * SIDE * SIDE), 'fc1.bias': (256,), 'fc2.weight': (128, 256),
              'fc2.bias': (128,), 'fc3.weight': (3, 128), 'fc3.bias': (3,)}
    state = {k: torch.randn(s, generator=g) * 0.15 for k, s in shapes.items()}
    fwd = DQNForward(state, SIDE, SIDE, 8, num_actions=3, precision='fp32')
    env = make_env()
    m = fwd.forward_features(env.reset().view(N * S, SIDE, SIDE, 8)).mean(0).cpu()
    env.close()
    W = torch.randn((3, 128), generator=g)
    W = W - (W @ m)[:, None] * m[None, :] / (m @ m)
    return fwd, (W, torch.zeros(3))


def make_controllers(torch, net, env, seed=17):
    from marlenv import GenomeHeads, GreedyActions, HybridNEAT, SafeDQN
    fwd, (W, b) = net
    heads = GenomeHeads.from_linear(W, b, num_envs=N)
    greedy = GreedyActions(env.obs_shape, generator=torch.Generator(device='cuda').manual_seed(seed))
    return [SafeDQN(fwd, env.obs_shape), HybridNEAT(fwd.forward_features, heads), greedy, greedy]


@pytest.fixture(scope='module')
def hand_loop(torch_gpu, net):
    """The loop of battle() written out; returns (episodes, mean reward, mean lifetime) summed on the host."""
    torch = torch_gpu
    fwd, (W, b) = net
    env = make_env()
    dqn, neat, greedy, _ = make_controllers(torch, net, env)
    W, b = W.numpy(), b.numpy()
    head = genome_ref.Network([-i - 1 for i in range(128)], range(3), [
        (o, genome_ref.relu_activation, genome_ref.sum_aggregation, float(b[o]), 1.0,
         [(-i - 1, float(W[o, i])) for i in range(128)]) for o in range(3)])
    draws = torch.Generator(device='cuda').manual_seed(17)      # the generator of make_controllers, again
    mine = {0: np.zeros(S, bool), 1: np.zeros(S, bool), 2: np.zeros(S, bool)}
    mine[0][0] = mine[1][1] = True
    mine[2][2:] = True
    obs = env.reset()
    done = np.zeros((N, S), bool)
    dirs_safe = np.full((N, S, 2), UNKNOWN, np.int8)
    dirs_greedy = np.full((N, S, 2), UNKNOWN, np.int8)
    ep_rew, ep_life = np.zeros((N, S)), np.zeros((N, S))
    tot_rew, tot_life, episodes = np.zeros(S), np.zeros(S), 0
    moved = [set() for _ in range(S)]
    for t in range(STEPS):
        skips = {k: done | ~m for k, m in mine.items()}
        dev = {k: torch.from_numpy(v).cuda() for k, v in skips.items()}
        rnd = torch.randint(-2 ** 31, 2 ** 31, (N, S), dtype=torch.int32, device='cuda', generator=draws)
        a0 = dqn(obs, dev[0], slots=(0,))
        a1 = neat(obs, dev[1], slots=(1,))
        a2 = greedy(obs, dev[2], rnd=rnd, slots=(2, 3))
        # ---- the restatements on the same observations
        o = obs.cpu().numpy()
        q = np.zeros((N, S, 3), np.float32)
        q[:, 0] = fwd(obs[:, 0].contiguous()).cpu().numpy()
        r0, dirs_safe, _ = policy_ref.safe_actions(o, q, skips[0].astype(np.uint8), dirs_safe)
        f = fwd.forward_features(obs[:, 1].contiguous()).cpu().numpy()
        out, err, r1 = genome_ref.reference([head], [0] * N, f, 1, skips[1][:, 1:2])
        assert (err == 0).all()
        r2, dirs_greedy, _ = greedy_ref.greedy_actions(o, rnd.cpu().numpy(), skips[2].astype(np.uint8), dirs_greedy)
        np.testing.assert_array_equal(a0.cpu().numpy(), r0, err_msg='dqn, step %d' % t)
        assert (r0[:, 1:] == 0).all()
        np.testing.assert_array_equal(a1.cpu().numpy()[:, 1], r1[:, 0], err_msg='neat, step %d' % t)
        assert (a1.cpu().numpy()[:, [0, 2, 3]] == 0).all()
        np.testing.assert_array_equal(a2.cpu().numpy(), r2, err_msg='greedy, step %d' % t)
        assert (r2[:, :2] == 0).all()
        np.testing.assert_array_equal(dqn.policy.dirs.cpu().numpy(), dirs_safe)
        np.testing.assert_array_equal(greedy.dirs.cpu().numpy(), dirs_greedy)
        actions = np.where(mine[0], r0, np.where(mine[1], np.concatenate([r1] * S, 1), r2)).astype(np.int8)
        for s in range(S):
            moved[s] |= set(actions[~done[:, s], s].tolist())
        # ---- the step and the sums
        ep_life += ~done
        obs, rew, done_dev, info = env.step(torch.from_numpy(actions).cuda())
        ep_rew += rew.cpu().numpy()
        ended = info['episode_done'].cpu().numpy()
        episodes += int(ended.sum())
        tot_rew += ep_rew[ended].sum(0)
        tot_life += ep_life[ended].sum(0)
        ep_rew[ended] = 0
        ep_life[ended] = 0
        done = done_dev.cpu().numpy() & ~ended[:, None]
        for c in (dqn, greedy):
            c.forget(info['episode_done'])
        dirs_safe[ended] = UNKNOWN
        dirs_greedy[ended] = UNKNOWN
    env.close()
    assert all(len(m) > 1 for m in moved), moved        # every slot's policy does move
    assert episodes >= N                                # (an episode lasts at most 40 of the 60 steps)
    return episodes, tot_rew / episodes, tot_life / episodes


def run_battle(torch, net):
    from marlenv import battle
    env = make_env()
    res = battle(env, make_controllers(torch, net, env), STEPS)
    env.close()
    return res


def test_hand_loop_matches_the_restatements(hand_loop):
    episodes, reward, life = hand_loop
    assert np.isfinite(reward).all() and (life > 0).all() and (life <= 40).all()


def test_battle_equals_the_hand_loop(torch_gpu, net, hand_loop):
    n, reward, life = run_battle(torch_gpu, net)
    assert n == hand_loop[0]
    assert reward.dtype == np.float64 and life.dtype == np.float64 and reward.shape == life.shape == (S,)
    np.testing.assert_array_equal(reward, hand_loop[1])
    np.testing.assert_array_equal(life, hand_loop[2])
    # a second battle from the same seeds: the same numbers
    n2, reward2, life2 = run_battle(torch_gpu, net)
    assert n2 == n
    np.testing.assert_array_equal(reward2, reward)
    np.testing.assert_array_equal(life2, life)


def test_no_host_sync_per_step(torch_gpu, net):
    """battle() keeps the host out of its loop: under torch's sync debug mode a
    battle of 13 steps waits for the device exactly as often as one of 3 steps
    (the set-up and the read of the results)."""
    import warnings
    torch = torch_gpu

    def syncs(steps):
        env = make_env()
        ctrl = make_controllers(torch, net, env)
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            torch.cuda.set_sync_debug_mode('warn')
            try:
                from marlenv import battle
                battle(env, ctrl, steps)
            finally:
                torch.cuda.set_sync_debug_mode('default')
        env.close()
        return sum('synchroniz' in str(w.message).lower() for w in seen)

    def upload_reported():
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            torch.cuda.set_sync_debug_mode('warn')
            try:
                torch.as_tensor([1, 2], dtype=torch.int64, device='cuda')
            finally:
                torch.cuda.set_sync_debug_mode('default')
        return any('synchroniz' in str(w.message).lower() for w in seen)

    assert upload_reported()        # (the mode sees a host list uploaded to the device)
    few, many = syncs(3), syncs(13)
    print('synchronizing calls:', few, many)
    assert few > 0          # (the results are read at the end)
    assert many == few


def test_controller_list_of_the_wrong_length(torch_gpu, net):
    from marlenv import battle
    env = make_env()
    with pytest.raises(ValueError):
        battle(env, make_controllers(torch_gpu, net, env)[:3], 1)
    env.close()


def test_shared_and_plain_controllers(torch_gpu):
    """One greedy object in all four slots is called once per step, and a plain
    callable (here: always turn, on its own slot) fits the protocol."""
    torch = torch_gpu
    from marlenv import GreedyActions, battle
    env = make_env()
    calls = []

    class Counting(GreedyActions):
        def __call__(self, obs, skip=None, **kw):
            calls.append(kw.get('slots'))
            return super().__call__(obs, skip, **kw)

    def turner(obs, skip, slots):
        calls.append(slots)
        return torch.where(skip, 0, 1).to(torch.int8)

    g = Counting(env.obs_shape, generator=torch.Generator(device='cuda').manual_seed(1))
    n, reward, life = battle(env, [g, turner, g, g], 10)
    env.close()
    assert calls == [(0, 2, 3), (1,)] * 10
    assert n == 0 or np.isfinite(reward).all()
