"""The device rule on the GPU. On one: an unindexed 'cuda' is resolved when the
object is built. On two: the DQN entry points launch on their stream's device
whatever device the calling thread has current, and a training chain bound to
the second device computes what it computes on the first.

Device 0 always runs first, so that whatever the library keeps per process is
filled for device 0 before device 1 asks for it."""
import ctypes

import pytest

torch = pytest.importorskip('torch')

from dqn_probe import probe_net, probe_obs  # noqa: E402

pytestmark = pytest.mark.gpu

B = 3
# (h, w, the plan 'auto' takes): the window plan, and the smallest square map
# whose convolution workgroup asks for more than 64 KB of LDS (12 * 5888 + 2 * P16)
GEOMETRIES = ((5, 5, 'window'), (17, 17, 'map'))


@pytest.fixture
def two_devices():
    if not torch.cuda.is_available() or torch.cuda.device_count() < 2:
        pytest.skip('needs two GPUs')
    torch.cuda.set_device(0)
    yield
    torch.cuda.set_device(0)


def test_unindexed_cuda_is_resolved_at_construction():
    """DQNForward(device='cuda') holds the device that was current when it was
    built, with its index, as DQNLearner and SnakeVecEnv do; a later change of
    the current device does not move it."""
    from marlenv import DQNForward, DQNLearner, SnakeVecEnv
    state = probe_net(5, 5, 8, 3, 0)
    last = torch.cuda.device_count() - 1            # (0 on a machine with one GPU)
    with torch.cuda.device(last):
        made = [DQNForward(state, 5, 5, 8, device='cuda'), DQNForward(state, 5, 5, 8, device='cuda', precision='fp32'),
                DQNForward.empty(5, 5, 8, device='cuda'), DQNForward(state, 5, 5, 8),
                DQNLearner(state, 5, 5, 8, device='cuda'), SnakeVecEnv(4, num_snakes=2, device='cuda')]
    torch.cuda.set_device(0)
    for obj in made:
        assert obj.device == torch.device('cuda', last) and obj.device.index == last, type(obj).__name__
    obs = probe_obs(B, 5, 5, 8, 0)
    assert made[0](obs).device == torch.device('cuda', last)


@pytest.mark.parametrize('h,w,plan', GEOMETRIES, ids=[g[2] for g in GEOMETRIES])
def test_dqn_entry_points_follow_the_stream(two_devices, h, w, plan):
    """snake_dqn_pack32 and the bf16 forward of either plan, called straight
    through the binding with device 0 current and no device block around them:
    buffers on cuda:1 and a stream of cuda:1 of its own (the default stream's
    handle is 0, which means the current device). Packed weights and Q-values
    equal device 0's bit for bit."""
    from marlenv import DQNForward
    from marlenv._device import ptr
    from marlenv._native import check
    from marlenv.dqn_weights import Net32
    state, obs = probe_net(h, w, 8, 3, 0), probe_obs(B, h, w, 8, 0)
    fwd0 = DQNForward(state, h, w, 8, 3, device='cuda:0')
    assert fwd0.plan == plan and (plan == 'window' or fwd0.layout.lds_conv > 64 * 1024)
    q0 = fwd0(obs.to('cuda:0')).cpu()

    dev1 = torch.device('cuda', 1)
    fwd1 = DQNForward.empty(h, w, 8, 3, device=dev1)            # torch allocations only: nothing launched yet
    master = Net32(h * w, 8, 3, dev1).load(state)
    obs1 = obs.to(dev1)
    scratch = torch.empty(2 * B * fwd1.layout.act_per_obs, dtype=torch.uint8, device=dev1)
    q1 = torch.empty((B, 3), dtype=torch.float32, device=dev1)
    side = torch.cuda.Stream(dev1)
    side.wait_stream(torch.cuda.current_stream(dev1))           # the uploads above
    assert side.cuda_stream != 0 and torch.cuda.current_device() == 0
    L, s = fwd1._L, ctypes.c_void_p(side.cuda_stream)
    check(L.snake_dqn_pack32(ctypes.byref(fwd1.cfg), int(plan == 'map'), ctypes.byref(master.struct),
                             ctypes.byref(fwd1.net), ptr(fwd1._rows), s), L)
    check(fwd1._forward_fn(ctypes.byref(fwd1.cfg), ctypes.byref(fwd1.net), ptr(obs1), B, ptr(scratch), ptr(q1), None,
                           s), L)
    assert torch.cuda.current_device() == 0
    side.synchronize()
    for k, t in fwd0.tensors.items():
        assert torch.equal(fwd1.tensors[k].cpu(), t.cpu()), k
    assert torch.equal(q1.cpu(), q0)


def _chain(dev):
    from marlenv import Collector, DQNLearner, PyRandom, ReplayBuffer, SnakeVecEnv
    env = SnakeVecEnv(8, num_snakes=2, vision_range=2, device=dev, height=12, width=12, seed=3)   # plan_cases' 12x12
    buf = ReplayBuffer(env.obs_shape, 64)
    learner = DQNLearner(probe_net(5, 5, 8, 3, 0), 5, 5, 8, device=dev)
    actor = learner.actor()
    rng = PyRandom(range(9))
    Collector(env, buf).run(actor, steps=4, epsilon=0.5, rng=rng)
    loss = learner.update(*buf.sample(8, rng=rng, stream=8))
    assert {buf.device, rng.device, actor.device, learner.device, loss.device} == {torch.device(dev)}
    assert torch.cuda.current_device() == 0
    return (loss.cpu().view(torch.int32).item(), {k: v.cpu() for k, v in learner.state_dict().items()},
            rng.getstate(8), len(buf))


def test_training_chain_on_the_second_device(two_devices):
    """Env, replay buffer, learner, its actor and a PyRandom on one device --
    the buffer and the generator bound by the first tensors they see -- while
    device 0 is current: four collected steps and one update give the same loss
    bits, weights and generator state on cuda:1 as on cuda:0."""
    loss0, state0, rng0, held0 = _chain('cuda:0')
    loss1, state1, rng1, held1 = _chain('cuda:1')
    assert held0 == held1 and held0 >= 8
    assert loss0 == loss1
    assert state0.keys() == state1.keys()
    for k in state0:
        assert torch.equal(state0[k], state1[k]), k
    assert rng0 == rng1
