"""The reference trainer's gradient step on the GPU.

train_dqn.py's Trainer.update_model (:228-257) runs once per env step: Q(s, a)
from the policy net, max Q(s', .) from the target net, smooth-L1 loss,
backward, clip_grad_norm_(10) and optim.Adam.step(). DQNLearner is that step in
fp32 on the device: the forward of dqn32_kernels.hip, and the backward pass, TD
loss and clip + Adam of dqn_train_kernels.hip (snake_dqn32_backward,
snake_dqn_td_loss, snake_adam_step; the exact semantics are in
include/snake_env.h). backward_precision='bf16' swaps the backward's GEMMs for
their bf16 forms (dqn_train16_kernels.hip, snake_dqn32_backward_bf16), and
forward_precision='bf16' the policy forward's (dqn_fwd16_kernels.hip,
snake_dqn32_forward_bf16: the same scratch, so either backward follows either
forward); target_precision='mixed' runs the target forward through the same
function. Nothing in update() syncs with the host.

The master weights are the fp32 kernels' own layouts (snake_dqn32_net), so
acting, the target forward and the update need no repacking: parameters, target
net, gradients and Adam's m and v are one dqn_weights.Net32 each -- a flat
float32 buffer, the twelve tensors views into it at offsets padded to 64 bytes,
and the struct of their addresses, built once. state_dict(), grads() and
checkpoint() convert to the reference's names and layouts with torch ops
(Net32.unpack), off the hot path.

Acting with the weights in training goes through actor(): a bf16 DQNForward
whose buffers snake_dqn_pack32 (dqn_pack_kernels.hip) refills from the master
weights after every step, one launch, no host sync.
"""
import ctypes
import weakref

from ._device import get_torch as _torch, check_on, check_tensor, default_device, ptr, stream_ptr
from ._native import ADAM_SCRATCH_BYTES, DqnCfg, check, lib
from .dqn import DQNForward, bf16_plan, forward32, forward32_bf16
from .dqn_weights import FIELDS, NAMES, Net32, check_shapes, from_kernel, kernel_shapes, to_kernel  # noqa: F401


class DQNLearner:
    """Trainer.update_model on the device.

    state: a state dict (or nn.Module) of the reference DQN; both the policy and
    the target net start from it. height, width, channels: the observation
    (anything snake_dqn32_forward accepts). lr, betas, eps: optim.Adam's;
    gamma: the discount; max_grad_norm: clip_grad_norm_'s bound.

    learner(obs) / forward_features(obs): the policy net on uint8 (B, h, w, C)
    observations; target_q(obs): the target net. update(*buf.sample(B)) is one
    gradient step and returns the loss as a float32 () tensor on the device.
    The stages of update() are methods of their own: td_loss, backward (for
    the observations of the last policy forward), apply; grads() and grad_norm
    show what they left.

    actor() is a bf16 DQNForward that follows the policy net, for collecting
    with the policy in training. target_precision='bf16' keeps a second,
    bf16-packed copy of the target net (refreshed by sync_target(),
    load_checkpoint() and here) and runs target_q -- so update()'s target
    forward -- on the bf16 matrix cores with it (plan 'auto'); the fp32 target
    buffer, target_state_dict() and checkpoint() are the same in both modes,
    and the default 'fp32' computes exactly what it did without the option.
    Both need a geometry a bf16 plan accepts (A <= 4, 8 to 32 channels, (h+2) *
    (w+2) <= 576) and raise ValueError with the plan's message, before any
    device work, where none does. The bf16 forward reads the observations as
    0/1 bytes: unlike the fp32 forward it does not take the reference's /255
    branch. target_precision='mixed' runs target_q on the fp32 target buffer
    through snake_dqn32_forward_bf16 instead (see forward_precision): no packed
    copy, any geometry, the /255 branch included.

    forward_precision='bf16' runs learner(obs) and forward_features(obs) -- so
    update()'s policy forward -- through snake_dqn32_forward_bf16: the five
    GEMMs of the matrix cores on the bf16 matrix cores, their operands (act(X)
    formed in fp32, and the fp32 master weights) rounded to bf16 as they are
    staged, fp32 sums, the pre-activations stored fp32 where either backward
    reads them; fc3 and the features stay fp32 (the rounding points are in
    include/snake_env.h). Any geometry the fp32 forward accepts. The default
    'fp32' launches exactly what it did without the option.
    pre_activations() returns fp32 copies of the last policy forward's
    Y1..Y5 (without bias, NHWC), in both modes, off the hot path.

    backward_precision='bf16' runs backward() -- so update()'s -- weight and
    input gradients on the bf16 matrix cores (snake_dqn32_backward_bf16: the
    GEMM operands rounded to bf16 as they are staged, fp32 sums; the rounding
    points are in include/snake_env.h). The forwards, the fp32 master weights,
    Adam, grads(), state_dict(), checkpoint() and actor() are the same in both
    modes, a checkpoint of one loads into the other, and the default 'fp32'
    computes exactly what it did without the option. Any geometry the fp32
    backward accepts. The same holds across forward_precision and
    target_precision: a checkpoint of any mode loads into any other."""

    def __init__(self, state, height, width, channels, num_actions=3, lr=5e-4, gamma=0.99, betas=(0.9, 0.999),
                 eps=1e-8, max_grad_norm=10.0, device=None, lib_path=None, target_precision='fp32',
                 backward_precision='fp32', forward_precision='fp32'):
        torch = _torch()
        if hasattr(state, 'state_dict'):
            state = state.state_dict()
        H, W, C, A = int(height), int(width), int(channels), int(num_actions)
        self._L = L = lib(lib_path)
        self._lib_path = lib_path
        self.cfg = DqnCfg(H, W, C, A, 0)
        n = L.snake_dqn32_train_scratch(ctypes.byref(self.cfg), 0)      # ValueError before any device work
        check(int(n) if n < 0 else 0, L)
        if target_precision not in ('fp32', 'bf16', 'mixed'):
            raise ValueError("target_precision must be 'fp32', 'bf16' or 'mixed'")
        if target_precision == 'bf16':
            bf16_plan(L, self.cfg)
        self.target_precision = target_precision
        if backward_precision not in ('fp32', 'bf16'):
            raise ValueError("backward_precision must be 'fp32' or 'bf16'")
        self.backward_precision = backward_precision
        if forward_precision not in ('fp32', 'bf16'):
            raise ValueError("forward_precision must be 'fp32' or 'bf16'")
        self.forward_precision = forward_precision
        check_shapes(state, C, H * W, A)
        if not (lr > 0.0 and eps >= 0.0 and max_grad_norm > 0.0 and 0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError('lr and max_grad_norm must be positive, eps >= 0, betas in [0, 1)')
        self.lr, self.gamma, self.betas, self.eps = float(lr), float(gamma), (float(betas[0]), float(betas[1])), float(eps)
        self.max_grad_norm = float(max_grad_norm)
        self.obs_shape = (H, W, C)
        self.num_actions = A
        self.device = dev = default_device(device, 'DQNLearner')
        # policy, target, gradient and Adam's m and v; and their flat buffers, which
        # the Adam kernel and the target sync take whole
        nets = self._pnet, self._tnet, self._gnet, self._mnet, self._vnet = [Net32(H * W, C, A, dev) for _ in range(5)]
        self._param, self._target, self._grad, self._m, self._v = (n.flat for n in nets)
        self.numel = self._pnet.numel
        self.step = 0
        self.grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)        # 1 once td_loss clamped an action
        self._adam_scratch = torch.zeros(ADAM_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
        self._scratch = {}          # 'policy' / 'target' / 'train' -> uint8 buffers
        self._fwd = None            # (obs, B) of the last policy forward
        self._keep = None
        self._actors = weakref.WeakSet()        # the auto_sync actors, held weakly
        self._target16 = DQNForward.empty(H, W, C, A, device=dev, lib_path=lib_path) \
            if target_precision == 'bf16' else None
        self._pnet.load(state)
        self.sync_target()

    def _buffer(self, key, nbytes):
        torch = _torch()
        buf = self._scratch.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = self._scratch[key] = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=self.device)
        return buf

    # ----------------------------------------------------------------- forward
    def _check_obs(self, obs, who):
        check_tensor('DQNLearner.' + who, 'observations', obs, 'uint8', (None,) + self.obs_shape, contiguous=True)
        check_on('observations', obs, self.device, 'DQNLearner')
        return obs.shape[0]

    def _forward(self, net, key, obs, features, who):
        B = self._check_obs(obs, who)
        mixed = self.forward_precision == 'bf16' if key == 'policy' else self.target_precision == 'mixed'
        q, feat, self._scratch[key] = (forward32_bf16 if mixed else forward32)(
            self._L, self.cfg, net.struct, obs, self._scratch.get(key), features)
        if key == 'policy':
            self._fwd = (obs, B)
        return q, feat

    def __call__(self, obs):
        """The policy net's Q-values: uint8 (B, h, w, C) -> float32 (B, A)."""
        return self._forward(self._pnet, 'policy', obs, False, '__call__')[0]

    def forward_features(self, obs):
        """The policy net's relu(fc2): float32 (B, 128)."""
        return self._forward(self._pnet, 'policy', obs, True, 'forward_features')[1]

    def pre_activations(self):
        """{'Y1'..'Y5'}: float32 copies of the pre-activations (without bias) the
        last policy forward left in its scratch, shaped (B, h, w, 32), (B, h, w,
        64), (B, h, w, 64), (B, 256) and (B, 128). ValueError before any policy
        forward."""
        torch = _torch()
        if self._fwd is None:
            raise ValueError('pre_activations needs a policy forward (call learner(obs) first)')
        B, (H, W, _) = self._fwd[1], self.obs_shape
        flat = self._scratch['policy'][16:].view(torch.float32)
        out, at = {}, 0
        for name, shape in (('Y1', (B, H, W, 32)), ('Y2', (B, H, W, 64)), ('Y3', (B, H, W, 64)), ('Y4', (B, 256)),
                            ('Y5', (B, 128))):
            n = 1
            for d in shape:
                n *= d
            out[name] = flat[at:at + n].view(shape).clone()
            at += n
        return out

    def target_q(self, obs):
        """The target net's Q-values (with target_precision='bf16': the bf16
        forward on the packed copy of the target net; with 'mixed': the bf16
        mixed-precision forward on the fp32 target buffer)."""
        if self._target16 is not None:
            self._check_obs(obs, 'target_q')
            return self._target16(obs)
        return self._forward(self._tnet, 'target', obs, False, 'target_q')[0]

    # ------------------------------------------------------------------ stages
    def td_loss(self, q, action, reward, done, next_q):
        """(loss, dq): the smooth-L1 loss of q[b][action[b]] against reward +
        (1 - done) * gamma * max next_q, float32 (), and its gradient with
        respect to q, float32 (B, A). q, next_q: float32 (B, A); action: int64
        (B,); reward, done: float32 (B,). An action outside [0, A) is clamped
        and sets self.err."""
        torch = _torch()
        A = self.num_actions
        check_tensor('DQNLearner.td_loss', 'q', q, 'float32', (None, A))
        B = q.shape[0]
        if B < 1:
            raise ValueError('td_loss needs at least one row')
        for name, t, dtype, shape in (('action', action, 'int64', (B,)), ('reward', reward, 'float32', (B,)),
                                      ('done', done, 'float32', (B,)), ('next_q', next_q, 'float32', (B, A))):
            check_tensor('DQNLearner.td_loss', name, t, dtype, shape)
        for name, t in (('q', q), ('action', action), ('reward', reward), ('done', done), ('next_q', next_q)):
            check_on(name, t, self.device, 'DQNLearner')
        q, action, reward, done, next_q = (t.contiguous() for t in (q, action, reward, done, next_q))
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        dq = torch.empty((B, A), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self._L.snake_dqn_td_loss(ptr(q), ptr(action), ptr(reward), ptr(done), ptr(next_q), B, A,
                                            self.gamma, ptr(loss), ptr(dq), ptr(self.err),
                                            stream_ptr(self.device)), self._L)
        self._keep = (q, action, reward, done, next_q)
        return loss, dq

    def backward(self, obs, dq):
        """The gradients of sum(dq * Q(obs)) into the gradient buffer. obs must be
        the tensor of the last policy forward (its scratch is what is read)."""
        B = self._check_obs(obs, 'backward')
        if self._fwd is None or self._fwd[0] is not obs or self._fwd[1] != B:
            raise ValueError('backward needs the observations of the last policy forward (call learner(obs) first)')
        check_tensor('DQNLearner.backward', 'dq', dq, 'float32', (B, self.num_actions))
        check_on('dq', dq, self.device, 'DQNLearner')
        dq = dq.contiguous()
        need = int(self._L.snake_dqn32_train_scratch(ctypes.byref(self.cfg), B))
        check(need if need < 0 else 0, self._L)
        ts = self._buffer('train', need)
        with _torch().cuda.device(self.device):
            fn = self._L.snake_dqn32_backward_bf16 if self.backward_precision == 'bf16' \
                else self._L.snake_dqn32_backward
            check(fn(ctypes.byref(self.cfg), ctypes.byref(self._pnet.struct), ptr(obs), B, ptr(self._scratch['policy']),
                     ptr(dq), ptr(ts), ctypes.byref(self._gnet.struct), stream_ptr(self.device)), self._L)
        self._keep_dq = dq

    def apply(self):
        """clip_grad_norm_ and one Adam step from the gradient buffer; the norm
        before clipping goes to self.grad_norm. The auto_sync actors are
        repacked from the new weights."""
        torch = _torch()
        self.step += 1
        with torch.cuda.device(self.device):
            check(self._L.snake_adam_step(ptr(self._param), ptr(self._grad), ptr(self._m), ptr(self._v), self.numel,
                                          self.step, self.lr, self.betas[0], self.betas[1], self.eps,
                                          self.max_grad_norm, ptr(self._adam_scratch), ptr(self.grad_norm),
                                          stream_ptr(self.device)), self._L)
        self._sync_actors()

    def update(self, state, action, reward, next_state, done):
        """update_model on ReplayBuffer.sample(format='uint8')'s five tensors;
        returns the loss, float32 () on the device. No host sync."""
        next_q = self.target_q(next_state)
        q = self(state)
        loss, dq = self.td_loss(q, action, reward, done, next_q)
        self.backward(state, dq)
        self.apply()
        return loss

    # ------------------------------------------------------------------- state
    def sync_target(self):
        """target_net.load_state_dict(policy_net.state_dict())."""
        self._target.copy_(self._param)
        if self._target16 is not None:
            self._target16.pack32(self._tnet.struct)

    # ------------------------------------------------------------------ actors
    def actor(self, plan='auto', conv_waves=0, auto_sync=True):
        """A bf16 DQNForward (DQNForward.empty: plan and conv_waves as there)
        packed from the policy net on the device, for acting with the policy
        that is being trained: Collector.run(learner.actor(), ...).

        With auto_sync the learner repacks it at the end of every apply() (so
        of every update()) and load_checkpoint(): one launch on the current
        stream, no host sync. Without, it keeps its snapshot until actor.sync()
        (= learner.sync_actor(actor)). The learner holds its auto_sync actors
        weakly: one that is no longer referenced anywhere else is dropped and
        costs nothing. A repack is ordered like any other launch on the current
        stream: act on the stream the updates run on, or order the two streams
        yourself. Raises ValueError with the plan's message, before any
        device work, where the plan rejects the geometry. The bf16 forward does
        not take the /255 branch: it is for the env's 0/1 observations."""
        a = DQNForward.empty(*self.obs_shape, num_actions=self.num_actions, device=self.device, plan=plan,
                             conv_waves=conv_waves, lib_path=self._lib_path)
        a._source = self
        a.pack32(self._pnet.struct)
        if auto_sync:
            self._actors.add(a)
        return a

    def sync_actor(self, actor):
        """Repack an actor of this learner from the policy net, on the current stream."""
        if getattr(actor, '_source', None) is not self:
            raise ValueError('sync_actor takes a DQNForward made by this learner\'s actor()')
        actor.pack32(self._pnet.struct)

    def _sync_actors(self):
        for a in list(self._actors):
            a.pack32(self._pnet.struct)

    def state_dict(self):
        """The policy net with the reference's names and layouts (copies)."""
        return self._pnet.unpack()

    def target_state_dict(self):
        return self._tnet.unpack()

    def grads(self):
        """The gradient buffer in the reference's layout (what .grad holds
        after loss.backward(), before the clip)."""
        return self._gnet.unpack()

    def checkpoint(self):
        """The learner's part of the reference's save_checkpoint (:356-383): both
        nets and Adam's state (step, exp_avg, exp_avg_sq by parameter name)."""
        return {'policy_net': self.state_dict(), 'target_net': self.target_state_dict(),
                'optimizer': {'step': self.step, 'exp_avg': self._mnet.unpack(),
                              'exp_avg_sq': self._vnet.unpack()}}

    def load_checkpoint(self, ckpt):
        opt = ckpt['optimizer']
        self._pnet.load(ckpt['policy_net'])
        self._tnet.load(ckpt['target_net'])
        self._mnet.load(opt['exp_avg'])
        self._vnet.load(opt['exp_avg_sq'])
        self.step = int(opt['step'])
        self._fwd = None
        if self._target16 is not None:
            self._target16.pack32(self._tnet.struct)
        self._sync_actors()
