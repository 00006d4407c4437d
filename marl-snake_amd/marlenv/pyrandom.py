"""Python's `random` module on the device.

The reference trainer draws all of its randomness from one `random` stream:
`random.random() < epsilon` and `random.randrange(3)` per live snake
(train_dqn.py:163-165) and `random.sample(buffer, batch_size)` per update
(:96-97). PyRandom keeps n such generators -- the 624 key words and the position
of `random.Random.getstate()[1]` -- in device memory; snake_pyrandom_act and
snake_pyrandom_sample (marl-snake_amd/csrc/pyrandom_kernels.hip; the exact
semantics are in include/snake_env.h) consume them word for word as CPython
does, so actions, minibatch indices and the generator state afterwards equal
the stdlib's. Seeding happens on the host through `random.Random(seed)` itself.
"""
import random

from ._device import get_torch as _torch, bind_device, ptr, stream_ptr
from ._native import check, lib

MT_N = 624


class PyRandom:
    """n independent `random.Random` streams on the device.

    seeds: an int or a sequence of ints, one stream each, seeded like
    random.Random(seed). device: a HIP device, or None for that of the first
    tensor the streams are used with. `n` is the stream count, `err` the device
    int32 the kernels set (and never clear) when a bounded rejection loop ran
    out, a position was out of range or a sample asked for more than is held."""

    def __init__(self, seeds, device=None, lib_path=None):
        if isinstance(seeds, int):
            seeds = [seeds]
        self._setup([random.Random(int(s)).getstate() for s in seeds], device, lib_path)

    @classmethod
    def from_states(cls, states, device=None, lib_path=None):
        """Streams from saved `random.Random.getstate()` tuples."""
        self = cls.__new__(cls)
        self._setup(list(states), device, lib_path)
        return self

    def _setup(self, states, device, lib_path):
        if not states:
            raise ValueError('PyRandom needs at least one stream')
        for st in states:
            if len(st) != 3 or st[0] != 3 or len(st[1]) != MT_N + 1 or not 0 <= st[1][MT_N] <= MT_N:
                raise ValueError('not a random.Random.getstate() tuple (version 3, 624 words and a position)')
        self._L = lib(lib_path)
        self._host = states             # until the device arrays exist
        self._gauss = [st[2] for st in states]
        self.n = len(states)
        self.device = _torch().device(device) if device is not None else None
        self.key = self.pos = self.err = None

    # ---------------------------------------------------------------- buffers
    def _on(self, t, name):
        """Binds the streams to the device of tensor `name` and, at the first
        use, creates the device arrays there."""
        torch = _torch()
        bind_device(self, t.device, name, name + ' is')
        dev = self.device
        if self.key is None:
            import numpy as np
            words = np.array([st[1] for st in self._host], dtype=np.uint32)
            self.key = torch.from_numpy(words[:, :MT_N].copy().view(np.int32)).to(dev)
            self.pos = torch.from_numpy(words[:, MT_N].astype(np.int32)).to(dev)
            self.err = torch.zeros(1, dtype=torch.int32, device=dev)
            self._host = None
        return dev

    def getstate(self, i=0):
        """Stream i as a tuple that random.Random().setstate accepts. Syncs."""
        i = int(i)
        if not 0 <= i < self.n:
            raise IndexError('stream %d of %d' % (i, self.n))
        if self.key is None:
            return self._host[i]
        import numpy as np
        words = self.key[i].cpu().numpy().view(np.uint32)
        return (3, tuple(int(w) for w in words) + (int(self.pos[i].item()),), self._gauss[i])

    # --------------------------------------------------------------- launches
    def act(self, q, num_snakes, epsilon, skip=None):
        """Epsilon-greedy actions, one launch. q: float32 (N * S, A) Q-values;
        skip: bool/uint8 (N, S) or None. Env e draws from stream e (N <= n): per
        snake in slot order, a skipped one gets 0 and draws nothing, every other
        one draws random() and then, below epsilon, randrange(A); otherwise it
        takes the first maximal Q-value. Returns int8 (N, S). No host sync."""
        torch = _torch()
        S = int(num_snakes)
        if not isinstance(q, torch.Tensor) or q.dim() != 2 or q.shape[0] % S:
            raise ValueError('q must be a (N * %d, A) tensor' % S)
        N, A = q.shape[0] // S, q.shape[1]
        if N > self.n:
            raise ValueError('%d envs need %d streams, this PyRandom has %d' % (N, N, self.n))
        check(self._L.snake_pyrandom_plan(A, 1, 1), self._L)
        dev = self._on(q, 'q')
        q = q.to(torch.float32).contiguous()
        if skip is not None:
            if tuple(skip.shape) != (N, S) or skip.device != dev:
                raise ValueError('skip must be (%d, %d) on %s' % (N, S, dev))
            skip = skip.contiguous().view(torch.uint8) if skip.dtype == torch.bool else skip.to(torch.uint8).contiguous()
        actions = torch.empty((N, S), dtype=torch.int8, device=dev)
        with torch.cuda.device(dev):
            check(self._L.snake_pyrandom_act(ptr(q), ptr(skip), float(epsilon), ptr(self.key), ptr(self.pos),
                                             ptr(actions), ptr(self.err), N, S, A, stream_ptr(dev)), self._L)
        self._keep = (q, skip)
        return actions

    def sample(self, count, capacity, batch_size, stream=0, out=None):
        """random.sample(range(n), batch_size) from stream `stream`, with n =
        min(count, capacity) read on the device. count: int64 (1,) device
        tensor. Returns int64 (batch_size,) indices (or fills `out`). One
        launch, no host sync."""
        torch = _torch()
        B, stream = int(batch_size), int(stream)
        if not 0 <= stream < self.n:
            raise ValueError('stream must be in [0, %d) (got %d)' % (self.n, stream))
        check(self._L.snake_pyrandom_plan(1, B, int(capacity)), self._L)
        dev = self._on(count, 'count')
        if count.dtype != torch.int64 or count.numel() != 1:
            raise TypeError('count must be one int64 on the device')
        idx = out if out is not None else torch.empty(B, dtype=torch.int64, device=dev)
        if idx.dtype != torch.int64 or tuple(idx.shape) != (B,) or not idx.is_contiguous() or idx.device != dev:
            raise ValueError('out must be a contiguous int64 (%d,) tensor on %s' % (B, dev))
        with torch.cuda.device(dev):
            check(self._L.snake_pyrandom_sample(ptr(self.key), ptr(self.pos), stream, ptr(count), int(capacity), B,
                                                ptr(idx), ptr(self.err), stream_ptr(dev)), self._L)
        return idx


def setsize(batch_size, L=None):
    """random.sample's set/pool threshold for batch_size draws (snake_pyrandom_plan)."""
    L = L or lib()
    return check(L.snake_pyrandom_plan(1, int(batch_size), 1), L)
