"""The fp32 kernel layout of the reference DQN's weights (include/snake_env.h
snake_dqn32_net), in one place: the fp32 forward, the learner's buffers and the
source of every bf16 pack (snake_dqn_pack32) are a Net32.

The reference's state dict holds conv weights [out][in][3][3] and fc1 columns
ch * h*w + position (the NCHW flatten); the kernels read conv weights
[out][(tap, ci)] and fc1 columns position * 64 + ch. The other nine tensors are
the same in both."""
from ._device import get_torch
from ._native import Dqn32Net

# snake_dqn32_net's field order, with the reference's parameter names
FIELDS = ('conv1_w', 'conv2_w', 'conv3_w', 'fc1_w', 'fc2_w', 'fc3_w',
          'conv1_b', 'conv2_b', 'conv3_b', 'fc1_b', 'fc2_b', 'fc3_b')
NAMES = tuple(f[:-2] + ('.weight' if f.endswith('_w') else '.bias') for f in FIELDS)
PAD = 16        # floats: every tensor starts at a multiple of 64 bytes


# The reference network's parameter shapes (train_dqn.py:104-151): the kernels
# hard-code 32/64/64 conv channels and 256/128 fc widths, so a mismatched state
# dict must raise here instead of making them read past the weights.
def check_shapes(state, C, P, A):
    want = {'conv1.weight': (32, C, 3, 3), 'conv1.bias': (32,),
            'conv2.weight': (64, 32, 3, 3), 'conv2.bias': (64,),
            'conv3.weight': (64, 64, 3, 3), 'conv3.bias': (64,),
            'fc1.weight': (256, 64 * P), 'fc1.bias': (256,),
            'fc2.weight': (128, 256), 'fc2.bias': (128,),
            'fc3.weight': (A, 128), 'fc3.bias': (A,)}
    for name, shape in want.items():
        if name not in state:
            raise ValueError('state dict has no %s' % name)
        got = tuple(state[name].shape)
        if got != shape:
            raise ValueError('%s shape %s != %s' % (name, got, shape))


def kernel_shapes(P, C, A):
    """The twelve tensors' shapes in the kernel layouts, in FIELDS order."""
    return ((32, 9 * C), (64, 288), (64, 576), (256, 64 * P), (128, 256), (A, 128),
            (32,), (64,), (64,), (256,), (128,), (A,))


def to_kernel(name, t, P):
    """A reference-layout tensor (conv [out][in][3][3], fc1 columns ch*P + p) in
    the kernel layout (conv [out][(tap, ci)], fc1 columns p*64 + ch)."""
    if name.startswith('conv') and t.dim() == 4:
        return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1)
    if name == 'fc1.weight':
        return t.reshape(256, 64, P).permute(0, 2, 1).reshape(256, P * 64)
    return t


def from_kernel(name, t, P):
    """The inverse of to_kernel (a new contiguous tensor)."""
    if name.startswith('conv') and t.dim() == 2:
        return t.reshape(t.shape[0], 3, 3, -1).permute(0, 3, 1, 2).contiguous()
    if name == 'fc1.weight':
        return t.reshape(256, P, 64).permute(0, 2, 1).reshape(256, 64 * P).contiguous()
    return t.clone()


class Net32:
    """One net in the kernel layout: `flat`, a zeroed float32 buffer on `device`
    (a cuda device or 'cpu'); `views`, the twelve tensors by the reference's
    names, views into it at offsets padded to 64 bytes; `struct`, the Dqn32Net
    of their addresses. `flat=` gives the net a buffer of the caller's instead
    (contiguous float32, Net32.size(P, C, A) elements, 16-byte aligned), used
    as it is: nothing is zeroed."""

    @staticmethod
    def spans(P, C, A):
        """((offset, elements, shape) of the twelve tensors in FIELDS order, total elements)."""
        spans, off = [], 0
        for shape in kernel_shapes(P, C, A):
            size = shape[0] * (shape[1] if len(shape) == 2 else 1)
            spans.append((off, size, shape))
            off += (size + PAD - 1) // PAD * PAD
        return spans, off

    @classmethod
    def size(cls, P, C, A):
        return cls.spans(P, C, A)[1]

    def __init__(self, P, C, A, device=None, flat=None):
        torch = get_torch()
        self.P, self.C, self.A = P, C, A
        spans, off = self.spans(P, C, A)
        self.numel = off
        if flat is not None:
            if flat.dtype != torch.float32 or flat.dim() != 1 or flat.numel() != off or not flat.is_contiguous():
                raise ValueError('flat must be a contiguous float32 tensor of %d elements' % off)
            if flat.data_ptr() % 16:
                raise ValueError('flat must be 16-byte aligned')
            self.flat = flat
        else:
            self.flat = torch.zeros(off, dtype=torch.float32, device=device)
        self.views = {name: self.flat[o:o + size].view(shape) for name, (o, size, shape) in zip(NAMES, spans)}
        base = self.flat.data_ptr()
        self.struct = Dqn32Net(*(base + 4 * o for o, _, _ in spans))

    def load(self, state):
        """Overwrite the net from a state dict of the reference's names."""
        check_shapes(state, self.C, self.P, self.A)
        for name, view in self.views.items():
            t = state[name].detach().to(device=view.device, dtype=view.dtype)
            view.copy_(to_kernel(name, t, self.P))
        return self

    def unpack(self):
        """The net with the reference's names and layouts (copies)."""
        return {name: from_kernel(name, view, self.P) for name, view in self.views.items()}
