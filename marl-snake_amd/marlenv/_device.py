"""What the wrappers of the policy, genome and replay kernels share on the
Python side: the lazy torch import, the rule that binds an object to the device
of the first tensor it sees, the skip mask and the current stream's pointer."""
import ctypes


def get_torch():
    import torch
    return torch


def bind_device(obj, dev, needs, subject):
    """obj.device becomes `dev` when it is still open (None, or 'cuda' without an
    index); ValueError when dev is no GPU or another one than obj.device.
    needs / subject: the tensor's name in the two messages."""
    name = type(obj).__name__
    if dev.type != 'cuda':
        raise ValueError('%s needs the %s on the GPU (got %s); there is no CPU fallback' % (name, needs, dev))
    if obj.device is None or (obj.device.type == 'cuda' and obj.device.index is None):
        obj.device = dev
    if dev != obj.device:
        raise ValueError('%s on %s, this %s on %s' % (subject, dev, name, obj.device))


def skip_mask(skip, N, S, dev):
    """skip (anything as_tensor takes, or None) as a contiguous uint8 (N, S) on dev."""
    if skip is None:
        return None
    torch = get_torch()
    return torch.as_tensor(skip, device=dev).reshape(N, S).to(torch.uint8).contiguous()


def ptr(t):
    """t's address for the C-ABI (None: a NULL pointer)."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream_ptr(dev):
    """The current stream of dev, as the C-ABI takes it."""
    return ctypes.c_void_p(get_torch().cuda.current_stream(dev).cuda_stream)
