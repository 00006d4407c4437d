"""What the wrappers of the kernels share on the Python side: the lazy torch
import, the one rule for the device an object lives on -- named at construction
(default_device) or taken from the first tensor it sees (bind_device) -- the one
check of a tensor argument (check_tensor, check_on), the skip mask, and the
pointers the C-ABI takes. Nothing here touches the GPU before a check passed."""
import ctypes


def get_torch():
    import torch
    return torch


def need_gpu(who):
    """RuntimeError without a GPU (asks torch, initialises nothing). who: the
    owner's name in the message."""
    if not get_torch().cuda.is_available():
        raise RuntimeError('%s needs a HIP device (MI355X); there is no CPU fallback' % who)


def default_device(device, who):
    """torch.device('cuda', index) for an object that allocates now: None and an
    unindexed 'cuda' become the device current at this call, which initialises
    the GPU, so every host-side rejection comes first. RuntimeError without a
    GPU (need_gpu)."""
    torch = get_torch()
    need_gpu(who)
    index = torch.device(device).index if device is not None else None
    return torch.device('cuda', torch.cuda.current_device() if index is None else index)


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


def check_tensor(who, name, t, dtypes, shape=None, contiguous=False):
    """Argument `name` of `who`: TypeError unless t is a tensor of one of
    `dtypes` (torch's names: 'uint8', or ('bool', 'uint8')) and, where asked,
    contiguous; then ValueError unless its shape is `shape`, in which None
    leaves a dimension (the batch) open. Reads no device."""
    torch = get_torch()
    names = (dtypes,) if isinstance(dtypes, str) else dtypes
    if (not isinstance(t, torch.Tensor) or t.dtype not in [getattr(torch, d) for d in names]
            or (contiguous and not t.is_contiguous())):
        raise TypeError('%s takes %s as a %s%s tensor (got %s)' % (
            who, name, 'contiguous ' if contiguous else '', ' or '.join(names), getattr(t, 'dtype', type(t).__name__)))
    if shape is not None and (t.dim() != len(shape) or any(w is not None and w != d for d, w in zip(t.shape, shape))):
        want = '(%s)' % ', '.join('B' if w is None else str(w) for w in shape)
        raise ValueError('%s shape %s is not %s' % (name, tuple(t.shape), want))


def check_on(name, t, dev, who):
    """ValueError unless tensor `name` is on `dev`, the device of this `who`."""
    if t.device != dev:
        raise ValueError('%s is on %s, this %s on %s%s' % (
            name, t.device, who, dev, '' if t.device.type == 'cuda' else '; there is no CPU fallback'))


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
