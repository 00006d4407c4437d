"""An arena with guard bands: the extents of what a kernel writes.

Every entry point of the library works on buffers the caller sizes by a plan
function (include/snake_env.h). Arena carves each buffer at EXACTLY that byte
count out of one uint8 allocation filled with GUARD_BYTE. Every payload starts
at a 256-byte aligned address and owns two guard bands: at least GUARD bytes
before its first byte, and GUARD bytes that begin at the first byte past its
end (not at the next aligned address). check() compares the whole arena with
the fill in one pass on the arena's device: a byte written before a buffer or
past its end fails, and the message names the buffer, the side, the first
offset and the number of changed bytes.

Payloads start as FILL_BYTE (outputs and scratch: a byte the kernel did not
write still reads 0x5A when the payload is compared with the reference) or as
zero (what the header says the caller zeroes).

GUARD is a condition, not a measurement: it exceeds one wave's widest store
(64 lanes x 16 bytes) and the staged encode's 8 KB group, so an overrun by one
tile, row group or line lands inside it. The arena sees stray writes only: a
read outside a buffer is invisible to it.
"""
import ctypes

import numpy as np
import torch

GUARD = 16384
ALIGN = 256
GUARD_BYTE = 0xA5
FILL_BYTE = 0x5A


class Arena:
    """sizes: the byte counts of the payloads that will be taken (any order)."""

    def __init__(self, sizes, device='cuda'):
        sizes = [int(s) for s in sizes]
        total = sum(sizes) + len(sizes) * (2 * GUARD + ALIGN) + ALIGN
        self.device = torch.device(device)
        self.raw = torch.full((total,), GUARD_BYTE, dtype=torch.uint8, device=self.device)
        self.base = self.raw.data_ptr()
        self.names, self.spans = [], []
        self._end = 0           # first arena offset behind the last payload's rear guard
        self._mask = None

    def take(self, name, nbytes, dtype=torch.uint8, shape=None, fill=FILL_BYTE):
        """A tensor of exactly nbytes bytes at a 256-byte aligned address, viewed
        as dtype (and shape); fill: 'zero' or a byte value."""
        nbytes = int(nbytes)
        assert nbytes >= 0 and name not in self.names, name
        start = self._end + GUARD
        start += -(self.base + start) % ALIGN
        end = start + nbytes
        assert end + GUARD <= self.raw.numel(), f'arena too small for {name} ({nbytes} bytes)'
        self.names.append(name)
        self.spans.append((start, end))
        self._end = end + GUARD
        self._mask = None
        payload = self.raw[start:end]
        payload.fill_(0 if fill == 'zero' else int(fill))
        esize = torch.empty((), dtype=dtype).element_size()
        assert nbytes % esize == 0, f'{name}: {nbytes} bytes are no whole number of {dtype}'
        t = payload if dtype == torch.uint8 else payload.view(dtype)
        return t.view(shape) if shape is not None else t

    def ptr(self, name):
        """The payload's address as a ctypes pointer."""
        return ctypes.c_void_p(self.base + self.spans[self.names.index(name)][0])

    def payload(self, name):
        a, b = self.spans[self.names.index(name)]
        return self.raw[a:b]

    def refill(self, name, fill=FILL_BYTE):
        self.payload(name).fill_(0 if fill == 'zero' else int(fill))

    def guard_mask(self):
        if self._mask is None:
            m = np.ones(self.raw.numel(), dtype=bool)
            for a, b in self.spans:
                m[a:b] = False
            self._mask = torch.from_numpy(m).to(self.device)
        return self._mask

    def check(self, where=''):
        """Every guard byte still holds GUARD_BYTE: one comparison on the arena's
        device; only a failure is located on the host."""
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)
        bad = (self.raw != GUARD_BYTE) & self.guard_mask()
        if not bool(bad.any()):
            return
        raw = self.raw.cpu().numpy()
        off = np.flatnonzero(bad.cpu().numpy())
        # payloads were carved in address order; the bytes between two of them
        # are the rear guard of the first (GUARD bytes) and then the front guard
        # of the second (the rest, alignment slack included)
        msgs = []
        for i, (name, (a, b)) in enumerate(zip(self.names, self.spans)):
            lo = self.spans[i - 1][1] + GUARD if i else 0
            before = off[(off >= lo) & (off < a)]
            after = off[(off >= b) & (off < b + GUARD)]
            if before.size:
                msgs.append(f"buffer '{name}' ({b - a} bytes): {before.size} bytes changed BEFORE it, from "
                            f'{a - before.min()} to {a - before.max()} bytes before its start '
                            f'(0x{raw[before.max()]:02x} nearest)')
            if after.size:
                msgs.append(f"buffer '{name}' ({b - a} bytes): {after.size} bytes changed AFTER it, the first at "
                            f'offset {after.min() - b} past its end, the last at {after.max() - b} '
                            f'(0x{raw[after.min()]:02x} first)')
        tail = off[off >= self._end]
        if tail.size:
            msgs.append(f'{tail.size} bytes changed behind the last guard')
        raise AssertionError(f'{where}: write outside a buffer: ' + '; '.join(msgs))


def untouched(t):
    """Per byte of payload tensor t: True where it still holds FILL_BYTE."""
    return t.contiguous().view(-1).view(torch.uint8) == FILL_BYTE
