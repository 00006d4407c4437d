"""A host copy of the body-ring bookkeeping of logic_body (step_logic.h), one
snake at a time, with switchable deliberate faults. It is no reference -- the
oracle is -- but a way to show, without running a broken kernel, that the
long-snake cases (grow_policy.py) would see a subtly wrong ring: the copy
without faults follows the oracle through every case, and each fault makes a
named case leave the oracle in a named kind of step (test_long_snakes_cpu.py).

State, as in the snake record: the ring bytes, ring head rh, direction count
rl, the packed tail queue tq (entry 0 = directions[-1], count in bits 28-31),
the pending head-word bits hbuf; plus the head and tail cells.

FAULTS (each is one plausible slip in the kernel):
  refill_below_head   the refill count ignores the head bound: n = t - base + 1
  refill_no_pending   the refill takes pending head-word bytes from the ring chunk
  refill_patch_tail   the refill patches every byte of the head's word, also the
                      deque's last directions wrapped in behind the head
  death_no_pending    the death walk does not patch the pending head-word bytes
  death_round_short   the rounds after the first stop one direction early
  death_no_wrap       the rounds after the first do not wrap at the ring's end
  handover_15th       a 15th entry is packed into the whole tail queue
"""
_DR = (-1, 0, 1, 0)
_DC = (0, 1, 0, -1)
_DIR = {(-1, 0): 0, (0, 1): 1, (1, 0): 2, (0, -1): 3}

FAULTS = ('refill_below_head', 'refill_no_pending', 'refill_patch_tail', 'death_no_pending', 'death_round_short', 'death_no_wrap',
          'handover_15th')


class RingSnake:
    def __init__(self, ring, coords, whole, faults=()):
        """coords head first. ring: the snake's bytearray of ring_cap bytes, kept
        by the caller across resets as the device keeps it (stale bytes stay).
        whole: the tail queue as a reset builds it (the whole deque, up to 14
        directions); else as inject does (one entry)."""
        co = [tuple(c) for c in coords]
        dirs = [_DIR[(a[0] - b[0], a[1] - b[1])] for a, b in zip(co[:-1], co[1:])]
        self.ring, self.cap, self.faults = ring, len(ring), frozenset(faults)
        ring[:len(dirs)] = bytes(dirs)
        self.rh, self.rl, self.hbuf = 0, len(dirs), 0
        self.head, self.tail = co[0], co[-1]
        if whole:
            n = min(len(dirs), 14)
            self.tq = sum(dirs[-1 - j] << (2 * j) for j in range(n)) | (n << 28)
        else:
            self.tq = dirs[-1] | (1 << 28)

    def move(self, d, eat):
        """One step of a snake that stays alive, heading d."""
        ring, mask, f = self.ring, self.cap - 1, self.faults
        tq, rh, rl, hbuf = self.tq, self.rh, self.rl, self.hbuf
        tdir, tcnt0 = tq & 3, tq >> 28
        tfull = tcnt0 == rl
        rt1 = (((rh - 1) & mask) + rl - 1) & mask
        rbase = rt1 & ~7
        rchunk = bytes(ring[rbase:rbase + 8])   # (read before this step's head-word store)
        rh = (rh - 1) & mask
        ho = rh & 3
        hbuf = (hbuf & ~(3 << (2 * ho))) | (d << (2 * ho))
        hfull = hbuf
        if ho == 0:
            ring[rh:rh + 4] = bytes((hbuf >> s) & 3 for s in (0, 2, 4, 6))
            hbuf = 0
        if not eat:
            self.tail = (self.tail[0] + _DR[tdir], self.tail[1] + _DC[tdir])
            cnt = tcnt0 - 1
            tq = ((tq & 0x0fffffff) >> 2) | (cnt << 28)
            if tfull:
                tq = (tq & 0x0fffffff) | (d << (2 * cnt)) | ((cnt + 1) << 28)
            elif cnt == 0:
                t, base = rt1, rbase
                n = t - base + 1
                if 'refill_below_head' not in f:
                    n = min(n, ((t - rh) & mask) + 1)
                nq = 0
                for j in range(n):
                    p = t - j
                    dd = rchunk[p - base] & 3
                    if 'refill_no_pending' not in f and (p >> 2) == (rh >> 2) and (p >= rh or 'refill_patch_tail' in f):
                        dd = (hfull >> (2 * (p & 3))) & 3
                    nq |= dd << (2 * j)
                tq = nq | (n << 28)
        else:
            if tfull and (tcnt0 < 14 or ('handover_15th' in f and tcnt0 < 15)):
                tq = ((tq & 0x0fffffff) | (d << (2 * tcnt0)) | ((tcnt0 + 1) << 28)) & 0xffffffff
            rl += 1
        self.head = (self.head[0] + _DR[d], self.head[1] + _DC[d])
        self.tq, self.rh, self.rl, self.hbuf = tq, rh, rl, hbuf

    def death_cells(self):
        """The cells the death walk clears: the head and the body without the
        tail (the tail cell is cleared by the tail rule)."""
        ring, cap, f = self.ring, self.cap, self.faults
        rh, hbuf, n = self.rh, self.hbuf, self.rl - 1
        c0, c1 = rh & (cap - 16), (rh + 16) & (cap - 16)
        two = bytes(ring[c0:c0 + 16]) + bytes(ring[c1:c1 + 16])
        r, c = self.head
        cells = [(r, c)]
        for m0 in range(0, n, 16):
            d = [0] * 16
            for t in range(16):
                if m0 == 0:
                    d[t] = two[(rh & 15) + t] if t < n else 0
                else:
                    last = n - 1 if 'death_round_short' in f else n
                    p = rh + m0 + t
                    if 'death_no_wrap' in f:
                        d[t] = (ring[p] if p < cap else 0) if m0 + t < last else 0
                    else:
                        d[t] = ring[p & (cap - 1)] if m0 + t < last else 0
            if m0 == 0 and rh & 3 and 'death_no_pending' not in f:
                for t in range(4 - (rh & 3)):
                    d[t] = (hbuf >> (2 * ((rh & 3) + t))) & 3
            for t in range(16):
                if m0 + t < n:
                    r, c = r - _DR[d[t] & 3], c - _DC[d[t] & 3]
                    cells.append((r, c))
        return cells
