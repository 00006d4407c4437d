"""CPython's `random` restated on raw 32-bit words, the cases the device streams
are tested on, and the reference trainer's loops (train_dqn.py:163-165,
:277-301) restated on a stdlib generator.

The model functions take `u32`, a callable that returns the generator's next
tempered MT19937 word (random.Random.getrandbits(32) is exactly one); they are
what pyrandom_kernels.hip implements. The expected values of every GPU test
come from the stdlib itself, never from this model: test_pyrandom_cpu.py holds
the model to the stdlib."""
import math
import random

import numpy as np

SEEDS = (0, 1, 2, 3, 4, 5)
# (n, B) at every branch edge of random.sample: n == B, the pool/set threshold
# (setsize 4117 at B = 512, 21 at B <= 5), the reference's BUFFER_SIZE, a power
# of two (half of its words rejected) and one above it
SAMPLE_CASES = [(n, 512) for n in (512, 513, 4116, 4117, 4118, 10000, 2 ** 20, 2 ** 20 + 1)] + [
    (5, 5), (21, 5), (22, 5), (1, 1), (65537, 64)]


def getrandbits(u32, k):
    return u32() >> (32 - k)


def randbelow(u32, n):
    k = n.bit_length()
    r = getrandbits(u32, k)
    while r >= n:
        r = getrandbits(u32, k)
    return r


def random_double(u32):
    a, b = u32() >> 5, u32() >> 6
    return (a * 67108864 + b) / 9007199254740992


def setsize_int(k):
    """The integer rule of the kernels: 21, and for k > 5 also the smallest
    power of four that is at least 3 k."""
    setsize = 21
    if k > 5:
        p = 1
        while p < 3 * k:
            p *= 4
        setsize += p
    return setsize


def setsize_float(k):
    """Lib/random.py's own lines."""
    setsize = 21
    if k > 5:
        setsize += 4 ** math.ceil(math.log(k * 3, 4))
    return setsize


def sample(u32, n, k):
    """random.sample(range(n), k)."""
    assert 0 <= k <= n
    out = [None] * k
    if n <= setsize_int(k):
        pool = list(range(n))
        for i in range(k):
            j = randbelow(u32, n - i)
            out[i] = pool[j]
            pool[j] = pool[n - i - 1]
    else:
        selected = set()
        for i in range(k):
            j = randbelow(u32, n)
            while j in selected:
                j = randbelow(u32, n)
            selected.add(j)
            out[i] = j
    return out


def word_source(rnd):
    return lambda: rnd.getrandbits(32)


def advanced(seed, words):
    """random.Random(seed) after `words` 32-bit draws."""
    rnd = random.Random(seed)
    for _ in range(words):
        rnd.getrandbits(32)
    return rnd


def select_actions(rnd, q, skip, epsilon):
    """One env's actions of one step: the loop of :280-285 around
    Agent.select_action (:163-165, training=True). q: (S, A) Q-values; skip:
    (S,) the snakes that were already done."""
    A = q.shape[1]
    actions = []
    for i in range(q.shape[0]):
        if skip[i]:
            actions.append(0)
        elif rnd.random() < epsilon:
            actions.append(rnd.randrange(A))
        else:
            actions.append(int(np.argmax(q[i])))
    return actions


def trainer_loop(rnd, q, skip, epsilon, batch, min_held, capacity):
    """Trainer.train's inner loop (:277-301) on recorded Q-values and done
    masks, all draws from the one generator: per step the actions, then the
    push of one transition per live snake, then update_model's
    random.sample(self.memory.buffer, batch) once min_held are held. Returns
    the actions per step and the index lists (None before min_held)."""
    buffer_len, actions, batches = 0, [], []
    for t in range(q.shape[0]):
        actions.append(select_actions(rnd, q[t], skip[t], epsilon))
        buffer_len = min(buffer_len + int((~skip[t]).sum()), capacity)
        batches.append(rnd.sample(range(buffer_len), batch) if buffer_len >= min_held else None)
    return actions, batches
