"""numpy restatement of the safe-action rule (include/snake_env.h,
snake_safe_actions), written from the rules: the yardstick of the policy tests.

safe_actions() takes one batch on the host and returns the actions, the new
directions and, per snake, which rule decided: the rule that masked the move
the plain argmax of the Q-values would have taken, or NONE when that move is
not masked.
"""
import numpy as np

UNKNOWN = -128
DEADLY = (0, 2, 3, 4, 6, 7)
NEIGH = ((-1, 0), (1, 0), (0, -1), (0, 1))
# why a move is masked, in test order; SKIP / NOHEAD: no move was examined
NONE, OUTSIDE, OCCUPIED, DEADLY_CELL, NEAR_HEAD, FILL, SKIP, NOHEAD = range(8)
RULE_NAMES = ('none', 'outside', 'occupied', 'deadly', 'near_head', 'fill', 'skip', 'nohead')


def first_cell(plane):
    """(y, x) of the first row-major cell equal to 1, or None."""
    idx = np.flatnonzero(plane.reshape(-1) == 1)
    if idx.size == 0:
        return None
    return divmod(int(idx[0]), plane.shape[1])


def fill_count(free, start, limit):
    """min(limit, size of the 4-connected component of start); start itself counts."""
    h, w = free.shape
    seen = {start}
    stack = [start]
    while stack and len(seen) < limit:
        y, x = stack.pop()
        for dy, dx in NEIGH:
            c = (y + dy, x + dx)
            if 0 <= c[0] < h and 0 <= c[1] < w and free[c] and c not in seen:
                seen.add(c)
                stack.append(c)
    return min(limit, len(seen))


def one_snake(o, q, d, occupied, limit):
    """o: (h, w, 8) uint8; q: (3,) float32; d: (dy, dx) or None.
    Returns (action, direction, claimed cell or None, rule)."""
    h, w = o.shape[:2]
    head = first_cell(o[:, :, 5])
    if head is None:
        return 0, (0, 0), None, NOHEAD
    hy, hx = head
    if d is None:
        d = (-1, 0)
        for dy, dx in NEIGH:
            y, x = hy - dy, hx - dx
            if 0 <= y < h and 0 <= x < w and (o[y, x, 6] == 1 or o[y, x, 7] == 1):
                d = (dy, dx)
                break
    dy, dx = d
    moves = ((dy, dx), (-dx, dy), (dx, -dy))
    deadly = np.zeros((h, w), bool)
    for ch in DEADLY:
        deadly |= o[:, :, ch] == 1
    length = int((o[:, :, 5] == 1).sum()) + int((o[:, :, 6] == 1).sum()) + int((o[:, :, 7] == 1).sum())
    why = [NONE] * 3
    for a, (my, mx) in enumerate(moves):
        y, x = hy + my, hx + mx
        if not (0 <= y < h and 0 <= x < w):
            why[a] = OUTSIDE
            continue
        if (y, x) in occupied:
            why[a] = OCCUPIED
            continue
        if deadly[y, x]:
            why[a] = DEADLY_CELL
            continue
        if any(0 <= y + ny < h and 0 <= x + nx < w and o[y + ny, x + nx, 2] == 1 for ny, nx in NEIGH):
            why[a] = NEAR_HEAD
            continue
        fruit = o[y, x, 1] == 1
        free = ~deadly
        if not fruit:
            tail = first_cell(o[:, :, 7])
            if tail is not None and not any(o[tail[0], tail[1], ch] == 1 for ch in DEADLY if ch != 7):
                free[tail] = True
        free[hy, hx] = False
        if fill_count(free, (y, x), limit) < length + (1 if fruit else 0):
            why[a] = FILL
    masked = np.array([-np.inf if why[a] else q[a] for a in range(3)], np.float32)
    act = int(np.argmax(masked))        # the first index of the maximum
    my, mx = moves[act]
    return act, (my, mx), (hy + my, hx + mx), why[int(np.argmax(q))]


def safe_actions(obs, q, skip, dirs, limit=60):
    """obs (N, S, h, w, 8) uint8; q (N, S, 3) float32; skip (N, S) or None; dirs
    (N, S, 2) int8. Returns (actions int8 (N, S), dirs_out int8 (N, S, 2),
    rule int8 (N, S))."""
    N, S = obs.shape[:2]
    q = np.asarray(q, np.float32).reshape(N, S, 3)
    actions = np.zeros((N, S), np.int8)
    out = np.array(dirs, np.int8).reshape(N, S, 2).copy()
    rule = np.zeros((N, S), np.int8)
    for n in range(N):
        occupied = set()
        for s in range(S):
            if skip is not None and skip[n, s]:
                rule[n, s] = SKIP
                continue
            d = None if (out[n, s] == UNKNOWN).all() else (int(out[n, s, 0]), int(out[n, s, 1]))
            a, nd, cell, r = one_snake(obs[n, s], q[n, s], d, occupied, limit)
            actions[n, s], rule[n, s] = a, r
            out[n, s] = np.array(nd, np.int64).astype(np.int8)
            if cell is not None:
                occupied.add(cell)
    return actions, out, rule


def load_calls():
    """tests/golden/policy_calls.npz (tests/golden/gen/make_policy_golden.py) as
    {config: dict(obs (R, S, h, w, 8) uint8, q, skip, din, act, dout)}."""
    import golden_io
    z = golden_io.load('policy_calls.npz')
    out = {}
    for name in sorted(k[:-6] for k in z.files if k.endswith('_shape')):
        S, h, w = (int(v) for v in z[name + '_shape'])
        d = {k: z[name + '_' + k] for k in ('q', 'skip', 'din', 'act', 'dout')}
        bits = np.unpackbits(z[name + '_obs'], axis=1)[:, :S * h * w * 8]
        d['obs'] = np.ascontiguousarray(bits.reshape(-1, S, h, w, 8))
        out[name] = d
    return out
