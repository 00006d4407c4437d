"""numpy restatement of the greedy opponent's rule (include/snake_env.h,
snake_greedy_actions), written from the rules: the yardstick of the greedy
tests.

greedy_actions() takes one batch on the host and returns the actions, the new
directions and, per snake, a set of category bits: which way the call went
(SKIP, NOHEAD, ALLDEAD, or N1 / N2 / N3 = how many moves shared the best score)
and, where moves were scored, NOFRUIT (no fruit visible) and FRUIT_TIE (several
fruits at the smallest distance, and taking the last of them in row-major order
instead of the first would change the set of best moves).
"""
import numpy as np

UNKNOWN = -128
DEADLY = (0, 2, 3, 4, 6, 7)
NEIGH = ((-1, 0), (1, 0), (0, -1), (0, 1))
SKIP, NOHEAD, ALLDEAD, N1, N2, N3, NOFRUIT, FRUIT_TIE = (1 << i for i in range(8))
CATEGORY_NAMES = {SKIP: 'skip', NOHEAD: 'nohead', ALLDEAD: 'alldead', N1: 'n1', N2: 'n2', N3: 'n3',
                  NOFRUIT: 'nofruit', FRUIT_TIE: 'fruit_tie'}


def pick(u, n):
    """The multiply-shift choice among n: (u * n) >> 32 with u a uint32."""
    return (int(u) * int(n)) >> 32


def cells_eq1(plane):
    """The (y, x) of the cells equal to 1, in row-major order."""
    h, w = plane.shape
    return [divmod(int(i), w) for i in np.flatnonzero(plane.reshape(-1) == 1)]


def best_moves(o, head, moves, fruit):
    """The live moves of maximal score in ascending order (empty: all dead)."""
    h, w = o.shape[:2]
    scores = {}
    for a, (my, mx) in enumerate(moves):
        y, x = head[0] + my, head[1] + mx
        if not (0 <= y < h and 0 <= x < w) or any(o[y, x, ch] == 1 for ch in DEADLY):
            continue
        scores[a] = 0 if fruit is None else -(abs(y - fruit[0]) + abs(x - fruit[1]))
    return [a for a in sorted(scores) if scores[a] == max(scores.values())]


def one_snake(o, d, u):
    """o: (h, w, 8) uint8; d: (dy, dx) or None; u: the snake's random bits.
    Returns (action, direction or None, category bits)."""
    h, w = o.shape[:2]
    heads = cells_eq1(o[:, :, 5])
    if not heads:
        return 0, d, NOHEAD
    hy, hx = heads[0]
    fruits = cells_eq1(o[:, :, 1])
    dist = [abs(y - hy) + abs(x - hx) for y, x in fruits]
    nearest = [f for f, v in zip(fruits, dist) if v == min(dist)]
    if d is None:
        d = (-1, 0)
        for ny, nx in NEIGH:
            y, x = hy + ny, hx + nx
            if 0 <= y < h and 0 <= x < w and (o[y, x, 6] == 1 or o[y, x, 7] == 1):
                d = (hy - y, hx - x)
                break
    dy, dx = d
    moves = ((dy, dx), (-dx, dy), (dx, -dy))
    best = best_moves(o, (hy, hx), moves, nearest[0] if nearest else None)
    cat = 0 if fruits else NOFRUIT
    if len(nearest) > 1 and best_moves(o, (hy, hx), moves, nearest[-1]) != best:
        cat |= FRUIT_TIE
    if not best:
        return 0, moves[0], cat | ALLDEAD
    a = best[pick(u, len(best))]
    return a, moves[a], cat | (N1, N2, N3)[len(best) - 1]


def greedy_actions(obs, rnd, skip, dirs):
    """obs (N, S, h, w, 8) uint8; rnd (N, S) int32 or uint32, or None (zeros);
    skip (N, S) or None; dirs (N, S, 2) int8. Returns (actions int8 (N, S),
    dirs_out int8 (N, S, 2), category bits uint8 (N, S))."""
    N, S = obs.shape[:2]
    rnd = np.zeros((N, S), np.uint32) if rnd is None else np.ascontiguousarray(rnd).view(np.uint32).reshape(N, S)
    actions = np.zeros((N, S), np.int8)
    out = np.array(dirs, np.int8).reshape(N, S, 2).copy()
    cat = np.zeros((N, S), np.uint8)
    for n in range(N):
        for s in range(S):
            if skip is not None and skip[n, s]:
                cat[n, s] = SKIP
                continue
            d = None if (out[n, s] == UNKNOWN).all() else (int(out[n, s, 0]), int(out[n, s, 1]))
            a, nd, c = one_snake(obs[n, s], d, rnd[n, s])
            actions[n, s], cat[n, s] = a, c
            if nd is not None:
                out[n, s] = np.array(nd, np.int64).astype(np.int8)
    return actions, out, cat


def load_calls():
    """tests/golden/greedy_calls.npz (tests/golden/gen/make_greedy_golden.py) as
    {config: dict(obs (R, S, h, w, 8) uint8, rnd, skip, din, act, dout)}."""
    import golden_io
    z = golden_io.load('greedy_calls.npz')
    out = {}
    for name in sorted(k[:-6] for k in z.files if k.endswith('_shape')):
        S, h, w = (int(v) for v in z[name + '_shape'])
        d = {k: z[name + '_' + k] for k in ('rnd', 'skip', 'din', 'act', 'dout')}
        bits = np.unpackbits(z[name + '_obs'], axis=1)[:, :S * h * w * 8]
        d['obs'] = np.ascontiguousarray(bits.reshape(-1, S, h, w, 8))
        out[name] = d
    return out
