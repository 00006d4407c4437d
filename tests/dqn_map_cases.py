"""Case tables of the map path's exact tests (tests/test_dqn_map_exact.py on the
GPU, tests/test_dqn_map_cpu.py proving the same probes valid on the CPU). The
probes themselves are tests/dqn_probe.py's, recipe unchanged."""
import dqn_probe as dp

SEEDS = dp.SEEDS
GRID_B = 37          # no multiple of 16: a partly filled fc row tile
# (h, w, c): the largest image and the most planes (22x22, 20x20 at 8 and 32
# channels), rectangular maps with 9 (12x10, 4x33 = the widest strip, 21x5 = 8)
# row tiles and every channel padding, 13x13 (the first size past the window
# path), and maps of one row tile, fewer tiles than waves (11x11 has 8)
GRID = ((20, 20, 8), (20, 20, 32), (22, 22, 8), (22, 22, 32),
        (12, 10, 8), (4, 33, 16), (21, 5, 24), (13, 13, 16),
        (11, 11, 8), (3, 3, 8), (1, 7, 8))
TAIL_GEO = (20, 20, 8)
TAIL_B = (1, 255, 257)              # prefixes of one 257-row probe
PERSIST = ((20, 20, 8), (22, 22, 32))
PERSIST_UNIQUE = 64
ACTIONS_GEO = (12, 10, 8)
ACTIONS = (1, 4)
SHARP_GEO = ((20, 20, 8), (12, 10, 8))

PLAN_ACCEPTS = ((20, 20, 8), (22, 22, 32), (12, 10, 8), (4, 33, 16), (21, 5, 24), (1, 7, 8), (3, 3, 8), (11, 11, 8))
# (h, w, c, num_actions): what snake_dqn_map_plan must reject
PLAN_REJECTS = ((40, 40, 8, 3), (20, 20, 12, 3), (20, 20, 40, 3), (20, 20, 8, 5), (0, 7, 8, 3), (23, 22, 8, 3))


def probe_keys():
    """Every (h, w, c, num_actions, seed, B) probe the GPU file runs."""
    keys = [g + (3, seed, GRID_B) for g in GRID for seed in SEEDS]
    keys.append(TAIL_GEO + (3, 0, max(TAIL_B)))
    keys += [ACTIONS_GEO + (a, seed, GRID_B) for a in ACTIONS for seed in SEEDS]
    keys += [g + (3, 0, PERSIST_UNIQUE) for g in PERSIST]
    return keys
