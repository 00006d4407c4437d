"""CPU checks of the genome heads (no GPU needed): the packer and the flat
program against the restated FeedForwardNetwork.activate (tests/genome_ref.py),
the host-only C calls (snake_genome_plan, snake_genome_check,
snake_genome_tiles), the names the packer accepts, from_linear's network, and
the host-side fitness mean."""
import ctypes
import math
import os

import numpy as np
import pytest

import genome_ref as R


@pytest.fixture(scope='module')
def native():
    from marlenv import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _native


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def test_flat_program_equals_activate(native):
    """200 random programs: the packed program, evaluated in numpy float64,
    equals activate() bit for bit on random float32 features, and the check call
    accepts it."""
    from marlenv import neat_head as H
    rs = np.random.RandomState(1)
    kinds = set()
    for case in range(200):
        I, A = int(rs.randint(1, 20)), int(rs.randint(1, 6))
        nets = [R.random_network(rs, I, A) for _ in range(int(rs.randint(1, 4)))]
        prog = H.pack(nets, I)
        cfg = H.program_cfg(prog, I)
        H.check_program(prog, cfg)
        assert (prog['link_src'] >= 0).all()
        x = R.random_features(rs, 3, I)
        for g, net in enumerate(nets):
            evaluated = {e[0] for e in net.node_evals}
            kinds.add('unevaluated output' if set(net.output_nodes) - evaluated else 'all outputs')
            kinds.add('no links' if any(not e[5] for e in net.node_evals) else 'links')
            kinds.add('from output' if any(s in net.output_nodes for e in net.node_evals for s, _ in e[5]) else 'plain')
            for row in x:
                want = net.activate([float(v) for v in row])
                got = R.eval_program(prog, I, g, row)
                assert bits(got).tolist() == bits(want).tolist(), (case, g)
                wb, _ = net.activate_bounded([float(v) for v in row])
                assert bits(wb).tolist() == bits(want).tolist()
    assert kinds == {'unevaluated output', 'all outputs', 'no links', 'links', 'from output', 'plain'}


def small_program():
    from marlenv import neat_head as H
    rs = np.random.RandomState(2)
    nets = [R.chain_network(rs, 4, 2, 3), R.chain_network(rs, 4, 2, 2)]
    prog = H.pack(nets, 4)
    return H, prog, H.program_cfg(prog, 4)


def test_check_accepts_and_rejects(native):
    H, prog, cfg = small_program()
    H.check_program(prog, cfg)

    def rejected(field, name, index, value):
        bad = {k: v.copy() for k, v in prog.items()}
        bad[name].reshape(-1)[index] = value
        with pytest.raises(ValueError, match=field):
            H.check_program(bad, cfg)

    # genome 0: nodes at slots 4 .. 8; its second node (slot 5) has three links, the middle one from slot 4
    l = int(prog['link_off'][1]) + 1
    assert prog['link_src'][l] == 4
    rejected('link_src', 'link_src', l, 5)              # its own slot: not below
    rejected('link_src', 'link_src', l, 6)              # forward
    rejected('link_src', 'link_src', 0, -1)
    rejected('link_off', 'link_off', 2, int(prog['link_off'][3]) + 1)   # not monotone
    rejected('node_off', 'node_off', 1, int(prog['node_off'][2]) + 1)
    rejected('node_off', 'node_off', 2, int(prog['node_off'][2]) - 1)   # does not end at num_nodes
    rejected('node_act', 'node_act', 3, 3)
    rejected('node_act', 'node_act', 0, -1)
    n0 = int(prog['node_off'][1]) - int(prog['node_off'][0])
    rejected('out_slot', 'out_slot', 0, 4 + n0)         # past genome 0's nodes
    rejected('out_slot', 'out_slot', 1, -2)
    bad_cfg = H.program_cfg(prog, 4)
    bad_cfg.max_nodes += 1
    with pytest.raises(ValueError, match='max_nodes'):
        H.check_program(prog, bad_cfg)


@pytest.mark.parametrize('field,value', [('num_inputs', 0), ('num_inputs', 1025), ('num_outputs', 0),
                                         ('num_outputs', 17), ('num_genomes', 0)])
def test_plan_rejects(native, field, value):
    c = native.GenomeCfg(128, 3, 2, 5, 8, 20)
    L, lay = native.lib(), native.GenomeLayout()
    assert L.snake_genome_plan(ctypes.byref(c), 1024, ctypes.byref(lay)) == 0
    setattr(c, field, value)
    rc = L.snake_genome_plan(ctypes.byref(c), 1024, ctypes.byref(lay))
    assert rc == -1 and field in L.snake_last_error().decode()
    with pytest.raises(ValueError):
        native.check(rc)


def test_plan_sizes(native):
    """The LDS carve: 64 rows per tile while 65 floats per input fit 40 KB, node
    values in the rest of 64 KB, and a scratch slice per possible tile only when
    the largest genome does not fit."""
    L, lay = native.lib(), native.GenomeLayout()
    c = native.GenomeCfg(128, 3, 100, 40, 2000, 9000)
    assert L.snake_genome_plan(ctypes.byref(c), 400, ctypes.byref(lay)) == 0
    assert (lay.tile_rows, lay.lds_nodes, lay.scratch) == (64, (65536 - 128 * 65 * 4) // 512, 0)
    assert lay.lds_bytes == 128 * 65 * 4 + 40 * 512 and lay.max_tiles == 7 + 100
    c.max_nodes = lay.lds_nodes + 1
    assert L.snake_genome_plan(ctypes.byref(c), 400, ctypes.byref(lay)) == 0
    assert lay.scratch == 107 * 64 * 512 and lay.lds_bytes <= 65536
    c = native.GenomeCfg(1024, 16, 1, 10, 10, 10)
    assert L.snake_genome_plan(ctypes.byref(c), 64, ctypes.byref(lay)) == 0
    assert lay.tile_rows == 8 and lay.lds_bytes <= 65536 and lay.max_tiles == 9


def test_tiles_group_rows_by_genome(native):
    from marlenv import neat_head as H
    rs = np.random.RandomState(3)
    nets = [R.random_network(rs, 6, 2) for _ in range(5)]
    g = [3, 0, 3, 1, 1, 3, 0, 4] * 30         # unsorted, repeating, genome 2 unused
    heads = H.GenomeHeads(nets, num_inputs=6, genome_of_env=g)
    lay, tiles, rows = heads.tiles(3)
    assert sorted(rows.tolist()) == list(range(len(g) * 3))
    assert len(tiles) <= lay.max_tiles
    at = 0
    for genome, count, start, scratch in tiles.tolist():
        assert start == at and 1 <= count <= lay.tile_rows and scratch == -1
        assert {g[r // 3] for r in rows[start:start + count].tolist()} == {genome}
        at += count
    assert at == rows.size
    for genome in range(5):         # the envs of a genome keep their order
        mine = [r for r in rows.tolist() if g[r // 3] == genome]
        assert mine == sorted(mine)
    with pytest.raises(ValueError):
        H.GenomeHeads(nets, num_inputs=6, genome_of_env=[0, 5])


def test_unknown_names_raise(native):
    from marlenv import neat_head as H

    def softplus_activation(z):
        return z

    def max_aggregation(x):
        return max(x)

    ok = (0, R.relu_activation, R.sum_aggregation, 0.0, 1.0, [(-1, 1.0)])
    H.pack([R.Network([-1], [0], [ok])], 1)
    H.pack([R.Network([-1], [0], [(0, 'tanh', 'sum', 0.0, 1.0, [(-1, 1.0)])])], 1)
    with pytest.raises(ValueError, match='softplus_activation'):
        H.pack([R.Network([-1], [0], [(0, softplus_activation, R.sum_aggregation, 0.0, 1.0, [(-1, 1.0)])])], 1)
    with pytest.raises(ValueError, match='max_aggregation'):
        H.pack([R.Network([-1], [0], [(0, R.relu_activation, max_aggregation, 0.0, 1.0, [(-1, 1.0)])])], 1)
    with pytest.raises(ValueError, match='no value'):
        H.pack([R.Network([-1], [0], [(0, 'relu', 'sum', 0.0, 1.0, [(7, 1.0)])])], 1)
    with pytest.raises(ValueError, match='inputs'):
        H.pack([R.Network([-1], [0], [ok])], 2)


def test_from_linear(native):
    from marlenv import GenomeHeads
    rs = np.random.RandomState(4)
    W, b = rs.randn(3, 128).astype(np.float32), rs.randn(3).astype(np.float32)
    heads = GenomeHeads.from_linear(W, b, num_envs=5)
    p = heads.program
    assert heads.num_inputs == 128 and heads.num_outputs == 3 and heads.num_genomes == 1 and heads.num_envs == 5
    assert p['node_off'].tolist() == [0, 3] and p['link_off'].tolist() == [0, 128, 256, 384]
    assert p['node_act'].tolist() == [0, 0, 0] and p['node_resp'].tolist() == [1.0, 1.0, 1.0]
    assert p['link_src'].tolist() == list(range(128)) * 3
    assert bits(p['link_w']).tolist() == bits(W.astype(np.float64).reshape(-1)).tolist()
    assert bits(p['node_bias']).tolist() == bits(b.astype(np.float64)).tolist()
    assert p['out_slot'].tolist() == [[128, 129, 130]]
    x = R.random_features(rs, 1, 128)[0]
    want = []
    for o in range(3):
        s = 0.0
        for i in range(128):
            s = s + float(x[i]) * float(W[o, i])
        z = float(b[o]) + s
        want.append(z if z > 0.0 else 0.0)
    assert bits(R.eval_program(p, 128, 0, x)).tolist() == bits(want).tolist()
    assert GenomeHeads.from_linear(W, b, activation='tanh').program['node_act'].tolist() == [2, 2, 2]


def test_real_neat_network_equals_stand_in():
    """Where neat-python is installed: its FeedForwardNetwork.activate equals the
    stand-in's on hand-built networks, and its functions carry the names the
    packer recognises."""
    neat = pytest.importorskip('neat')
    from neat.activations import relu_activation, sigmoid_activation, tanh_activation
    from neat.aggregations import sum_aggregation
    from marlenv import neat_head as H
    real = {R.relu_activation: relu_activation, R.sigmoid_activation: sigmoid_activation,
            R.tanh_activation: tanh_activation}
    rs = np.random.RandomState(5)
    for _ in range(20):
        mine = R.random_network(rs, 7, 3)
        evals = [(n, real[a], sum_aggregation, b, r, l) for n, a, _, b, r, l in mine.node_evals]
        theirs = neat.nn.FeedForwardNetwork(mine.input_nodes, mine.output_nodes, evals)
        for row in R.random_features(rs, 4, 7):
            x = [float(v) for v in row]
            assert bits(theirs.activate(x)).tolist() == bits(mine.activate(x)).tolist()
        assert H.pack([theirs], 7)['node_act'].tolist() == H.pack([mine], 7)['node_act'].tolist()


@pytest.mark.parametrize('S', [1, 4, 8, 16])
def test_fitness_is_numpy_mean(native, S):
    """evaluate_population's fitness is np.mean of a row of R: the reference's
    float(R.mean()) on its own (S,) float64 array, pairwise order and all."""
    from marlenv import neat_head as H
    rs = np.random.RandomState(6)
    R_ = rs.uniform(-50, 50, size=(7, S)) * 10.0 ** rs.randint(-3, 4, size=(7, S))
    got = H.population_fitness(R_, np.array([0, 1, 1, 2, 0, 1, 4]), 5)
    for i in range(7):
        assert bits(got[0][i]) == bits(float(R_[i].copy().mean()))
    assert bits(got[1][1]) == bits(np.mean(got[0][[1, 2, 5]]))
    assert math.isnan(got[1][3]) and not np.isnan(got[1][[0, 1, 2, 4]]).any()
