"""A restatement of neat.nn.FeedForwardNetwork for the genome-head tests:
neat-python's activate() loop written out with Python floats, its three
activations and the sum aggregation under neat-python's names, a seeded
generator of random feed-forward programs, and a forward error bound carried
along with every value.

The bound is derived, not measured. An input has bound 0. A relu node whose
sources all have bound 0 has bound 0: the device does the same IEEE operations
in the same order, so it must match bit for bit. Otherwise, for a node with k
links, sources v_i +- e_i, weights w_i, bias b and response r,

    e = L * (|r| * sum |w_i| e_i  +  2^-52 (k + 2) (|b| + |r| sum |w_i v_i|))  +  t

The first term carries the sources' errors through the sum; the second allows
one rounding per product, add, response multiply and bias add on either side
(2^-52 = 2 * 2^-53); L is the Lipschitz constant of the clamped activation in
its argument (relu 1, sigmoid 5/4, tanh 5/2); t is 4 ulp of the node's value for
sigmoid and tanh -- 1 ulp for the device library's exp / tanh, up to 2 for the
host libm, 1 for the rounding of the division or the result -- and 0 for relu.
"""
import math

import numpy as np

EPS = 2.0 ** -52


def relu_activation(z):
    return z if z > 0.0 else 0.0


def sigmoid_activation(z):
    z = max(-60.0, min(60.0, 5.0 * z))
    return 1.0 / (1.0 + math.exp(-z))


def tanh_activation(z):
    z = max(-60.0, min(60.0, 2.5 * z))
    return math.tanh(z)


def sum_aggregation(x):
    s = 0.0
    for v in x:         # left to right from +0.0 (the builtin sum of neat-python, before Python 3.12 made it compensated)
        s = s + v
    return s


ACTS = (relu_activation, sigmoid_activation, tanh_activation)
LIPSCHITZ = {relu_activation: 1.0, sigmoid_activation: 1.25, tanh_activation: 2.5}


class Network:
    """neat.nn.FeedForwardNetwork: the same three attributes and activate()."""

    def __init__(self, inputs, outputs, node_evals):
        self.input_nodes = list(inputs)
        self.output_nodes = list(outputs)
        self.node_evals = list(node_evals)

    def activate(self, inputs):
        if len(self.input_nodes) != len(inputs):
            raise RuntimeError('Expected {0:n} inputs, got {1:n}'.format(len(self.input_nodes), len(inputs)))
        values = dict((key, 0.0) for key in self.input_nodes + self.output_nodes)
        for k, v in zip(self.input_nodes, inputs):
            values[k] = v
        for node, act_func, agg_func, bias, response, links in self.node_evals:
            node_inputs = []
            for i, w in links:
                node_inputs.append(values[i] * w)
            s = agg_func(node_inputs)
            values[node] = act_func(bias + response * s)
        return [values[i] for i in self.output_nodes]

    def activate_bounded(self, inputs):
        """(outputs, bounds): activate() with the module docstring's error bound
        carried along. inputs: Python floats."""
        values = dict((key, 0.0) for key in self.input_nodes + self.output_nodes)
        err = dict((key, 0.0) for key in values)
        for k, v in zip(self.input_nodes, inputs):
            values[k] = v
        for node, act_func, agg_func, bias, response, links in self.node_evals:
            s, carried, mag = 0.0, 0.0, 0.0
            for i, w in links:
                s = s + values[i] * w
                carried += abs(w) * err[i]
                mag += abs(w * values[i])
            v = act_func(bias + response * s)
            if act_func is relu_activation and carried == 0.0:
                e = 0.0
            else:
                e = LIPSCHITZ[act_func] * (abs(response) * carried
                                           + EPS * (len(links) + 2) * (abs(bias) + abs(response) * mag))
                if act_func is not relu_activation:
                    e += 4.0 * math.ulp(v)
            values[node], err[node] = v, e
        return [values[i] for i in self.output_nodes], [err[i] for i in self.output_nodes]


def random_network(rs, num_inputs, num_outputs, hidden=None, acts=ACTS, max_links=8):
    """A random feed-forward program: `hidden` hidden nodes (default 0..12) and
    most of the outputs in a random evaluation order, each reading up to
    max_links of the inputs and the nodes before it; weights, biases and
    responses in [-3, 3]. Outputs are read by later nodes like any other node,
    about a tenth of the links leave an output that has not been evaluated yet
    (it reads 0.0), about a tenth of the nodes have no links, and about a fifth
    of the outputs are never evaluated."""
    inputs = [-i - 1 for i in range(num_inputs)]
    outputs = list(range(num_outputs))
    if hidden is None:
        hidden = int(rs.randint(0, 13))
    order = [num_outputs + i for i in range(hidden)] + [o for o in outputs if rs.rand() < 0.8]
    order = [order[i] for i in rs.permutation(len(order))]
    evals, seen = [], []
    for node in order:
        avail = inputs + seen
        pending = [o for o in outputs if o not in seen and o != node]
        links = []
        if rs.rand() >= 0.1:
            k = int(rs.randint(1, min(len(avail), max_links) + 1))
            for j in rs.choice(len(avail), k, replace=False):
                src = avail[int(j)]
                if pending and rs.rand() < 0.1:
                    src = pending[int(rs.randint(len(pending)))]
                links.append((src, float(rs.uniform(-3, 3))))
        evals.append((node, acts[int(rs.randint(len(acts)))], sum_aggregation, float(rs.uniform(-3, 3)),
                      float(rs.uniform(-3, 3)), links))
        seen.append(node)
    return Network(inputs, outputs, evals)


def chain_network(rs, num_inputs, num_outputs, depth, acts=ACTS):
    """inputs -> h_1 -> ... -> h_depth -> every output: each hidden node reads
    the one before it and two inputs."""
    inputs = [-i - 1 for i in range(num_inputs)]
    outputs = list(range(num_outputs))
    evals, prev = [], None
    for d in range(depth):
        links = [(inputs[int(rs.randint(num_inputs))], float(rs.uniform(-3, 3))) for _ in range(2)]
        if prev is not None:
            links.insert(1, (prev, float(rs.uniform(-3, 3))))
        prev = num_outputs + d
        evals.append((prev, acts[int(rs.randint(len(acts)))], sum_aggregation, float(rs.uniform(-1, 1)),
                      float(rs.uniform(-3, 3)), links))
    for o in outputs:
        evals.append((o, acts[int(rs.randint(len(acts)))], sum_aggregation, float(rs.uniform(-1, 1)),
                      float(rs.uniform(-3, 3)), [(prev, float(rs.uniform(-3, 3))), (inputs[0], 0.5)]))
    return Network(inputs, outputs, evals)


def random_features(rs, rows, num_inputs):
    """float32 features with negative values and exact zeros."""
    x = (rs.randn(rows, num_inputs) * 2).astype(np.float32)
    x[rs.rand(rows, num_inputs) < 0.3] = 0.0
    return x


def eval_program(prog, num_inputs, genome, x):
    """The packed program (marlenv.neat_head.pack) of one genome on one feature
    row x, in numpy float64 scalars: the second restatement, of the flat form."""
    I = num_inputs
    n0, n1 = int(prog['node_off'][genome]), int(prog['node_off'][genome + 1])
    vals = np.zeros(I + n1 - n0, np.float64)
    vals[:I] = np.asarray(x, np.float32).astype(np.float64)
    for n in range(n0, n1):
        s = np.float64(0.0)
        for l in range(int(prog['link_off'][n]), int(prog['link_off'][n + 1])):
            s = s + vals[prog['link_src'][l]] * prog['link_w'][l]
        z = prog['node_bias'][n] + prog['node_resp'][n] * s
        act = int(prog['node_act'][n])
        if act == 0:
            v = z if z > 0.0 else np.float64(0.0)
        elif act == 1:
            z = max(-60.0, min(60.0, 5.0 * z))
            v = 1.0 / (1.0 + math.exp(-z))
        else:
            z = max(-60.0, min(60.0, 2.5 * z))
            v = math.tanh(z)
        vals[I + n - n0] = v
    return np.array([vals[s] if s >= 0 else 0.0 for s in prog['out_slot'][genome]], np.float64)


def reference(networks, genome_of_env, features, num_snakes, skip=None):
    """activate_bounded for every row: (outputs (N, S, A), bounds (N, S, A),
    actions (N, S) int8 = first maximum, 0 where skip)."""
    N, S = len(genome_of_env), num_snakes
    A = len(networks[0].output_nodes)
    x = np.asarray(features, np.float32).reshape(N, S, -1)
    out, err = np.zeros((N, S, A)), np.zeros((N, S, A))
    for n in range(N):
        for s in range(S):
            out[n, s], err[n, s] = networks[genome_of_env[n]].activate_bounded([float(v) for v in x[n, s]])
    act = np.argmax(out, axis=-1).astype(np.int8)
    if skip is not None:
        act[np.asarray(skip).reshape(N, S) != 0] = 0
    return out, err, act
