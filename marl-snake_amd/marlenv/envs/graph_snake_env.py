"""GraphSnakeEnv: the reference's single-env class behind 'SnakeGraph-v1'
(marlenv/marlenv/envs/graph_snake_env.py), backed by the HIP kernels.

The SnakeEnv of this package with the grid observation replaced by the graph
observation, exactly as the reference returns it: reset() and step() give the
live snakes' (5, C) feature rows in index order, cast to uint8 as the
reference's np.array(obs, dtype=np.uint8) casts them (which truncates: 0.5 +
0.33 is 0, 1 + 0.5 is 1), an array of shape (0,) when no snake is alive. The
rows come from k_graph_obs with source='reference' (marlenv/graph.py): the
reference indexes the observations with a counter of the live snakes, so a
live snake above a dead one reads another snake's observation, and so does
this class. `graph_rows` holds the float64 rows of the last call, before the
cast. observer='human' raises ValueError (at construction; the reference raises
it at the first reset()).
"""
import numpy as np

from ..graph import HUMAN_MESSAGE, GraphObs
from .snake_env import SnakeEnv


class GraphSnakeEnv(SnakeEnv):
    def __init__(self, *args, **kwargs):
        observer = args[6] if len(args) > 6 else kwargs.get('observer', 'snake')
        if observer != 'snake':
            raise ValueError(HUMAN_MESSAGE)
        super().__init__(*args, **kwargs)
        self._graph = GraphObs(self._vec, source='reference')
        self.graph_rows = None

    def _process_obs(self):
        """The graph rows of the observation the last reset/step left on the device."""
        rows = self._graph(self._obs_dev)[0].cpu().numpy()
        alive = self._graph.alive()[0].cpu().numpy()
        live = rows[alive]
        self.graph_rows = live if len(live) else np.zeros((0,), np.float64)
        return self.graph_rows.astype(np.uint8)

    def reset(self):
        super().reset()
        return self._process_obs()

    def step(self, actions):
        _, rews, dones, info = super().step(actions)
        return self._process_obs(), rews, dones, info
