"""MCTSActor — drop-in for acme/agents/tf/mcts/acting.py:35-121: every action comes from a
fresh policy- and value-guided tree search on the model; the search's visit distribution is
the policy that is sampled and stored beside the transition as extras['pi'].

`network` is anything with `evaluate(observation) -> (probs, value)` (the AZLearner, whose
evaluation is one native launch on its current parameters) or a callable of that signature.
The reference's variable client is out of scope: the actor reads the learner's
parameters in place.

search="host" (the default) builds the tree in Python with search.mcts.  search="native" runs
the whole search in one launch (acme_mcts_search_run) on the model's current state buffer and
copies one packed row back; it needs a models.MLPModel and a network exposing its NativeAZ as
`native` (the AZLearner), both on one device.  Ties of the PUCT maximum are then broken by
Philox on (seed, the actor's call count) and not by numpy's global state."""

from __future__ import annotations

import numpy as np

from acme_amd import core, specs
from acme_amd.agents.mcts import search
from acme_amd.agents.mcts.models.mlp import MLPModel
from acme_amd.native import NativeAZ, NativeMCTSSearch


class MCTSActor(core.Actor):

    def __init__(self, environment_spec: specs.EnvironmentSpec, model, network, discount: float,
                 num_simulations: int, adder=None, variable_client=None, search: str = "host",
                 seed: int = 0):
        if variable_client is not None:
            raise ValueError("acme_amd's MCTSActor does not support variable_client: it must "
                             "be None")
        evaluate = getattr(network, "evaluate", None) or network
        if not callable(evaluate):
            raise ValueError("network must have an evaluate(observation) method or be callable")
        self._evaluate = evaluate
        self._model = model
        self._adder = adder
        self._num_actions = environment_spec.actions.num_values
        self._num_simulations = num_simulations
        self._actions = list(range(self._num_actions))
        self._discount = discount
        # The search policy of the last action, stored with its transition in observe().
        self._probs = np.ones((self._num_actions,), np.float32) / self._num_actions
        self._prev_timestep = None
        if search not in ("host", "native"):
            raise ValueError(f"search must be 'host' or 'native', got {search!r}")
        self._native_search = None
        if search == "native":
            if not isinstance(model, MLPModel):
                raise ValueError("search='native' plans on a models.MLPModel (the learned model "
                                 f"on the device), not on a {type(model).__name__}")
            az = getattr(network, "native", None)
            if not isinstance(az, NativeAZ):
                raise ValueError("search='native' needs a network that exposes its NativeAZ as "
                                 "`native` (the AZLearner), not a "
                                 f"{type(network).__name__}")
            self._native_search = NativeMCTSSearch(az, model.native, num_simulations)
            self._seed, self._calls = int(seed), 0

    def _forward(self, observation):
        probs, value = self._evaluate(observation)
        return np.asarray(probs), float(value)

    def select_action(self, observation):
        if self._model.needs_reset:
            self._model.reset(observation)
        if self._native_search is not None:
            return self._act(self._search_native())
        root = search.mcts(observation, model=self._model, search_policy=search.puct,
                           evaluation=self._forward, num_simulations=self._num_simulations,
                           num_actions=self._num_actions, discount=self._discount)
        return self._act(search.visit_count_policy(root))

    def _search_native(self):
        """One launch on the model's current state, one blocking copy of the packed row."""
        model, n = self._model, self._native_search
        row = n.run(model.state_row, self._num_simulations, self._discount,
                    sigmoid=model.sigmoid_discount, terminal_tol=model.terminal_tol,
                    seed=self._seed, call_counter=self._calls).cpu().numpy()
        self._calls += 1
        out = n.unpack(row)
        if out["status"]:
            raise ValueError("check_numerics failed: NaN or Inf in a PUCT score of the device "
                             "search")
        return search.visits_policy(out["visits"])

    def _act(self, probs):
        action = np.int32(np.random.choice(self._actions, p=probs))
        self._probs = probs.astype(np.float32)
        return action

    def update(self):
        """Nothing to fetch: the evaluation reads the learner's parameters."""

    def observe_first(self, timestep):
        self._prev_timestep = timestep
        if self._adder:
            self._adder.add_first(timestep)

    def observe(self, action, next_timestep):
        self._model.update(self._prev_timestep, action, next_timestep)
        self._prev_timestep = next_timestep
        if self._adder:
            self._adder.add(action, next_timestep, extras={"pi": self._probs})
