"""MCTSActor — drop-in for acme/agents/tf/mcts/acting.py:35-121: every action comes from a
fresh policy- and value-guided tree search on the model; the search's visit distribution is
the policy that is sampled and stored beside the transition as extras['pi'].

`network` is anything with `evaluate(observation) -> (probs, value)` (the AZLearner, whose
evaluation is one native launch on its current parameters) or a callable of that signature.
The reference's variable client is out of scope: the actor reads the learner's
parameters in place."""

from __future__ import annotations

import numpy as np

from acme_amd import core, specs
from acme_amd.agents.mcts import search


class MCTSActor(core.Actor):

    def __init__(self, environment_spec: specs.EnvironmentSpec, model, network, discount: float,
                 num_simulations: int, adder=None, variable_client=None):
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

    def _forward(self, observation):
        probs, value = self._evaluate(observation)
        return np.asarray(probs), float(value)

    def select_action(self, observation):
        if self._model.needs_reset:
            self._model.reset(observation)
        root = search.mcts(observation, model=self._model, search_policy=search.puct,
                           evaluation=self._forward, num_simulations=self._num_simulations,
                           num_actions=self._num_actions, discount=self._discount)
        probs = search.visit_count_policy(root)
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
