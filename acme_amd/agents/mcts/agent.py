"""MCTS agent — drop-in for acme/agents/tf/mcts/agent.py:33-100: an MCTSActor planning on
`model` with the learner's policy-value network, and an AZLearner trained on the stored
transitions and search policies.  Same constructor; the replay table lives in GPU memory."""

from __future__ import annotations

import numpy as np

from acme_amd import datasets, replay, specs
from acme_amd.adders import reverb as adders
from acme_amd.agents import agent
from acme_amd.agents.mcts import acting, learning
from acme_amd.networks import PolicyValueMLP


class MCTS(agent.Agent):

    def __init__(self, network: PolicyValueMLP, model, optimizer, n_step: int, discount: float,
                 replay_capacity: int, num_simulations: int,
                 environment_spec: specs.EnvironmentSpec, batch_size: int, seed: int = 0):
        if not isinstance(network, PolicyValueMLP):
            raise ValueError("acme_amd's MCTS agent takes a networks.PolicyValueMLP, not a "
                             f"{type(network).__name__}")
        num_actions = environment_spec.actions.num_values
        if network.num_actions != num_actions:
            raise ValueError(f"the network has num_actions = {network.num_actions}, the "
                             f"environment spec {num_actions}")
        obs_dim = int(np.prod(environment_spec.observations.shape))
        if network.obs_dim != obs_dim:
            raise ValueError(f"the network has obs_dim = {network.obs_dim}, the environment "
                             f"spec's observations hold {obs_dim} values")
        extra_spec = {"pi": specs.Array((num_actions,), np.float32)}
        table = replay.Table(
            name=adders.DEFAULT_PRIORITY_TABLE, sampler=replay.selectors.Uniform(),
            remover=replay.selectors.Fifo(), max_size=replay_capacity,
            rate_limiter=replay.rate_limiters.MinSize(1),
            signature=adders.NStepTransitionAdder.signature(environment_spec, extra_spec),
            seed=1234 + seed)
        self._server = replay.Server([table], port=None)
        address = f"localhost:{self._server.port}"
        adder = adders.NStepTransitionAdder(client=replay.Client(address), n_step=n_step,
                                            discount=discount)
        dataset = datasets.make_reverb_dataset(server_address=address, batch_size=batch_size)
        learner = learning.AZLearner(network=network, optimizer=optimizer, dataset=dataset,
                                     discount=discount, batch_size=batch_size, seed=seed)
        actor = acting.MCTSActor(environment_spec=environment_spec, model=model, network=learner,
                                 discount=discount, adder=adder,
                                 num_simulations=num_simulations)
        super().__init__(actor=actor, learner=learner, min_observations=10,
                         observations_per_step=1)
