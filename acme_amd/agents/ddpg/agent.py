"""DDPG agent — drop-in for acme/agents/tf/ddpg/agent.py:37-160.

Same constructor (environment_spec, policy_network, critic_network,
observation_network=identity, discount=0.99, batch_size=256, prefetch_size=4,
target_update_period=100, min_replay_size=1000, max_replay_size=1e6,
samples_per_insert=32.0, n_step=5, sigma=0.3, clipping=True, logger=None, counter=None,
checkpoint=True, replay_table_name).  Uniform GPU replay table instead of a Reverb server;
the behaviour policy is the learner's online policy + ClippedGaussian(sigma) + ClipToSpec
(agent.py:129-135), the one D4PG uses."""

from __future__ import annotations

import copy

from acme_amd import specs
from acme_amd.adders import reverb as adders
from acme_amd.agents import agent
from acme_amd.agents.actors import FeedForwardActor
from acme_amd.agents.d4pg.agent import GaussianBehaviourPolicy, make_transition_replay
from acme_amd.agents.ddpg import learning


class DDPG(agent.Agent):

    def __init__(self, environment_spec: specs.EnvironmentSpec, policy_network, critic_network,
                 observation_network="identity", discount: float = 0.99, batch_size: int = 256,
                 prefetch_size: int = 4, target_update_period: int = 100,
                 min_replay_size: int = 1000, max_replay_size: int = 1000000,
                 samples_per_insert: float = 32.0, n_step: int = 5, sigma: float = 0.3,
                 clipping: bool = True, logger=None, counter=None, checkpoint: bool = True,
                 replay_table_name: str = adders.DEFAULT_PRIORITY_TABLE, seed: int = 0):
        self._server, adder, dataset = make_transition_replay(
            environment_spec, replay_table_name, max_replay_size, n_step, discount, batch_size,
            prefetch_size, seed)
        learner = learning.DDPGLearner(
            policy_network=policy_network, critic_network=critic_network,
            target_policy_network=copy.deepcopy(policy_network),
            target_critic_network=copy.deepcopy(critic_network),
            observation_network=observation_network,
            target_observation_network=observation_network,
            clipping=clipping, discount=discount, target_update_period=target_update_period,
            dataset=dataset, counter=counter, logger=logger, checkpoint=checkpoint,
            batch_size=batch_size, seed=seed)
        acts = environment_spec.actions
        behaviour = GaussianBehaviourPolicy(learner.policy, sigma, acts.minimum, acts.maximum,
                                            seed=seed)
        actor = FeedForwardActor(behaviour, adder)
        super().__init__(actor=actor, learner=learner,
                         min_observations=max(batch_size, min_replay_size),
                         observations_per_step=float(batch_size) / samples_per_insert)
