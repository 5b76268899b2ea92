"""R2D2 agent — drop-in for acme/agents/tf/r2d2/agent.py:36-160.

Same constructor (environment_spec, network, burn_in_length, trace_length, replay_period,
counter=None, logger=None, discount=0.99, batch_size=32, prefetch_size=None,
target_update_period=100, importance_sampling_exponent=0.2, priority_exponent=0.6,
epsilon=0.01, learning_rate=1e-3, min_replay_size=1000, max_replay_size=1e6,
samples_per_insert=32.0, store_lstm_state=True, max_priority_weight=0.9, checkpoint=True).
The prioritized sequence table lives in GPU memory (agents/r2d2/make_replay); the actor is a
RecurrentActor whose policy is one acme_r2d2_q_step per environment step on the learner's
online network (the TF agent shares the network object between actor and learner): the core
state stays on the device, the epsilon-greedy action is selected there from the q row, and
the state that went into each step is stored as extras['core_state']."""

from __future__ import annotations

import copy
import os
from typing import Optional

import numpy as np

from acme_amd import replay, specs
from acme_amd.agents import agent
from acme_amd.agents.actors import RecurrentActor
from acme_amd.agents.r2d2.learning import R2D2Learner
from acme_amd.networks import LSTMState
from acme_amd.utils import savers


def core_state_spec(network):
    """The extras an R2D2 actor stores with every step: the core state that went into it."""
    H = network.lstm_size
    return {"core_state": LSTMState(specs.Array((H,), np.float32),
                                    specs.Array((H,), np.float32))}


class RecurrentReplayAgent(agent.Agent):
    """What R2D2 and R2D3 share once their replay stands: the R2D2 learner on `dataset`, its
    checkpointer, the epsilon-greedy policy on the learner's online network, a RecurrentActor
    writing to `adder`, and the agent's observation arithmetic.  `learner_kwargs` go to
    R2D2Learner as they are."""

    def _finish(self, server, adder, dataset, *, environment_spec, network, target_network,
                burn_in_length: int, trace_length: int, replay_period: int, batch_size: int,
                min_replay_size: int, samples_per_insert: float, epsilon: float,
                checkpoint: bool, checkpoint_subpath: str, seed: int, **learner_kwargs):
        self._server = server
        learner = R2D2Learner(
            environment_spec=environment_spec, network=network,
            target_network=copy.deepcopy(network) if target_network is None else target_network,
            burn_in_length=burn_in_length,
            sequence_length=burn_in_length + trace_length + 1, dataset=dataset,
            reverb_client=replay.Client(server), batch_size=batch_size, seed=seed,
            **learner_kwargs)
        self._checkpointer = None
        if checkpoint:
            self._checkpointer = savers.Checkpointer(
                objects_to_save={"learner": learner},
                directory=os.path.join(os.path.expanduser(checkpoint_subpath), "r2d2_learner"),
                time_delta_minutes=60.0)
        self._learner_obj = learner
        self._policy = learner.make_policy(epsilon, seed)
        # The actor stores its core state whatever store_lstm_state says (the table's
        # signature has it; the learner ignores it then), as the reference's.
        actor = RecurrentActor(self._policy, network.initial_state, adder)
        observations_per_step = float(replay_period * batch_size) / samples_per_insert
        super().__init__(actor=actor, learner=learner,
                         min_observations=replay_period * max(batch_size, min_replay_size),
                         observations_per_step=observations_per_step)

    @property
    def learner(self) -> R2D2Learner:
        return self._learner_obj

    @property
    def policy(self):
        """The actor's policy (its seed and call counter replay its draws)."""
        return self._policy

    @property
    def server(self):
        return self._server

    def update(self):
        super().update()
        if self._checkpointer is not None:
            self._checkpointer.save()


class R2D2(RecurrentReplayAgent):

    def __init__(self, environment_spec: specs.EnvironmentSpec, network, burn_in_length: int,
                 trace_length: int, replay_period: int, counter=None, logger=None,
                 discount: float = 0.99, batch_size: int = 32,
                 prefetch_size: Optional[int] = None, target_update_period: int = 100,
                 importance_sampling_exponent: float = 0.2, priority_exponent: float = 0.6,
                 epsilon: float = 0.01, learning_rate: float = 1e-3,
                 min_replay_size: int = 1000, max_replay_size: int = 1_000_000,
                 samples_per_insert: float = 32.0, store_lstm_state: bool = True,
                 max_priority_weight: float = 0.9, checkpoint: bool = True,
                 checkpoint_subpath: str = "~/acme/", seed: int = 0):
        from acme_amd.agents.r2d2 import make_replay
        replay_parts = make_replay(
            environment_spec, core_state_spec(network), burn_in_length, trace_length,
            replay_period, batch_size=batch_size, max_replay_size=max_replay_size,
            priority_exponent=priority_exponent, prefetch_size=prefetch_size, seed=1234 + seed)
        self._finish(
            *replay_parts, environment_spec=environment_spec, network=network,
            target_network=None, burn_in_length=burn_in_length, trace_length=trace_length,
            replay_period=replay_period, batch_size=batch_size, min_replay_size=min_replay_size,
            samples_per_insert=samples_per_insert, epsilon=epsilon, checkpoint=checkpoint,
            checkpoint_subpath=checkpoint_subpath, seed=seed, counter=counter, logger=logger,
            discount=discount, target_update_period=target_update_period,
            importance_sampling_exponent=importance_sampling_exponent,
            max_replay_size=max_replay_size, learning_rate=learning_rate,
            store_lstm_state=store_lstm_state, max_priority_weight=max_priority_weight)
