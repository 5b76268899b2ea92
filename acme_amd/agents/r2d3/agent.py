"""R2D3 agent — drop-in for acme/agents/tf/r2d3/agent.py:38-160.

Same constructor (environment_spec, network, target_network, burn_in_length, trace_length,
replay_period, demonstration_dataset, demonstration_ratio, counter=None, logger=None,
discount=0.99, batch_size=32, target_update_period=100, importance_sampling_exponent=0.2,
epsilon=0.01, learning_rate=1e-3, checkpoint=True, min_replay_size=1000, max_replay_size=1e6,
samples_per_insert=32.0), plus `seed`; target_network may be None (a copy of `network`) and
the arguments after it are passed by keyword, as the reference's callers pass them.  A
single-process R2D2 agent whose every batch mixes demonstration sequences with the actor's
experience: a Uniform + Fifo sequence table (agent.py:74-81), the SequenceAdder, the table's
dataset with the demonstrations mixed in on the GPU (acme_amd.datasets.demonstrations,
csrc/demos.hip), the R2D2 learner with store_lstm_state=False (a demonstration has no
core state: its extras are zeros, so every sequence is burnt in from a zero state) and a
RecurrentActor on the learner's online network.

`demonstration_dataset` is a SequenceDemonstrationStore or the iterable of (observations,
actions, rewards, discounts) episodes one is built from
(DemonstrationRecorder.make_dataset()); observations are the environment's (an OAR)."""

from __future__ import annotations

from acme_amd import datasets, replay, specs
from acme_amd.adders import reverb as adders
from acme_amd.agents.r2d2.agent import RecurrentReplayAgent, core_state_spec
from acme_amd.datasets import demonstrations


class R2D3(RecurrentReplayAgent):

    def __init__(self, environment_spec: specs.EnvironmentSpec, network, target_network=None,
                 *, burn_in_length: int, trace_length: int, replay_period: int,
                 demonstration_dataset, demonstration_ratio: float, counter=None, logger=None,
                 discount: float = 0.99, batch_size: int = 32, target_update_period: int = 100,
                 importance_sampling_exponent: float = 0.2, epsilon: float = 0.01,
                 learning_rate: float = 1e-3, checkpoint: bool = True,
                 min_replay_size: int = 1000, max_replay_size: int = 1_000_000,
                 samples_per_insert: float = 32.0, checkpoint_subpath: str = "~/acme/",
                 seed: int = 0):
        table = replay.Table(
            name=adders.DEFAULT_PRIORITY_TABLE, sampler=replay.selectors.Uniform(),
            remover=replay.selectors.Fifo(), max_size=max_replay_size,
            rate_limiter=replay.rate_limiters.MinSize(1),
            signature=adders.SequenceAdder.signature(environment_spec,
                                                     core_state_spec(network)),
            seed=1234 + seed)
        server = replay.Server([table], port=None)
        sequence_length = burn_in_length + trace_length + 1
        adder = adders.SequenceAdder(client=replay.Client(server), period=replay_period,
                                     sequence_length=sequence_length)
        store = demonstration_dataset
        if not isinstance(store, demonstrations.SequenceDemonstrationStore):
            store = demonstrations.SequenceDemonstrationStore(store, table)
        dataset = datasets.make_reverb_dataset(server_address=server, batch_size=batch_size,
                                               sequence_length=sequence_length)
        # The demonstrations' draws have a stream of their own (seed + tag), apart from the
        # table's.
        dataset = demonstrations.mix_sequence_demonstrations(
            dataset, store, demonstration_ratio=demonstration_ratio, period=replay_period,
            sequence_length=sequence_length, seed=4321 + seed)
        self._finish(
            server, adder, dataset, environment_spec=environment_spec, network=network,
            target_network=target_network, burn_in_length=burn_in_length,
            trace_length=trace_length, replay_period=replay_period, batch_size=batch_size,
            min_replay_size=min_replay_size, samples_per_insert=samples_per_insert,
            epsilon=epsilon, checkpoint=checkpoint, checkpoint_subpath=checkpoint_subpath,
            seed=seed, counter=counter, logger=logger, discount=discount,
            target_update_period=target_update_period,
            importance_sampling_exponent=importance_sampling_exponent,
            max_replay_size=max_replay_size, learning_rate=learning_rate,
            store_lstm_state=False)
