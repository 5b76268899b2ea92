"""The MCTS agent end to end on the GPU: the reference's agent test configuration
(acme/agents/tf/mcts/agent_test.py) through EnvironmentLoop, and the actor planning on Catch with
the learner's native evaluation."""

import numpy as np
import pytest
import torch

from acme_amd import specs
from acme_amd.agents.mcts import MCTS, AZLearner, MCTSActor
from acme_amd.agents.mcts.models import Simulator
from acme_amd.environment_loop import EnvironmentLoop
from acme_amd.networks import PolicyValueMLP
from acme_amd.optimizers import Adam
from acme_amd.testing import fakes
from acme_amd.utils import loggers

pytestmark = pytest.mark.gpu


def test_agent_runs_the_reference_configuration():
    num_actions = 5
    environment = fakes.DiscreteEnvironment(num_actions=num_actions, num_observations=10,
                                            obs_dtype=np.float32, episode_length=10)
    spec = specs.make_environment_spec(environment)
    network = PolicyValueMLP(int(np.prod(spec.observations.shape)), [50, 50], num_actions)
    agent = MCTS(environment_spec=spec, network=network, model=Simulator(environment),
                 optimizer=Adam(1e-3), n_step=1, discount=1.0, replay_capacity=100,
                 num_simulations=10, batch_size=10)
    learner = agent._learner  # noqa: SLF001
    before = learner.native.get_params("params")
    np.random.seed(0)
    EnvironmentLoop(environment, agent, logger=loggers.NoOpLogger()).run(num_episodes=2)
    torch.cuda.synchronize()
    assert learner.num_steps > 0
    after = learner.native.get_params("params")
    assert all(np.isfinite(v).all() for v in after.values())
    assert any((after[k] != before[k]).any() for k in after)
    assert np.isfinite(learner.native.loss.item())
    sample = next(iter(learner._iterator))  # noqa: SLF001
    pi = sample.data[5]["pi"].cpu().numpy()
    assert pi.shape == (10, num_actions) and pi.dtype == np.float32
    assert (pi >= 0).all()
    np.testing.assert_allclose(pi.astype(np.float64).sum(axis=1), 1.0, atol=1e-6)
    variables = agent.get_variables(["policy"])
    assert set(variables[0]) == {name for name, _ in network.tensor_shapes()}


def test_actor_plans_on_catch_with_the_learners_evaluation():
    from acme_amd.environments.catch import Catch
    env = Catch(rows=4, columns=3, seed=1)
    spec = specs.make_environment_spec(env)
    network = PolicyValueMLP(12, (32,), 3)
    learner = AZLearner(network, Adam(1e-3), iter(()), discount=1.0, batch_size=4,
                        logger=loggers.NoOpLogger())
    probs, value = learner.evaluate(env.reset().observation)
    assert probs.shape == (3,) and isinstance(value, float)
    assert abs(float(probs.astype(np.float64).sum()) - 1.0) < 1e-6
    batch_probs, batch_values = learner.evaluate(np.zeros((1, 12), np.float32))
    assert batch_probs.shape == (1, 3) and batch_values.shape == (1,)
    # More rows than the learner's batch size go through the native call in chunks.
    many = np.random.default_rng(0).standard_normal((9, 4, 3)).astype(np.float32)
    p9, v9 = learner.evaluate(many)
    assert p9.shape == (9, 3) and v9.shape == (9,)
    for i in (0, 4, 8):
        pi, vi = learner.evaluate(many[i])
        np.testing.assert_array_equal(pi, p9[i])
        assert vi == float(v9[i])

    class Adder:
        steps = []

        def add_first(self, timestep):
            pass

        def add(self, action, next_timestep, extras=()):
            self.steps.append(extras)

    env = Catch(rows=4, columns=3, seed=1)
    actor = MCTSActor(spec, Simulator(env), learner, discount=1.0, num_simulations=10,
                      adder=Adder())
    np.random.seed(0)
    ts = env.reset()
    actor.observe_first(ts)
    action = actor.select_action(ts.observation)
    assert action.dtype == np.int32 and 0 <= action < 3
    actor.observe(action, env.step(action))
    pi = Adder.steps[-1]["pi"]
    assert pi.shape == (3,) and pi.dtype == np.float32 and (pi >= 0).all()
    assert abs(float(pi.astype(np.float64).sum()) - 1.0) < 1e-6


@pytest.mark.parametrize("with_signature", [False, True])
def test_table_keeps_a_one_leaf_extras_dict(with_signature):
    """(o, a, r, d, o', {'pi': x}) has as many elements as leaves but is no flat tuple: the
    table flattens it, and every sampled row comes back whole."""
    from acme_amd import datasets, replay
    from acme_amd.adders import reverb as adders
    spec = specs.EnvironmentSpec(
        observations=specs.Array((4,), np.float32), actions=specs.DiscreteArray(3),
        rewards=specs.Array((), np.float32), discounts=specs.BoundedArray((), np.float32, 0., 1.))
    signature = adders.NStepTransitionAdder.signature(
        spec, {"pi": specs.Array((3,), np.float32)}) if with_signature else None
    table = replay.Table(name=adders.DEFAULT_PRIORITY_TABLE, sampler=replay.selectors.Uniform(),
                         remover=replay.selectors.Fifo(), max_size=16,
                         rate_limiter=replay.rate_limiters.MinSize(1), signature=signature)
    server = replay.Server([table], port=None)
    for i in range(5):
        item = (np.full(4, i, np.float32), np.int32(i % 3), np.float32(i + 0.5), np.float32(1.0),
                np.full(4, i + 1, np.float32), {"pi": np.array([i, 1, 2], np.float32)})
        table.insert(item, 1.0)
    dataset = datasets.make_reverb_dataset(server_address=f"localhost:{server.port}", batch_size=8)
    o, a, r, d, o2, extras = next(iter(dataset)).data
    assert set(extras) == {"pi"}
    o, a, r, o2, pi = (x.cpu().numpy() for x in (o, a, r, o2, extras["pi"]))
    assert pi.shape == (8, 3) and pi.dtype == np.float32
    i = o[:, 0]
    assert set(i.astype(int)) <= set(range(5))
    np.testing.assert_array_equal(o, np.repeat(i[:, None], 4, axis=1))
    np.testing.assert_array_equal(o2, o + 1)
    np.testing.assert_array_equal(r, i + 0.5)
    np.testing.assert_array_equal(a, i.astype(np.int32) % 3)
    np.testing.assert_array_equal(pi, np.stack([i, np.ones(8), np.full(8, 2.0)], axis=1))
