"""The device tree search (acme_mcts_search_*, MCTSActor(search="native")) against search.mcts
itself run in float64: the model and the network are the float64 forwards of
tests/mlp_model_oracle.py and tests/az_oracle.py, the search policy computes search.puct's
scores, and the `rng` stand-in breaks ties by the device's Philox rule (include/acme_hip.h).

Counts (root visits, every node's edge visits, nodes used, deepest path) must be equal; root
prior, value and child values meet tests/test_az_gpu.py::_close (rtol 1e-5 + 2e-6 max|ref|).
A float32 search may choose differently from float64 where two scores are within rounding
(~1e-6 |score|), so each case fixes a seed for which the reference's smallest gap between the
best and the best non-tied score is >= 1e-3 of its largest |score|, and asserts that.  The
reference is tests/mcts_search_oracle.py; the kernel's edges are in
tests/test_mcts_native_search_edges_gpu.py."""

import numpy as np
import pytest
import torch

from tests import az_oracle as AO
from tests.mcts_search_oracle import _reference, _setup
from tests.test_az_gpu import _close, _params as _az_params

pytestmark = pytest.mark.gpu

# (D, model hidden, net hidden, A, S, activation, discount, stream_weights, seed).  The wide
# case's 280 KB of weights cannot be staged.  TOL = 0.5: terminal where the logit is negative.
CASES = [(1, (1,), (1,), 1, 3, "softmax", 1.0, False, 0),
         (5, (7,), (7,), 3, 24, "softmax", 0.99, False, 2),
         (5, (7,), (7,), 3, 24, "softmax", 0.99, True, 2),
         (50, (50,), (50,), 3, 50, "softmax", 1.0, False, 0),
         (20, (33, 17), (36, 68), 18, 40, "sigmoid", 0.99, False, 67),
         (7, (36,), (36,), 64, 8, "softmax", 0.99, False, 2),
         (64, (256,), (256, 256), 4, 12, "softmax", 0.99, False, 0)]
TOL = 0.5


def _native(D, mh, zh, A, S, seed, stream=False, zero=False):
    from acme_amd.native import NativeAZ, NativeMCTSSearch, NativeMLPModel
    _, _, mp, zp, root = _setup(D, mh, zh, A, seed, zero)
    az = NativeAZ(obs_dim=D, hidden=zh, num_actions=A, max_batch=4)
    model = NativeMLPModel(obs_dim=D, hidden=mh, num_actions=A, max_batch=4)
    az.set_params(zp)
    model.set_params(mp)
    return NativeMCTSSearch(az, model, S, stream_weights=stream), torch.from_numpy(root).cuda()


def _check_counts(n, row, ref, S):
    got = n.unpack(row)
    assert got["status"] == 0 and got["visits"].sum() == S
    np.testing.assert_array_equal(got["visits"], ref["visits"])
    assert (got["nodes"], got["deepest"]) == (ref["nodes"], ref["deepest"])
    tree = n.debug_buffer("visits").reshape(S + 1, -1)
    np.testing.assert_array_equal(tree[:got["nodes"]], ref["tree"])
    assert not tree[got["nodes"]:].any()
    return got


@pytest.mark.parametrize("D,mh,zh,A,S,activation,discount,stream,seed", CASES)
def test_search_matches_f64(D, mh, zh, A, S, activation, discount, stream, seed):
    ref = _reference(D, mh, zh, A, S, activation, discount, seed)
    print({k: ref[k] for k in ("gap", "scale", "nodes", "deepest", "terminal_edges", "revisits")})
    assert ref["gap"] >= 1e-3 * ref["scale"], "the seed leaves a near-tie: pick another"
    assert activation != "sigmoid" or (ref["terminal_edges"] >= 1 and ref["revisits"] >= 1)
    n, root = _native(D, mh, zh, A, S, seed, stream)
    row = n.run(root, S, discount, sigmoid=activation == "sigmoid", terminal_tol=TOL,
                seed=seed).cpu().numpy()
    got = _check_counts(n, row, ref, S)
    _close(got["prior"], ref["prior"], name="root prior")
    _close([got["root_value"]], [ref["root_value"]], name="root value")
    _close(got["values"], ref["values"], name="root child values")


def test_all_ties():
    """Zero parameters: uniform priors, zero values and rewards, so every selection is a tie
    among the least visited actions and the Philox rule alone shapes the tree."""
    D, mh, zh, A, S = 5, (7,), (7,), 3, 24
    n, root = _native(D, mh, zh, A, S, 0, zero=True)
    ccs = (0, (1 << 32) + 5)
    refs = [_reference(D, mh, zh, A, S, "softmax", 1.0, 0, call_counter=c, zero=True) for c in ccs]
    assert (refs[0]["tree"] != refs[1]["tree"]).any()
    for cc, ref in zip(ccs, refs):
        assert ref["gap"] >= 1e-3 * ref["scale"]
        _check_counts(n, n.run(root, S, 1.0, seed=0, call_counter=cc).cpu().numpy(), ref, S)


def test_search_leaves_everything_alone():
    from acme_amd import specs
    from acme_amd.agents.mcts.models import MLPModel
    from acme_amd.environments.catch import Catch
    from acme_amd.native import NativeAZ, NativeMCTSSearch
    spec = specs.make_environment_spec(Catch(rows=3, columns=2))
    model = MLPModel(spec, replay_capacity=8, batch_size=4, hidden_sizes=(9,), seed=1)
    az = NativeAZ(obs_dim=6, hidden=(9,), num_actions=3, max_batch=4)
    az.set_params(_az_params(AO.AZConfig(6, (9,), 3), 2))
    n = NativeMCTSSearch(az, model.native, 16)
    rng = np.random.default_rng(0)
    model.reset(rng.standard_normal((3, 2)).astype(np.float32))
    model.save_checkpoint()
    model.step(1)

    def snapshot():
        bufs = [model._bufs] + [getattr(x, k) for x in (az, model.native)  # noqa: SLF001
                                for k in ("params", "grads", "m", "v")]
        return [b.clone() for b in bufs], (model._cur, model._ckpt)  # noqa: SLF001

    before, choice = snapshot()
    run = lambda: n.run(model.state_row, 16, 0.99, seed=3, call_counter=7)  # noqa: E731
    first = run().clone()
    after, choice2 = snapshot()
    assert choice == choice2 and all(torch.equal(x, y) for x, y in zip(before, after))
    assert torch.equal(first, run())
    # Both networks step, the search follows on the stream: it sees the updated parameters.
    B = 4
    az.step(*[torch.as_tensor(rng.standard_normal(s).astype(np.float32)).cuda()
              for s in ((B, 6), (B,), (B,), (B, 6))],
            torch.full((B, 3), 1 / 3, device="cuda"))
    ring = torch.as_tensor(rng.standard_normal((8, 15)).astype(np.float32)).cuda()
    ring[:, 6] = 1.0
    model.native.step(ring, torch.arange(B, dtype=torch.int32, device="cuda"))
    unsynchronised = run().clone()
    torch.cuda.synchronize()
    assert torch.equal(unsynchronised, run()) and not torch.equal(unsynchronised, first)


def test_create_refuses_networks_it_cannot_serve():
    from acme_amd.native import NativeAZ, NativeMCTSSearch, NativeMLPModel
    model = NativeMLPModel(obs_dim=6, hidden=(9,), num_actions=64, max_batch=4)
    for kw, field in ((dict(obs_dim=7), "obs_dim"), (dict(num_actions=3), "num_actions"),
                      (dict(hidden=(9, 257)), r"hidden\[1\]"), (dict(), "max_simulations")):
        az = NativeAZ(**{**dict(obs_dim=6, hidden=(9,), num_actions=64, max_batch=4), **kw})
        with pytest.raises(ValueError, match=field):
            NativeMCTSSearch(az, model, 101)  # (20 * 64 + 8) * 102 = 131376 > 131072
    NativeMCTSSearch(az, model, 100)


def test_actor_native_search():
    from acme_amd import networks, optimizers, specs
    from acme_amd.agents.mcts import MCTS
    from acme_amd.agents.mcts.models import MLPModel, Simulator
    from acme_amd.environment_loop import EnvironmentLoop
    from acme_amd.environments.catch import Catch
    from acme_amd.utils import loggers
    env = Catch(rows=10, columns=5, seed=0)
    spec = specs.make_environment_spec(env)
    common = dict(optimizer=optimizers.Adam(1e-3), n_step=1, discount=0.99, replay_capacity=1000,
                  num_simulations=8, environment_spec=spec, batch_size=16, search="native")
    model = MLPModel(spec, replay_capacity=1000, batch_size=16, hidden_sizes=(50,))
    agent = MCTS(networks.PolicyValueMLP(50, (50,), 3), model, **common)
    adder, stored = agent._actor._adder, []  # noqa: SLF001
    add = adder.add
    adder.add = lambda action, ts, extras=(): (stored.append(extras["pi"]),
                                               add(action, ts, extras=extras))
    np.random.seed(0)
    EnvironmentLoop(env, agent, logger=loggers.NoOpLogger()).run(num_episodes=3)
    assert len(stored) == 27 and model.num_steps == model.size - 15
    pi = np.array(stored) * 8
    assert pi.shape == (27, 3) and pi.dtype == np.float32
    np.testing.assert_allclose(pi, np.round(pi), atol=1e-5)
    assert (np.round(pi).sum(axis=1) == 8).all()
    with pytest.raises(ValueError, match="plans on a models.MLPModel"):
        MCTS(networks.PolicyValueMLP(50, (50,), 3), Simulator(env), **common)
