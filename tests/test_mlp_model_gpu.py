"""The native learned model of the MCTS agent (acme_mlp_model_*, agents.mcts.models.MLPModel)
against the float64 oracle (tests/mlp_model_oracle.py).

Tolerances are those of tests/test_az_gpu.py (its helpers are used): losses and predictions
rtol 1e-5 + 2e-6 max|ref|; gradients 1e-4 |g| + 2e-5 max|g|; params within 2 lr and 99 % within
1e-5 relative.  A reward or logit of one or two rows takes its floor from sum_k |h_k w_k| + |b|,
which bounds a dot product's rounding error, as _close_few_values does there."""

import numpy as np
import pytest
import torch

from tests import mlp_model_oracle as O
from tests.test_az_gpu import _check_grads, _check_params, _close, _state_of

pytestmark = pytest.mark.gpu

RING = 40  # ring rows: more than any B below but the limits'


def _native(cfg, B, rows=1):
    from acme_amd.native import NativeMLPModel
    return NativeMLPModel(obs_dim=cfg.obs_dim, hidden=cfg.hidden, num_actions=cfg.num_actions,
                          max_batch=B, max_rows=rows, learning_rate=cfg.lr)


def _params(cfg, seed):
    rng = np.random.default_rng(seed)
    return {k: ((0.1 * rng.standard_normal(s)) if k.endswith("/b") else
                rng.standard_normal(s) / np.sqrt(s[0])).astype(np.float32)
            for k, s in O.tensor_shapes(cfg)}


def _ring(cfg, seed, rows=RING, d=None, actions=None):
    rng = np.random.default_rng(seed)
    D = cfg.obs_dim
    ring = rng.standard_normal((rows, 2 * D + 5)).astype(np.float32)  # a row stride past 2D + 3
    ring[:, D] = rng.choice(actions if actions is not None else cfg.num_actions, rows)
    ring[:, D + 1] = rng.uniform(-1, 1, rows)
    ring[:, D + 2] = (rng.random(rows) < 0.7) if d is None else d
    return ring


def _idx(B, seed, rows=RING):
    idx = np.random.default_rng(seed).integers(0, rows, B).astype(np.int32)
    if B > 1:
        idx[-1] = idx[0]  # a duplicate
    return idx


def _check_pred(cfg, params, got, ref, acts, tag):
    """Packed rows [next state, reward, logit]; the two scalar columns of one or two rows take
    the floor's scale from the dot product's terms."""
    D, L = cfg.obs_dim, len(cfg.hidden)
    got = np.asarray(got).reshape(ref.shape)
    _close(got[:, :D], ref[:, :D], name=f"next state{tag}")
    for col, tower in ((D, "reward_network"), (D + 1, "discount_network")):
        scale = None
        if len(ref) <= 2:
            w, b = params[f"{tower}/linear_{L}/w"], params[f"{tower}/linear_{L}/b"]
            terms = np.abs(acts[tower][L] * np.asarray(w, np.float64)[:, 0]).sum(axis=1) + abs(float(b[0]))
            scale = max(terms.max(), np.abs(ref[:, col]).max())
        _close(got[:, col], ref[:, col], name=f"{tower}{tag}", scale=scale)


def _check_step(n, cfg, state, ring, idx, tag="", dev=None, clamp=False):
    """One native step on ring rows idx from `state` (which the learner holds).  dev: the device
    tensor that holds `ring` (a view of a larger one, say), else ring is uploaded; clamp: the
    oracle clips idx into the ring, as the kernel does."""
    B = len(idx)
    n.step(torch.as_tensor(ring).cuda() if dev is None else dev, torch.as_tensor(idx).cuda())
    torch.cuda.synchronize()
    out, grads, new = O.step(cfg, state, O.batch_of(cfg, ring, idx, clamp=clamp))
    for k in ("loss", "state_loss", "reward_loss", "discount_loss"):
        got = getattr(n, k).item()
        assert np.isfinite(got), k
        _close(got, out[k], name=f"{k}{tag}")
    _check_pred(cfg, state["params"], n.debug_buffer("pred")[:B * (cfg.obs_dim + 2)], out["pred"],
                out["acts"], tag)
    _close(n.debug_buffer("dout")[:out["dout"].size], out["dout"], name=f"dout{tag}")
    _check_grads(n, grads)
    _check_params(n.get_params("params"), new["params"], cfg.lr)


# B = 17 crosses a 16-row tile, 33 fills three slab slots; 3, 5, 7, 36, 50 are off the MFMA tile.
@pytest.mark.parametrize("B,D,hidden,A", [
    (1, 3, (5,), 1), (2, 3, (5,), 3), (16, 50, (50,), 3), (17, 7, (50,), 3),
    (33, 7, (36, 68), 64), (33, 50, (36, 68), 3), (17, 3, (256, 256, 256), 64),
    (2, 50, (256, 256, 256), 1)])
def test_step_matches_oracle(B, D, hidden, A):
    cfg = O.Config(D, hidden, A)
    n = _native(cfg, B)
    n.set_params(_params(cfg, 1))
    ring = _ring(cfg, 2)
    for s in range(3):  # teacher-forced: the oracle continues from the kernel's state
        _check_step(n, cfg, _state_of(n), ring, _idx(B, 10 + s), tag=f" t={s + 1}")
    state = _state_of(n)
    for s in range(3):  # free-running
        idx = _idx(B, 20 + s)
        n.step(torch.as_tensor(ring).cuda(), torch.as_tensor(idx).cuda())
        _, _, state = O.step(cfg, state, O.batch_of(cfg, ring, idx))
    assert n.num_steps == 6
    _check_params(n.get_params("params"), state["params"], cfg.lr)


@pytest.mark.parametrize("case", ["d_zero", "d_one", "big_logits", "unused_action"])
def test_inputs_that_can_go_wrong(case):
    cfg = O.Config(7, (36, 68), 5)
    B, D = 33, cfg.obs_dim
    p = _params(cfg, 3)
    ring = _ring(cfg, 4, d={"d_zero": 0.0, "d_one": 1.0}.get(case),
                 actions=[0, 1, 3, 4] if case == "unused_action" else None)
    idx = _idx(B, 5)
    if case == "big_logits":  # the discount logits reach +-50
        w, b = "discount_network/linear_2/w", "discount_network/linear_2/b"
        p[b] = np.zeros_like(p[b])
        x = O.forward(cfg, p, ring[idx, :D], ring[idx, D])[2]
        p[w] = (p[w] * (50.0 / np.abs(x).max())).astype(np.float32)
        x = O.forward(cfg, p, ring[idx, :D], ring[idx, D])[2]
        assert np.abs(x).max() >= 49.0
    n = _native(cfg, B)
    n.set_params(p)
    _check_step(n, cfg, _state_of(n), ring, idx, tag=f" {case}")
    if case == "unused_action":
        g = n.get_params("grads")
        for tower in O.TOWERS:
            assert (g[f"{tower}/linear_0/w"][D + 2] == 0.0).all(), tower


@pytest.mark.parametrize("rows", [1, 2, 17, 1024])
@pytest.mark.parametrize("D,hidden,A", [(50, (50,), 3), (256, (256, 256, 256), 64)])
def test_predict_matches_oracle(D, hidden, A, rows):
    cfg = O.Config(D, hidden, A)
    n = _native(cfg, 4, rows=1024)  # rows = 1024 = max_rows
    p = _params(cfg, 7)
    n.set_params(p)
    before = [x.clone() for x in (n.params, n.m, n.v, n.grads)]
    rng = np.random.default_rng(8)
    state = torch.as_tensor(rng.standard_normal((rows, D)).astype(np.float32)).cuda()
    for hop in range(2):  # the second hop reads the first's packed output as its state
        actions = rng.integers(0, A, rows).astype(np.int32)
        by_value = rows == 1 and hop == 0
        out = n.predict_packed(state, int(actions[0]) if by_value
                               else torch.as_tensor(actions).cuda())
        s, r, x, acts = O.forward(cfg, p, state.cpu().numpy()[:, :D], actions)
        _check_pred(cfg, p, out.cpu().numpy(), np.column_stack([s, r, x]), acts, f" hop {hop}")
        state = out
    for x, y in zip(before, (n.params, n.m, n.v, n.grads)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_limits():
    from acme_amd import _lib
    W, A, R = _lib.MLP_MODEL_MAX_WIDTH, _lib.MLP_MODEL_MAX_ACTIONS, _lib.MLP_MODEL_MAX_ROWS
    cfg = O.Config(W, (W,) * _lib.MLP_MODEL_MAX_HIDDEN, A)
    n = _native(cfg, R, rows=R)
    n.set_params(_params(cfg, 12))
    ring = _ring(cfg, 13, rows=R + 7)
    _check_step(n, cfg, _state_of(n), ring, _idx(R, 14, rows=R + 7), tag=" limits")
    p = n.get_params("params")
    actions = ring[:R, W].astype(np.int32)
    out = n.predict_packed(torch.as_tensor(ring[:R]).cuda(), torch.as_tensor(actions).cuda())
    s, r, x, acts = O.forward(cfg, p, ring[:R, :W], actions)
    _check_pred(cfg, p, out.cpu().numpy(), np.column_stack([s, r, x]), acts, " limits")
    buf = torch.zeros(3, W + 2, device="cuda")  # rows 1-2 as state, rows 0-1 as out
    with pytest.raises(ValueError, match="must not overlap"):
        n.predict_packed(buf[1:3], torch.zeros(2, dtype=torch.int32, device="cuda"), out=buf[0:2])
    ok = dict(obs_dim=8, hidden=(8,), num_actions=3, max_batch=4, max_rows=4)
    for bad, msg in ((dict(obs_dim=W + 1), "obs_dim must be in"),
                     (dict(num_actions=A + 1), "num_actions must be in"),
                     (dict(hidden=(8,) * 4), "num_hidden must be in"),
                     (dict(hidden=(8, W + 1)), r"hidden\[1\] must be in"),
                     (dict(max_batch=R + 1), "max_batch must be in"),
                     (dict(max_rows=R + 1), "max_rows must be in")):
        from acme_amd.native import NativeMLPModel
        with pytest.raises(ValueError, match=msg):
            NativeMLPModel(**{**ok, **bad})


def test_step_repeats_bit_for_bit():
    cfg = O.Config(7, (36, 68), 5)
    B = 33
    ring, idx = torch.as_tensor(_ring(cfg, 5)).cuda(), torch.as_tensor(_idx(B, 6)).cuda()
    got = []
    for _ in range(2):
        n = _native(cfg, B)
        assert [(name, shape) for name, _, shape in n.tensors] == O.tensor_shapes(cfg)
        assert all(off % 64 == 0 for _, off, _ in n.tensors)
        n.set_params(_params(cfg, 6))
        n.step(ring, idx)
        n.step(ring, idx)
        torch.cuda.synchronize()
        got.append(np.concatenate([n.params.cpu().numpy(), n._losses.cpu().numpy()]))  # noqa: SLF001
    np.testing.assert_array_equal(got[0].view(np.uint32), got[1].view(np.uint32))


@pytest.mark.parametrize("activation", ["softmax", "sigmoid"])
def test_model_follows_reference_semantics(activation):
    from acme_amd import dm_env, specs
    from acme_amd.agents.mcts.models import MLPModel
    from acme_amd.environments.catch import Catch
    cfg = O.Config(6, (9,), 3)  # a 3 x 2 board, three actions
    model = MLPModel(specs.make_environment_spec(Catch(rows=3, columns=2)), replay_capacity=6, batch_size=4, hidden_sizes=cfg.hidden,
                     seed=1, discount_activation=activation)
    n = model.native
    oracle = O.Model(cfg, _state_of(n), 6, 4, sigmoid=activation == "sigmoid")
    rng = np.random.default_rng(2)

    def same(ts, ref, params, tag):
        assert int(ts.step_type) == ref[0], tag
        acts = O.forward(cfg, params, prev[None], [action])[3]
        _check_pred(cfg, params, np.concatenate([np.ravel(ts.observation), [ts.reward, 0.0]]),
                    np.concatenate([ref[2], [ref[1], 0.0]])[None], acts, tag)

    obs = rng.standard_normal((3, 2)).astype(np.float32)
    assert model.needs_reset and model.reset(obs).first()
    oracle.reset(obs)
    for i in range(8):  # past batch_size = 4 and around the ring of 6
        if model.needs_reset:
            _ = model.reset(obs), oracle.reset(obs)
        nxt, action, last = rng.standard_normal((3, 2)).astype(np.float32), int(rng.integers(3)), i % 4 == 3
        reward, prev = float(rng.uniform(-1, 1)), obs.reshape(-1).astype(np.float64)
        nts = dm_env.termination(reward, nxt) if last else dm_env.transition(reward, nxt)
        ts = model.update(dm_env.transition(0.0, obs), action, nts)
        idx = None if model.last_indices is None else model.last_indices.cpu().numpy()
        params = oracle.state["params"]
        ref = oracle.update(obs, action, reward, nts.discount, nxt, last, idx)
        same(ts, ref, params, f" update {i}")
        assert model.needs_reset == oracle.needs_reset == last
        _check_params(n.get_params("params"), oracle.state["params"], cfg.lr)
        oracle.state = _state_of(n)  # teacher-forced
        obs = nxt
    assert model.num_steps == 5 and model.size == 6
    if activation == "sigmoid":  # a bias low enough to terminate
        p = n.get_params("params")
        p["discount_network/linear_1/b"][:] = -30.0
        n.set_params(p)
        oracle.state = _state_of(n)
    for m in (model, oracle):
        m.reset(obs)
        m.save_checkpoint()
    for k, action in enumerate((0, 2, 1, 1)):  # three steps, load, one step
        if k == 3 or model.needs_reset:
            _ = model.load_checkpoint(), oracle.load_checkpoint()
        prev = oracle._state.copy()  # noqa: SLF001
        same(model.step(action), oracle.step(action), oracle.state["params"], f" step {k}")
        assert model.needs_reset == oracle.needs_reset == (activation == "sigmoid")


def test_agent_runs_on_learned_model():
    from acme_amd import networks, optimizers, specs
    from acme_amd.agents.mcts import MCTS
    from acme_amd.agents.mcts.models import MLPModel
    from acme_amd.environment_loop import EnvironmentLoop
    from acme_amd.environments.catch import Catch
    from acme_amd.utils import loggers
    env = Catch(rows=10, columns=5, seed=0)
    spec = specs.make_environment_spec(env)
    model = MLPModel(spec, replay_capacity=1000, batch_size=16, hidden_sizes=(50,))
    agent = MCTS(networks.PolicyValueMLP(50, (50,), 3), model, optimizers.Adam(1e-3), n_step=1,
                 discount=0.99, replay_capacity=1000, num_simulations=8, environment_spec=spec, batch_size=16)
    np.random.seed(0)
    EnvironmentLoop(env, agent, logger=loggers.NoOpLogger()).run(num_episodes=2)
    assert model.size >= 16 and model.num_steps == model.size - 15  # updates with size >= 16
    for k in ("loss", "state_loss", "reward_loss", "discount_loss"):
        assert np.isfinite(getattr(model.native, k).item()), k
