"""The inputs of tests/test_limits_gpu.py against the float64 oracles alone (no GPU): a case
that silently stopped exercising its edge would be worthless, so every data-edge input is
shown here to produce the edge it is named after, and every oracle is run at every shape of
the case tables (tests/limit_cases.py) and must return finite output.
"""

import numpy as np
import pytest

from oracle import d4pg_oracle as D4
from oracle import dqn_oracle as DQ
from oracle import impala_oracle as IM
from oracle import r2d2_oracle as R2
from tests import ddpg_oracle as DD
from tests import dmpo_oracle as DM
from tests import limit_cases as C
from tests import mpo_oracle as MP
from tests import test_d4pg_gpu as d4pg_t
from tests import test_ddpg_gpu as ddpg_t
from tests import test_dmpo_gpu as dmpo_t
from tests import test_dqn_gpu as dqn_t
from tests import test_mpo_gpu as mpo_t
from tests import test_r2d2_learner_gpu as r2d2_t


def _finite(tree):
    for k, v in tree.items():
        if isinstance(v, dict):
            _finite(v)
        elif isinstance(v, (np.ndarray, float, np.floating)):
            assert np.isfinite(np.asarray(v, np.float64)).all(), k


def _zero_state(params):
    z = {k: np.zeros_like(v) for k, v in params.items()}
    return dict(m=z, v=dict(z), num_steps=0)


# ------------------------------------------------------------------ argmax ties


@pytest.mark.parametrize("name", C.DQN_TIES)
def test_dqn_tie_inputs_tie(name):
    """The selector's columns j and k are bitwise equal in float64 and the row maximum in
    every row, np.argmax takes j, and the loss from index k (the oracle on the target with
    its columns j and k exchanged) is more than 100x the loss bar (rtol 1e-5) away."""
    net, params, target, batch, (j, k) = C.dqn_tie_case(name)
    cfg = dqn_t._cfg(net)
    out, _ = DQ.dqn_loss_and_grads(cfg, params, target, batch, np.float64)
    q = out["q_t_selector"]
    assert q.dtype == np.float64
    np.testing.assert_array_equal(q[:, j], q[:, k])
    np.testing.assert_array_equal(q[:, j], q.max(axis=1))
    np.testing.assert_array_equal(np.argmax(q, axis=1), np.full(len(q), j))
    if name == "tie_pair":  # the pair alone: every other column is at least 1 below
        assert (np.delete(q, [j, k], axis=1).max(axis=1) <= q[:, j] - 0.99).all()
    other = C.swap_columns(target, ["mlp/linear_1/w", "mlp/linear_1/b"], j, k)
    out_k, _ = DQ.dqn_loss_and_grads(cfg, params, other, batch, np.float64)
    assert abs(out_k["loss"] - out["loss"]) > 100 * 1e-5 * abs(out["loss"])
    assert np.abs(out_k["td_error"] - out["td_error"]).max() > 0.1


def test_r2d2_tie_inputs_tie():
    """As the DQN pair, on the online q of every suffix row; the loss bar is rtol 2e-4."""
    cfg, B, T, params_fn, batch, (j, k) = C.r2d2_tie_inputs()
    seed = C.R2D2_TIE["seed"]
    params, target = params_fn(cfg, 10 + seed), params_fn(cfg, 20 + seed)
    np.testing.assert_array_equal(params[C.R2D2_ADV[0]][:, j], params[C.R2D2_ADV[0]][:, k])
    ref, _ = R2.loss_and_grads(cfg, params, target, batch)
    q = ref["q"].reshape(B * T, cfg.num_actions)
    assert q.dtype == np.float64
    np.testing.assert_array_equal(q[:, j], q[:, k])
    np.testing.assert_array_equal(q[:, j], q.max(axis=1))
    np.testing.assert_array_equal(np.argmax(q, axis=1), np.full(len(q), j))
    assert (np.delete(q, [j, k], axis=1).max(axis=1) <= q[:, j] - 0.99).all()
    ref_k, _ = R2.loss_and_grads(cfg, params, C.swap_columns(target, C.R2D2_ADV, j, k), batch)
    assert abs(ref_k["loss"] - ref["loss"]) > 100 * 2e-4 * abs(ref["loss"])
    # The batch is the one _compare draws, and the other seeds' parameters are untouched.
    again = r2d2_t._batch(cfg, B, T, 100 * seed)
    for key in batch:
        np.testing.assert_array_equal(batch[key], again[key])
    for s, p in ((20 + seed, target), (31, params_fn(cfg, 31))):
        np.testing.assert_array_equal(p[C.R2D2_ADV[0]], r2d2_t._params(cfg, s)[C.R2D2_ADV[0]])


# ------------------------------------------------------------------ D4PG projection


def test_d4pg_projection_batch_hits_every_branch():
    cfg, batch = C.d4pg_projection_batch()
    z = D4.support(cfg, np.float64)
    np.testing.assert_array_equal(z, np.arange(-10.0, 11.0))  # spacing exactly 1
    params, target = d4pg_t._random_params(cfg, 1), d4pg_t._random_params(cfg, 2)
    out, _ = D4.d4pg_loss_and_grads(cfg, params, target, batch, np.float64)
    t = out["target_dist"]
    np.testing.assert_allclose(t.sum(axis=1), 1.0, rtol=0, atol=1e-12)

    def one_hot(i):
        return np.eye(21)[i]

    def same(a, b):  # the softmax's own sum is 1 to a few ulp only
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)

    same(t[0], one_hot(0))
    same(t[1], one_hot(20))
    same(t[2], one_hot(10))
    same(t[3], one_hot(11))
    same(t[4], 0.5 * (one_hot(10) + one_hot(11)))
    same(t[5], t[0])
    same(t[6], t[1])
    same(t[7], 0.5 * (one_hot(0) + one_hot(1)))
    # Bootstrapped rows: r + 0.99 d z leaves the support at the end the row is named for.
    zt = batch["r_t"][:, None].astype(np.float64) + \
        (np.float64(np.float32(cfg.discount)) * batch["d_t"].astype(np.float64))[:, None] * z[None]
    assert (zt[8] > 10).any() and (zt[9] < -10).any() and (zt[10] > 10).any()
    assert (zt[11] > 10).any() and (zt[14] > 10).any() and (zt[15] < -10).any()
    assert (zt[12:14] > -10).all() and (zt[12:14] < 10).all()


# ------------------------------------------------------------------ IMPALA data edges


def _impala_out(name):
    cfg, B, T, params, batch, _ = C.impala_case(name)
    out, grads = IM.loss_and_grads(cfg, params, batch, np.float64)
    return cfg, batch, out, grads


def test_impala_rho_batches_leave_f32_exp_range():
    """log rho above f32 exp's overflow (88.7) in both batches and, with the peaked policy,
    below the last f32 denormal (-103.9); the float64 oracle stays finite throughout."""
    for name in ("rho_overflow", "rho_underflow"):
        _, _, out, grads = _impala_out(name)
        assert (out["log_rhos"] > 89).any(), name
        if name == "rho_underflow":
            assert (out["log_rhos"] < -104).any()
        _finite(out)
        _finite(grads)


def test_impala_reward_clip_batch_clips_some_rewards():
    cfg, batch, _, _ = _impala_out("reward_clip")
    r = np.abs(batch["reward"][:, :-1])
    assert cfg.max_abs_reward == 1.0 and (r > 1.0).any() and (r < 1.0).any()


def test_impala_discount_rows():
    _, batch, _, _ = _impala_out("discount_rows")
    assert not batch["discount"][0].any() and batch["discount"][1].all()


# ------------------------------------------------------------------ every shape, every oracle


@pytest.mark.parametrize("name", list(C.DQN_MLP) + list(C.DQN_ATARI))
def test_dqn_oracle_runs_case(name):
    net, params, target, batch = (C.dqn_mlp_case if name in C.DQN_MLP else C.dqn_atari_case)(name)
    out, grads = DQ.dqn_loss_and_grads(dqn_t._cfg(net), params, target, batch, np.float64)
    _finite({k: v for k, v in out.items() if k != "cache"})
    _finite(grads)


@pytest.mark.parametrize("name", list(C.IMPALA))
def test_impala_oracle_runs_case(name):
    cfg, B, T, params, batch, _ = C.impala_case(name)
    state = dict(params=params, **_zero_state(params))
    out, raw, st = IM.impala_step(cfg, state, batch)
    _finite(out)
    _finite(raw)
    _finite(st["params"])


@pytest.mark.parametrize("name", list(C.R2D2))
def test_r2d2_oracle_runs_case(name):
    c = C.R2D2[name]
    cfg = C.r2d2_cfg(c)
    batch = r2d2_t._batch(cfg, c["B"], c["T"], 0)
    ref, grads = R2.loss_and_grads(cfg, r2d2_t._params(cfg, 10), r2d2_t._params(cfg, 20), batch)
    _finite({k: ref[k] for k in ("q", "target_q", "errors", "loss")})
    _finite(grads)


@pytest.mark.parametrize("name", list(C.D4PG) + ["projection"])
def test_d4pg_oracle_runs_case(name):
    if name == "projection":
        cfg, batch = C.d4pg_projection_batch()
    else:
        cfg, B = C.D4PG[name]
        batch = d4pg_t._batch(cfg, B, 10)
    params = d4pg_t._random_params(cfg, 1)
    state = dict(params=params, target=d4pg_t._random_params(cfg, 2), **_zero_state(params))
    out, raw, st = D4.d4pg_step(cfg, state, batch, np.float64)
    _finite(out)
    _finite(raw)
    _finite(st["params"])


@pytest.mark.parametrize("name", list(C.DDPG))
def test_ddpg_oracle_runs_case(name):
    cfg, B = C.DDPG[name]
    params = ddpg_t._random_params(cfg, 1)
    state = dict(params=params, target=ddpg_t._random_params(cfg, 2), **_zero_state(params))
    out, raw, st = DD.ddpg_step(cfg, state, ddpg_t._batch(cfg, B, 10), np.float64)
    _finite(out)
    _finite(raw)
    _finite(st["params"])


@pytest.mark.parametrize("name", list(C.MPO))
def test_mpo_oracle_runs_case(name):
    cfg, B = C.MPO[name]
    target = C.mpo_target(name, cfg, mpo_t._random_params(cfg, 2))
    state = mpo_t._state(mpo_t._random_params(cfg, 1), target, 1)
    out, raw, st = MP.mpo_step(cfg, state, mpo_t._batch(cfg, B, 11), mpo_t._eps(cfg, B, 111),
                               np.float64)
    assert abs(out["stats"]["loss_temperature"]) >= 0.05  # no near-total cancellation
    _finite(out)
    _finite(raw)
    _finite(st["params"])


@pytest.mark.parametrize("name", list(C.DMPO))
def test_dmpo_oracle_runs_case(name):
    """The step test_limits_gpu.py runs (seeds 1 / 2, start = 1: no target copy), and what
    test_dmpo_gpu._run_steps asserts of its inputs before it compares: the projection's
    branches are all taken and loss_temperature is no near-total cancellation."""
    cfg, B = C.DMPO[name]
    state = mpo_t._state(dmpo_t._random_params(cfg, 1, critic_scale=4.0),
                         dmpo_t._random_params(cfg, 2, critic_scale=4.0), 1)
    batch = dmpo_t._batch(cfg, B, 11)
    dmpo_t._assert_projection_branches(cfg, batch)
    out, raw, st = DM.dmpo_step(cfg, state, batch, dmpo_t._eps(cfg, B, 111), np.float64)
    assert abs(out["stats"]["loss_temperature"]) >= 0.05
    _finite(out)
    _finite(raw)
    _finite(st["params"])
