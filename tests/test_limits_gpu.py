"""Every learner at the ends of the ranges its create() accepts (include/acme_hip.h), and on
the inputs random data never produces, against the float64 oracles.

The cases are tests/limit_cases.py's (tests/test_limits_cpu.py shows on the oracle alone that
each data-edge input produces its edge).  Every comparison is made by the helpers of the
per-learner modules, at the bars their docstrings state: test_dqn_gpu.py, test_impala_gpu.py,
test_r2d2_learner_gpu.py, test_d4pg_gpu.py, test_ddpg_gpu.py, test_mpo_gpu.py and
test_dmpo_gpu.py.  No tolerance is introduced here.  Networks are tiny: a case is about one
limit, not about a workload.

For the two IMPALA batches whose importance ratios leave f32 exp's range the float32 oracle
itself stays within a ninth of every bar against float64 (worst: vs and pg_advantages at
0.105 of the bound with the peaked policy), so they are held to the module's bars as well.

Where float32 arithmetic itself misses a bar (the oracle run in float32 against float64 on
the case's inputs misses it too) that one quantity of that one case is held to 4x the float32
oracle's error, computed here on the case's inputs, and everything else stays: the relative
bar of R2D2's end-to-end errors at T = 256 (float32 oracle 2.8e-4 / 6.9e-4, kernels 5.7e-4 /
2.3e-4; limit_cases.R2D2) and D4PG's dqda at 65536 rows (float32 oracle 1.20e-5, kernel
1.25e-5; limit_cases.D4PG_F32_DQDA).  Measured on the MI355X; DESIGN.md 5.3 has the same.
"""

import ctypes
import re

import numpy as np
import pytest
import torch

from oracle import d4pg_oracle as D4
from oracle import dqn_oracle as DQ
from tests import limit_cases as C
from tests import test_d4pg_gpu as d4pg_t
from tests import test_ddpg_gpu as ddpg_t
from tests import test_dmpo_gpu as dmpo_t
from tests import test_dqn_gpu as dqn_t
from tests import test_impala_gpu as impala_t
from tests import test_mpo_gpu as mpo_t
from tests import test_r2d2_learner_gpu as r2d2_t
from tests.test_mpo_gpu import _report_all_misses  # noqa: F401  (MPO / DMPO helpers' misses)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ DQN


def _dqn_check(net, params, target, batch):
    """forward_backward against the oracle as test_dqn_gpu's
    test_forward_backward_matches_oracle, then one step: Adam on the kernel's own gradients
    (rtol 1e-6) and the step-0 target copy."""
    B = len(batch["a_tm1"])
    d = dqn_t._learner(net, B)
    d.set_params(params, target)
    dev = dqn_t._dev(batch)
    q = torch.empty(B, net.num_actions, device="cuda")
    d.forward_backward(*dev, q_tm1=q)
    torch.cuda.synchronize()
    masks = dqn_t._relu_masks(d, net, batch, params, B)
    out, grads = DQ.dqn_loss_and_grads(dqn_t._cfg(net), params, target, batch, np.float64,
                                       masks=masks)
    np.testing.assert_allclose(q.cpu().numpy(), out["q_tm1"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(d.loss.item(), out["loss"], rtol=1e-5)
    np.testing.assert_allclose(d.td_error[:B].cpu().numpy(), out["td_error"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(d.priorities[:B].cpu().numpy(), out["priorities"], rtol=1e-5,
                               atol=1e-6)
    dqn_t._check_grads(d.get_params("grads"), grads)
    d.step(*dev)
    torch.cuda.synchronize()
    g = d.get_params("grads")  # the step's own
    dqn_t._check_grads(g, grads)
    got, tgt = d.get_params("params"), d.get_params("target")
    for k in params:
        z = np.zeros_like(params[k])
        want = DQ.adam_update(params[k], g[k].reshape(z.shape), z, z, 1, 1e-3)[0]
        np.testing.assert_allclose(got[k].reshape(z.shape), want, rtol=1e-6, atol=1e-9, err_msg=k)
        np.testing.assert_array_equal(tgt[k], got[k], err_msg=k)
    assert d.num_steps == 1
    return out


@pytest.mark.parametrize("name", list(C.DQN_MLP))
def test_dqn_mlp_limits(name):
    _dqn_check(*C.dqn_mlp_case(name))


@pytest.mark.parametrize("name", list(C.DQN_ATARI))
def test_dqn_atari_head_limits(name):
    """The generic head kernels at the widest and the narrowest head."""
    _dqn_check(*C.dqn_atari_case(name))


@pytest.mark.parametrize("name", C.DQN_TIES)
def test_dqn_argmax_tie_takes_first_index(name):
    """Every selector row ties (all 9 entries / columns 2 and 8, which the 8-entry reads see
    in different groups); the oracle's np.argmax takes the first, and the later index is O(1)
    away in TD error (test_limits_cpu.py)."""
    net, params, target, batch, _ = C.dqn_tie_case(name)
    _dqn_check(net, params, target, batch)


# ------------------------------------------------------------------ IMPALA


@pytest.mark.parametrize("name", list(C.IMPALA))
def test_impala_limits(name):
    cfg, B, T, params, batch, kw = C.impala_case(name)
    n = impala_t._native(cfg, B, T, **kw)
    n.set_params(params)
    impala_t._run(n, batch)
    impala_t._compare(cfg, n, params, batch)
    if C.IMPALA[name].get("one_launch"):
        assert n.debug_buffer("lstm_timeout")[:1].view(np.uint32)[0] == 0


# ------------------------------------------------------------------ R2D2


@pytest.mark.parametrize("name", list(C.R2D2))
def test_r2d2_limits(name):
    """Two steps for the action counts (the second keeps the target), one for the long
    sequences."""
    c = C.R2D2[name]
    n = r2d2_t._compare(C.r2d2_cfg(c), B=c["B"], T=c["T"], seed=C.R2D2_SEED,
                        steps=2 if name.startswith("a") else 1,
                        errors_rtol=C.r2d2_errors_rtol(c))
    if c.get("one_launch"):
        assert n.debug_buffer("lstm_timeout").view(np.uint32)[0] == 0


def test_r2d2_greedy_tie_takes_first_index(monkeypatch):
    """q[2] = q[8] is the maximum of every online row; _compare holds the kernel's errors
    bit for bit to the oracle's loss on the kernel's own q, whose argmax takes the first."""
    cfg, B, T, params_fn, _, (j, k) = C.r2d2_tie_inputs()
    monkeypatch.setattr(r2d2_t, "_params", params_fn)
    n = r2d2_t._compare(cfg, B=B, T=T, seed=C.R2D2_TIE["seed"], steps=1)
    L = T - cfg.burn_in_length
    q = n.debug_buffer("q")[:L * B * cfg.num_actions].reshape(L * B, cfg.num_actions)
    np.testing.assert_array_equal(q[:, j], q[:, k])  # the kernel's rows tie too
    np.testing.assert_array_equal(q[:, j], q.max(axis=1))


# ------------------------------------------------------------------ D4PG / DDPG


def _d4pg_step(cfg, B, batch, f32_dqda=False):
    """One step from step count 1 (no target copy: the target network is its own draw) at
    test_d4pg_gpu's bars.  f32_dqda: dqda may miss its bar by limit_cases.d4pg_dqda_allowance."""
    n = d4pg_t._native(cfg, B)
    params, target = d4pg_t._random_params(cfg, 7), d4pg_t._random_params(cfg, 8)
    n.set_params(params, target)
    n.num_steps = 1
    n.step(*d4pg_t._dev(batch))
    torch.cuda.synchronize()
    z = {k: np.zeros_like(v) for k, v in params.items()}
    ref, raw, st = D4.d4pg_step(cfg, dict(params=params, target=target, m=z, v=dict(z),
                                          num_steps=1), batch, np.float64)
    K, A = cfg.num_atoms, cfg.act_dim
    d4pg_t._close(n.critic_loss.item(), ref["critic_loss"], name="critic_loss")
    d4pg_t._close(n.policy_loss.item(), ref["policy_loss"], rtol=1e-4, name="policy_loss")
    d4pg_t._close(n.debug_buffer("c_logits")[:B * K], ref["q_tm1"], name="q_tm1")
    d4pg_t._close(n.debug_buffer("t_logits")[:B * K], ref["q_t"], name="q_t")
    dqda = n.debug_buffer("dqda")[:B * A].reshape(B, A).astype(np.float64)
    if f32_dqda:
        extra = C.d4pg_dqda_allowance(cfg, params, target, batch)
        err = np.abs(dqda - ref["dqda"])
        bound = 1e-4 * np.abs(ref["dqda"]) + 2e-6 * np.abs(ref["dqda"]).max() + extra
        print(f"dqda: max |err| {err.max():.3e}, f32-oracle allowance {extra:.3e}")
        assert (err <= bound).all(), (float(err.max()), extra)
    else:
        d4pg_t._close(dqda, ref["dqda"], rtol=1e-4, name="dqda")
    d4pg_t._close(n.debug_buffer("norms"), ref["norms"], rtol=1e-4, name="norms")
    d4pg_t._check_grads(n, raw)
    d4pg_t._check_params(n.get_params("params"), st["params"], cfg.policy_lr)
    assert n.num_steps == 2


@pytest.mark.parametrize("name", list(C.D4PG))
def test_d4pg_limits(name):
    cfg, B = C.D4PG[name]
    _d4pg_step(cfg, B, d4pg_t._batch(cfg, B, 10), f32_dqda=name in C.D4PG_F32_DQDA)


def test_d4pg_projection_on_atoms_and_clipped():
    """TD targets exactly on an atom, at vmin / vmax, mid-way and clipped on either side
    (limit_cases.PROJECTION_R / _D): the projected target reaches the oracle through the
    critic loss and the critic's gradients (the head's bias gradient is sum_b softmax - target)."""
    cfg, batch = C.d4pg_projection_batch()
    _d4pg_step(cfg, len(batch["r_t"]), batch)


@pytest.mark.parametrize("name", list(C.DDPG))
def test_ddpg_limits(name):
    cfg, B = C.DDPG[name]
    ddpg_t._run_steps(cfg, B, B, 1 if B > 1000 else 2, 7, 20)


# ------------------------------------------------------------------ MPO / DMPO


@pytest.mark.parametrize("name", list(C.MPO))
def test_mpo_limits(name):
    """One step from step count 1: neither target is copied, so no KL is zero."""
    cfg, B = C.MPO[name]
    mpo_t._run_steps(cfg, B, 1, 1, 10, start=1,
                     target=C.mpo_target(name, cfg, mpo_t._random_params(cfg, 2)))


@pytest.mark.parametrize("name", list(C.DMPO))
def test_dmpo_limits(name):
    cfg, B = C.DMPO[name]
    dmpo_t._run_steps(cfg, B, 1, 1, 10, critic_scale=4.0, start=1)


# ------------------------------------------------------------------ rejections


def _rejected(n, change, names):
    """create() on learner n's own configuration with one field changed returns
    ACME_ERR_INVALID, no handle, and a message that names the limit."""
    from acme_amd import _lib
    cfg = type(n.cfg).from_buffer_copy(n.cfg)
    change(cfg)
    h = ctypes.c_void_p()
    rc = n._fn("create")(ctypes.byref(cfg), ctypes.byref(h))
    msg = _lib.lib().acme_last_error().decode(errors="replace")
    if rc == _lib.ACME_OK:
        n._fn("destroy")(h)
    assert rc == _lib.ACME_ERR_INVALID and not h.value, (rc, msg)
    assert re.search(names, msg), msg


def _set(field, value, index=None):
    def change(cfg):
        if index is None:
            setattr(cfg, field, value)
        else:
            getattr(cfg, field)[index] = value
    return change


def test_dqn_create_rejects_past_limits():
    from acme_amd.native import NativeDQN
    from acme_amd.networks import MLP
    n = dqn_t._learner(MLP(12, [32], 5), 4)
    for a in (0, 64):
        _rejected(n, _set("num_actions", a), r"num_actions must be in \[1, 63\]")
    _rejected(n, _set("num_hidden", 9), r"num_hidden must be in \[0, 8\]")
    with pytest.raises(ValueError, match="at most 8 hidden layers"):
        NativeDQN(network="mlp", num_actions=5, max_batch=4, obs_dtype="float32", obs_dim=12,
                  hidden=[4] * 9)


def test_impala_create_rejects_past_limits():
    cfg, B, T, _, _, _ = C.impala_case("head4")
    n = impala_t._native(cfg, B, T)
    for a in (0, 64):
        _rejected(n, _set("num_actions", a), r"num_actions must be in \[1, 63\]")
    _rejected(n, _set("max_sequence_length", 65), r"max_sequence_length must be in \[2, 64\]")


def test_r2d2_create_rejects_past_limits():
    n = r2d2_t._native(r2d2_t._cfg(), 2, 5)
    _rejected(n, _set("num_actions", 1025), r"num_actions must be in \[1, 1024\]")
    _rejected(n, _set("max_sequence_length", 257),
              r"max_sequence_length must be in \[burn_in_length \+ 2, 256\]")


def test_actor_critic_create_rejects_past_limits():
    """The checks D4PG, DDPG, MPO and DMPO share (on D4PG's create), num_atoms on D4PG and
    DMPO, num_samples on MPO and DMPO."""
    from acme_amd.native import NativeD4PG, NativeMPO
    cfg, B = C.D4PG["in64_k64"]  # obs 48 + act 16
    n = d4pg_t._native(cfg, B)
    for k in (1, 65):
        _rejected(n, _set("num_atoms", k), r"num_atoms must be in \[2, 64\]")
    _rejected(n, _set("obs_dim", 49), r"obs_dim \+ act_dim must be in \[2, 64\]")

    def act17(c):
        c.obs_dim, c.act_dim = 8, 17

    _rejected(n, act17, r"act_dim must be <= 16")
    for field in ("num_policy_layers", "num_critic_layers"):
        _rejected(n, _set(field, 5), r"layer count must be in \[1, 4\]")
    for w in (1028, 6):
        _rejected(n, _set("policy_sizes", w, 0),
                  r"policy layer sizes must be multiples of 4 in \[4, 1024\]")
        _rejected(n, _set("critic_sizes", w, 0),
                  r"critic layer sizes must be multiples of 4 in \[4, 1024\]")
    small = dict(obs_dim=3, act_dim=2, max_batch=4)
    with pytest.raises(ValueError, match="1..4 layer sizes"):
        NativeD4PG(policy_sizes=(8,) * 5, critic_sizes=(8,), **small)
    with pytest.raises(ValueError, match="act_dim must be <= 16"):
        NativeD4PG(obs_dim=8, act_dim=17, max_batch=4, policy_sizes=(8,), critic_sizes=(8,))
    with pytest.raises(ValueError, match=r"num_samples must be in \[1, 64\]"):
        NativeMPO(policy_sizes=(8,), critic_sizes=(8,), num_samples=65, **small)
    mcfg, mB = C.MPO["in64"]
    _rejected(mpo_t._native(mcfg, mB), _set("num_samples", 65),
              r"num_samples must be in \[1, 64\]")
    dcfg, dB = C.DMPO["in64_k2"]
    d = dmpo_t._native(dcfg, dB)
    _rejected(d, _set("num_samples", 65), r"num_samples must be in \[1, 64\]")
    for k in (1, 65):
        _rejected(d, _set("num_atoms", k), r"num_atoms must be in \[2, 64\]")
