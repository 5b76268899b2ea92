"""The native AlphaZero learner step and evaluation (acme_az_*) against the float64 oracle
(tests/az_oracle.py).

Tolerances are those of tests/test_ddpg_gpu.py:
  losses, values, probabilities: rtol 1e-5 (+ an atol of 2e-6 times the tensor's largest
      magnitude, the fp32 rounding floor of its scale)
  gradients: per tensor |g - g_ref| <= 1e-4 |g_ref| + 2e-5 max|g_ref|
  Adam-updated params: every element within 2 lr of the oracle's and 99% within 1e-5 relative.
"""

import numpy as np
import pytest
import torch

from tests import az_oracle as O

pytestmark = pytest.mark.gpu

A_MAX = 64  # ACME_AZ_MAX_ACTIONS

# (B, D, hidden, A): B = 33 crosses the 32-row tile and 2B = 66 crosses 64; D = 3 and D = 7
# and the widths 5, 50, 36 take the loaders for sizes that are no multiple of 4.
SHAPES = [(1, 3, (5,), 1), (2, 3, (5,), 3), (5, 8, (50, 50), 5), (33, 10, (50, 50), 5),
          (33, 10, (36, 68), 64), (33, 7, (36, 68), A_MAX), (8, 10, (256, 256), 18)]


def _cfg(D, hidden, A, **kw):
    return O.AZConfig(obs_dim=D, hidden=tuple(hidden), num_actions=A, **kw)


def _native(cfg, B, rows=1):
    from acme_amd.native import NativeAZ
    return NativeAZ(obs_dim=cfg.obs_dim, hidden=cfg.hidden, num_actions=cfg.num_actions,
                    max_batch=B, max_eval_rows=rows, activate_final=cfg.activate_final,
                    discount=cfg.discount, learning_rate=cfg.lr, adam_beta1=cfg.b1,
                    adam_beta2=cfg.b2, adam_epsilon=cfg.eps)


def _params(cfg, seed):
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in O.az_tensor_shapes(cfg):
        v = 0.1 * rng.standard_normal(shape) if name.endswith("/b") else \
            rng.standard_normal(shape) / np.sqrt(shape[0])
        out[name] = v.astype(np.float32)
    return out


def _batch(cfg, B, seed, pi="dirichlet", d_zero=False):
    rng = np.random.default_rng(seed)
    A = cfg.num_actions
    if pi == "onehot":
        p = np.eye(A)[rng.integers(0, A, B)]
    elif pi == "uniform":
        p = np.full((B, A), 1.0 / A)
    else:
        p = rng.dirichlet(np.ones(A), B)
    d = np.zeros(B) if d_zero else np.where(rng.random(B) < 0.2, 0.0, 1.0)
    return dict(o_t=rng.standard_normal((B, cfg.obs_dim)).astype(np.float32),
                r_t=rng.uniform(-1, 1, B).astype(np.float32), d_t=d.astype(np.float32),
                o_tp1=rng.standard_normal((B, cfg.obs_dim)).astype(np.float32),
                pi=p.astype(np.float32))


def _dev(batch):
    return [torch.as_tensor(batch[k]).cuda().contiguous()
            for k in ("o_t", "r_t", "d_t", "o_tp1", "pi")]


def _close(got, ref, rtol=1e-5, floor=2e-6, name="", scale=None):
    """The project's rule: the floor is 2e-6 times ref's own largest magnitude.  scale: another
    magnitude for the floor, used only by _close_few_values."""
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    scale = max(float(np.abs(ref).max()) if scale is None else float(scale), 1e-30)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    print(f"{name}: max |err| {err:.3e}, scale {scale:.3e}")
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=floor * scale, err_msg=name)


def _close_few_values(cfg, params, obs, got, ref, name):
    """Values of one or two rows.  A value is the dot product h . wv + bv, and one row's can
    cancel to near zero (-0.003 from terms that sum to 2.2 in magnitude at rows = 1 below), where
    no float32 evaluation meets a floor taken from the result: a float32 numpy restatement
    misses it by 1.7x.  The rounding error of a dot product is bounded by its terms,
    n u sum_k |h_k w_k|, so with so few rows the floor's scale is the largest sum_k |h_k w_k| +
    |bv| of the compared rows instead of the largest |v|; the rtol stays 1e-5."""
    assert len(ref) <= 2
    _, _, acts = O.forward(cfg, params, obs)
    wv = np.asarray(params[O.VW], np.float64)[:, 0]
    terms = (np.abs(acts[-1] * wv[None, :]).sum(axis=1) + abs(float(params[O.VB][0]))).max()
    _close(got, ref, name=name, scale=max(terms, np.abs(ref).max()))


def _check_grads(native, g_ref):
    g = native.get_params("grads")
    for name, ref in g_ref.items():
        got = g[name].reshape(ref.shape).astype(np.float64)
        scale = np.abs(ref).max()
        err = np.abs(got - ref)
        bound = 1e-4 * np.abs(ref) + 2e-5 * scale + 1e-30
        print(f"grad {name}: max |err| {float(err.max()):.3e}, scale {float(scale):.3e}")
        assert (err <= bound).all(), (name, float(err.max()), float(scale))


def _check_params(got, ref, lr):
    for k, r in ref.items():
        gk = got[k].reshape(r.shape).astype(np.float64)
        err = np.abs(gk - r)
        assert err.max() <= 2 * lr + 1e-6, (k, float(err.max()))
        frac = np.mean(err <= 1e-5 * np.abs(r) + 1e-7)
        assert frac >= 0.99, (k, frac)


def _state_of(n) -> dict:
    f = lambda w: {k: v.astype(np.float64) for k, v in n.get_params(w).items()}  # noqa: E731
    return dict(params=f("params"), m=f("m"), v=f("v"), num_steps=n.num_steps)


def _check_step(n, cfg, state, batch, tag=""):
    """One native step on `batch` from `state` (which the learner holds) against the oracle;
    returns the oracle's new state."""
    B, A = len(batch["r_t"]), cfg.num_actions
    n.step(*_dev(batch))
    torch.cuda.synchronize()
    out, grads, new = O.az_step(cfg, state, batch)
    for k in ("loss", "value_loss", "policy_loss"):
        got = getattr(n, k).item()
        assert np.isfinite(got), k
        _close(got, out[k], name=f"{k}{tag}")
    _close(n.debug_buffer("logits")[:B * A], out["logits"], name=f"logits{tag}")
    _close(n.debug_buffer("v")[:2 * B], out["v"], name=f"v{tag}")
    _close(n.debug_buffer("td")[:B], out["td"], name=f"td{tag}")
    _check_grads(n, grads)
    _check_params(n.get_params("params"), new["params"], cfg.lr)
    return new


def test_tensor_layout():
    cfg = _cfg(7, (36, 68), 5)
    n = _native(cfg, 4)
    assert [(name, shape) for name, _, shape in n.tensors] == O.az_tensor_shapes(cfg)
    offs = [off for _, off, _ in n.tensors]
    assert offs == sorted(offs) and all(o % 64 == 0 for o in offs)


@pytest.mark.parametrize("B,D,hidden,A,activate_final",
                         [s + (False,) for s in SHAPES] + [SHAPES[2] + (True,), SHAPES[4] + (True,)])
def test_step_matches_oracle(B, D, hidden, A, activate_final):
    cfg = _cfg(D, hidden, A, activate_final=activate_final)
    n = _native(cfg, B)
    n.set_params(_params(cfg, 1))
    # Teacher-forced: the oracle continues from the kernel's parameters and moments.
    for s in range(3):
        _check_step(n, cfg, _state_of(n), _batch(cfg, B, 10 + s), tag=f" t={s + 1}")
    # Free-running: both continue from their own state.
    state = _state_of(n)
    for s in range(3):
        batch = _batch(cfg, B, 20 + s)
        n.step(*_dev(batch))
        _, _, state = O.az_step(cfg, state, batch)
    assert n.num_steps == 6
    _check_params(n.get_params("params"), state["params"], cfg.lr)


@pytest.mark.parametrize("case", ["d_zero", "onehot", "uniform", "big_logits"])
def test_inputs_that_can_go_wrong(case):
    cfg = _cfg(10, (50, 50), 5)
    B = 33
    n = _native(cfg, B)
    p = _params(cfg, 2)
    if case == "big_logits":  # logits reach +-50
        p[O.PB] = np.zeros_like(p[O.PB])
        lg, _, _ = O.forward(cfg, p, _batch(cfg, B, 3)["o_t"])
        p[O.PW] = (p[O.PW] * (50.0 / np.abs(lg).max())).astype(np.float32)
    n.set_params(p)
    batch = _batch(cfg, B, 3, pi=case if case in ("onehot", "uniform") else "dirichlet",
                   d_zero=case == "d_zero")
    if case == "big_logits":
        lg, _, _ = O.forward(cfg, p, batch["o_t"])
        assert np.abs(lg).max() >= 49.0
    _check_step(n, cfg, _state_of(n), batch, tag=f" {case}")


def test_smaller_batches_than_created_for():
    cfg = _cfg(10, (50, 50), 5)
    n = _native(cfg, 8)
    n.set_params(_params(cfg, 4))
    for i, B in enumerate((3, 8)):
        _check_step(n, cfg, _state_of(n), _batch(cfg, B, 30 + i), tag=f" B={B}")
    with pytest.raises(ValueError, match="batch must be in"):
        n.step(*_dev(_batch(cfg, 9, 0)))


def test_step_repeats_bit_for_bit():
    cfg = _cfg(10, (36, 68), 64)
    B = 33
    batch = _dev(_batch(cfg, B, 5))
    got = []
    for _ in range(2):
        n = _native(cfg, B)
        n.set_params(_params(cfg, 6))
        n.step(*batch)
        n.step(*batch)
        torch.cuda.synchronize()
        got.append((n.params.cpu().numpy().copy(), n._losses.cpu().numpy().copy()))  # noqa: SLF001
    np.testing.assert_array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32))
    np.testing.assert_array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32))


# The fused kernel takes rows <= 32 at widths <= 256; hidden 257 is the smallest width past it,
# rows 33 the smallest row count.
@pytest.mark.parametrize("hidden,rows,path", [
    ((50, 50), 1, "fused"), ((50, 50), 2, "fused"), ((50, 50), 17, "fused"),
    ((256, 256), 32, "fused"), ((257,), 1, "layered"), ((257,), 2, "layered"),
    ((257,), 17, "layered"), ((50, 50), 33, "layered")])
@pytest.mark.parametrize("activate_final", [False, True])
def test_evaluate_matches_oracle(hidden, rows, path, activate_final):
    from acme_amd import _lib
    fused = rows <= _lib.AZ_FUSED_MAX_ROWS and max(hidden) <= _lib.AZ_FUSED_MAX_WIDTH
    assert fused == (path == "fused")
    cfg = _cfg(10, hidden, 5, activate_final=activate_final)
    n = _native(cfg, 4, rows=rows)
    p = _params(cfg, 7)
    n.set_params(p)
    before = [x.clone() for x in (n.params, n.m, n.v, n.grads)]
    obs = np.random.default_rng(8).standard_normal((33, cfg.obs_dim)).astype(np.float32)[:rows]
    probs, value = n.evaluate(torch.as_tensor(obs).cuda())
    probs, value = probs.cpu().numpy(), value.cpu().numpy()
    rp, rv = O.evaluate(cfg, p, obs)
    _close(probs, rp, name="probs")
    if rows <= 2:
        _close_few_values(cfg, p, obs, value, rv, "value")
    else:
        _close(value, rv, name="value")
    np.testing.assert_allclose(probs.astype(np.float64).sum(axis=1), 1.0, atol=1e-6)
    for x, y in zip(before, (n.params, n.m, n.v, n.grads)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    with pytest.raises(ValueError, match="rows must be in"):
        n.evaluate(torch.zeros(rows + 1, cfg.obs_dim, device="cuda"))


@pytest.mark.parametrize("hidden", [(50, 50), (257,)])
def test_evaluate_sees_the_update(hidden):
    cfg = _cfg(10, hidden, 5)
    n = _native(cfg, 8, rows=2)
    n.set_params(_params(cfg, 9))
    batch = _batch(cfg, 8, 11)
    state = _state_of(n)
    n.step(*_dev(batch))
    probs, value = n.evaluate(torch.as_tensor(batch["o_t"][:2]).cuda())
    _, _, new = O.az_step(cfg, state, batch)
    rp, rv = O.evaluate(cfg, new["params"], batch["o_t"][:2])
    _, old_v = O.evaluate(cfg, state["params"], batch["o_t"][:2])
    assert np.abs(rv - old_v).max() > 1e-4  # the step moved the values far past the tolerance
    _close(probs.cpu().numpy(), rp, name="probs after step")
    _close_few_values(cfg, new["params"], batch["o_t"][:2], value.cpu().numpy(), rv,
                      "value after step")


def test_largest_accepted_shapes():
    from acme_amd import _lib
    W = _lib.AZ_MAX_WIDTH
    cfg = _cfg(W, (W, W), A_MAX)
    n = _native(cfg, 2, rows=2)
    n.set_params(_params(cfg, 12))
    batch = _batch(cfg, 2, 13)
    _check_step(n, cfg, _state_of(n), batch, tag=" widest")
    p = n.get_params("params")
    probs, value = n.evaluate(torch.as_tensor(batch["o_t"]).cuda())
    rp, rv = O.evaluate(cfg, p, batch["o_t"])
    _close(probs.cpu().numpy(), rp, name="probs widest")
    _close(value.cpu().numpy(), rv, name="value widest")


def test_most_layers_and_rows():
    """ACME_MAX_MLP_LAYERS trunk layers; max_batch and max_eval_rows at ACME_AZ_MAX_ROWS."""
    from acme_amd import _lib
    cfg = _cfg(6, (12,) * _lib.MAX_MLP_LAYERS, 3)
    R = _lib.AZ_MAX_ROWS
    n = _native(cfg, R, rows=R)
    n.set_params(_params(cfg, 14))
    batch = _batch(cfg, R, 15)
    _check_step(n, cfg, _state_of(n), batch, tag=" rows")
    p = n.get_params("params")
    probs, value = n.evaluate(torch.as_tensor(batch["o_t"]).cuda())
    rp, rv = O.evaluate(cfg, p, batch["o_t"])
    _close(probs.cpu().numpy(), rp, name="probs rows")
    _close(value.cpu().numpy(), rv, name="value rows")


def test_save_restore_reproduces_bits():
    from acme_amd.agents.mcts.learning import AZLearner
    from acme_amd.networks import PolicyValueMLP
    from acme_amd.optimizers import Adam
    from acme_amd.replay import ReplaySample, SampleInfo
    net = PolicyValueMLP(10, (50, 50), 5)
    cfg = _cfg(10, (50, 50), 5)
    B = 8
    batches = [_dev(_batch(cfg, B, 40 + i)) for i in range(4)]

    def dataset(order):
        for i in order:
            o_t, r, d, o_tp1, pi = batches[i]
            a = torch.zeros(B, dtype=torch.int32, device="cuda")
            yield ReplaySample(info=SampleInfo(None, None, None, None),
                               data=(o_t, a, r, d, o_tp1, {"pi": pi}))

    from acme_amd.utils import loggers
    mk = lambda order: AZLearner(net, Adam(1e-3), dataset(order), discount=0.99,  # noqa: E731
                                 batch_size=B, seed=3, logger=loggers.NoOpLogger())
    a = mk([0, 1, 2, 3])
    a.step()
    a.step()
    saved = a.save()
    a.step()
    a.step()
    b = mk([2, 3])
    b.restore(saved)
    assert b.num_steps == 2
    b.step()
    b.step()
    torch.cuda.synchronize()
    for w in ("params", "m", "v"):
        x, y = a.native.get_params(w), b.native.get_params(w)
        for k in x:
            np.testing.assert_array_equal(x[k].view(np.uint32), y[k].view(np.uint32), err_msg=k)
    assert a.num_steps == b.num_steps == 4
