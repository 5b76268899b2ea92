"""DMPO oracle (tests/dmpo_oracle.py) checked against a torch-autograd restatement in float64
of DistributionalMPOLearner._step's losses (acme/agents/tf/dmpo/learning.py:183-254: the same
formulas in torch ops, gradients from autograd instead of the oracle's hand-written backward),
against its golden fixture, and against the properties of the bootstrap mixture.  The bar is
tests/test_mpo_oracle_cpu.py's: 1e-10 of each tensor's scale.  Parity with TF / TFP / Sonnet
themselves is UNPINNED (none is installed and the reference holds no DMPO golden value)."""

import os

import numpy as np
import pytest
import torch

from tests import dmpo_oracle as O
from tests.test_mpo_oracle_cpu import (_batch, _eps, _rel, _t_lnmlp, _t_np_kl, _t_policy,
                                       _t_weights_and_temperature_loss)

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "dmpo_step_b8.npz")
MPO_GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "mpo_step_b8.npz")


def _small_cfg(**kw):
    base = dict(obs_dim=5, act_dim=3, policy_sizes=(16, 12, 8), critic_sizes=(20, 12, 8),
                num_samples=4, num_atoms=7, vmin=-2.0, vmax=3.0)
    base.update(kw)
    return O.DMPOConfig(**base)


def _params(cfg, seed, scale=0.5, mean_scale=1.0):
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in O.policy_tensor_shapes(cfg) + O.critic_tensor_shapes(cfg):
        if name.endswith("/scale"):
            out[name] = (1.0 + 0.1 * rng.standard_normal(shape)).astype(np.float32)
        else:
            out[name] = (scale * rng.standard_normal(shape) / np.sqrt(shape[0])).astype(np.float32)
    out[O.HEAD + "/linear/w"] = out[O.HEAD + "/linear/w"] * np.float32(mean_scale)
    for name, v in O.init_duals(cfg).items():
        out[name] = (v + 0.5 * rng.standard_normal(v.shape)).astype(np.float32)
    return out


# ------------------------------------------------------------------ torch restatement


def _t_critic_logits(cfg, p, o, a):
    h = _t_lnmlp(p, "critic", torch.cat([o, a], 1), len(cfg.critic_sizes), cfg.ln_eps)
    return h @ p["critic/discrete_valued_head/linear/w"] + p["critic/discrete_valued_head/linear/b"]


def _t_l2_project(zp, P, zq):
    """acme/tf/losses/distributional.py:44-83 in torch ops."""
    vmin, vmax = zq[0], zq[-1]
    d_pos = torch.cat([zq, vmin[None]])[1:]
    d_neg = torch.cat([vmax[None], zq])[:-1]
    clipped_zp = zp.clamp(vmin, vmax)[:, None, :]
    clipped_zq = zq[None, :, None]
    d_pos = (d_pos - zq)[None, :, None]
    d_neg = (zq - d_neg)[None, :, None]
    delta_qp = clipped_zp - clipped_zq
    d_sign = (delta_qp >= 0).to(P.dtype)
    delta_hat = (d_sign * delta_qp / d_pos) - ((1 - d_sign) * delta_qp / d_neg)
    return ((1 - delta_hat).clamp(0, 1) * P[:, None, :]).sum(2)


def _torch_losses_and_grads(cfg, params, target, batch, eps):
    Normal, kl = torch.distributions.Normal, torch.distributions.kl_divergence
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    tp = {k: torch.tensor(v, dtype=torch.float64) for k, v in target.items()}
    b = {k: torch.tensor(v, dtype=torch.float64) for k, v in batch.items()}
    N, B, K = cfg.num_samples, len(batch["r_t"]), cfg.num_atoms
    e = torch.tensor(eps, dtype=torch.float64)
    values = torch.tensor(O.support(cfg, np.float64))
    on_mean, on_std = _t_policy(cfg, p, b["o_t"])
    with torch.no_grad():
        t_mean, t_std = _t_policy(cfg, tp, b["o_t"])
        actions = t_mean + t_std * e
        o_tiled = b["o_t"].expand(N, *b["o_t"].shape).reshape(N * B, -1)
        sampled_logits = _t_critic_logits(cfg, tp, o_tiled, actions.reshape(N * B, -1))
        sampled_logits = sampled_logits.reshape(N, B, K)
        sampled_logprobs = torch.log_softmax(sampled_logits, dim=-1)              # :216
        averaged_logits = torch.logsumexp(sampled_logprobs, dim=0)                # :217
        sampled_q = (torch.softmax(sampled_logits, -1) * values).sum(-1)          # :232-233
        # losses.categorical's target (stop_gradient)
        z_t = b["r_t"][:, None] + (float(np.float32(cfg.discount)) * b["d_t"])[:, None] * values
        tgt = _t_l2_project(z_t, torch.softmax(averaged_logits, -1), values)
    q_tm1 = _t_critic_logits(cfg, p, b["o_tm1"], b["a_tm1"])
    ce = -(tgt * torch.log_softmax(q_tm1, -1)).sum(-1)
    critic_loss = ce.mean()
    # losses.MPO.__call__
    sp = torch.nn.functional.softplus
    temperature = sp(p["mpo/log_temperature"]) + 1e-8
    alpha_mean = sp(p["mpo/log_alpha_mean"]) + 1e-8
    alpha_stddev = sp(p["mpo/log_alpha_stddev"]) + 1e-8
    w, loss_temperature = _t_weights_and_temperature_loss(sampled_q, cfg.epsilon, temperature)
    kl_np = _t_np_kl(w)
    stats = {}
    if cfg.action_penalization:
        ptemp = sp(p["mpo/log_penalty_temperature"]) + 1e-8
        cost = -torch.linalg.vector_norm(actions - actions.clamp(-1.0, 1.0), dim=-1)
        pw, ploss = _t_weights_and_temperature_loss(cost, cfg.epsilon_penalty, ptemp)
        stats["penalty_kl_q_rel"] = _t_np_kl(pw).mean() / cfg.epsilon_penalty
        w = w + pw
        loss_temperature = loss_temperature + ploss
    target_d = Normal(t_mean, t_std)
    fixed_stddev = Normal(on_mean, t_std)
    fixed_mean = Normal(t_mean, on_std)
    xent = lambda d: (-(d.log_prob(actions).sum(-1) * w).sum(0)).mean()  # noqa: E731
    loss_policy = xent(fixed_stddev) + xent(fixed_mean)
    kl_mean, kl_stddev = kl(target_d, fixed_stddev), kl(target_d, fixed_mean)
    if not cfg.per_dim_constraining:
        kl_mean, kl_stddev = kl_mean.sum(-1, keepdim=True), kl_stddev.sum(-1, keepdim=True)

    def penalty(k, alpha, epsilon):
        m = k.mean(0)
        return (alpha.detach() * m).sum(), (alpha * (epsilon - m.detach())).sum()

    loss_kl_mean, loss_alpha_mean = penalty(kl_mean, alpha_mean, cfg.epsilon_mean)
    loss_kl_stddev, loss_alpha_stddev = penalty(kl_stddev, alpha_stddev, cfg.epsilon_stddev)
    loss = (loss_policy + loss_kl_mean + loss_kl_stddev + loss_alpha_mean + loss_alpha_stddev +
            loss_temperature).sum()
    stats.update({
        "dual_alpha_mean": alpha_mean.mean(), "dual_alpha_stddev": alpha_stddev.mean(),
        "dual_temperature": temperature.mean(), "loss_policy": loss,
        "loss_alpha": (loss_alpha_mean + loss_alpha_stddev), "loss_temperature": loss_temperature.sum(),
        "kl_q_rel": kl_np.mean() / cfg.epsilon,
        "kl_mean_rel": kl_mean.mean(0) / cfg.epsilon_mean,
        "kl_stddev_rel": kl_stddev.mean(0) / cfg.epsilon_stddev,
        "q_min": sampled_q.min(0).values.mean(), "q_max": sampled_q.max(0).values.mean(),
        "pi_stddev_min": on_std.min(-1).values.mean(), "pi_stddev_max": on_std.max(-1).values.mean(),
        "pi_stddev_cond": (on_std.max(-1).values / on_std.min(-1).values).mean()})
    pn = [k for k in p if k.startswith("policy/")]
    cn = [k for k in p if k.startswith("critic/")]
    dn = [k for k in p if k.startswith("mpo/")]
    gp = torch.autograd.grad(loss, [p[k] for k in pn + dn], retain_graph=True)
    gc = torch.autograd.grad(critic_loss, [p[k] for k in cn])
    grads = {k: g.numpy() for k, g in zip(pn + dn + cn, list(gp) + list(gc))}
    extra = dict(sampled_q=sampled_q.numpy(), mixture=torch.softmax(averaged_logits, -1).numpy(),
                 averaged_logits=averaged_logits.numpy(), target_dist=tgt.numpy(),
                 ce=ce.detach().numpy(), z_t=z_t.numpy())
    return (float(critic_loss.detach()), float(loss.detach()),
            {k: v.detach().numpy() for k, v in stats.items()}, grads, extra)


@pytest.mark.parametrize("penal", [True, False])
@pytest.mark.parametrize("per_dim", [True, False])
@pytest.mark.parametrize("seed", [0, 1])
def test_oracle_matches_torch_autograd(seed, per_dim, penal):
    # mean_scale 6: some samples leave [-1, 1], so the penalty weights are not uniform.
    cfg = _small_cfg(per_dim_constraining=per_dim, action_penalization=penal)
    params = _params(cfg, seed, 2.0, 6.0)
    target = _params(cfg, seed + 10, 2.0, 6.0)
    batch, eps = _batch(cfg, 9, seed + 20), _eps(cfg, 9, seed + 30)
    out, g = O.dmpo_loss_and_grads(cfg, params, target, batch, eps, np.float64)
    cl, pl, stats, gt, extra = _torch_losses_and_grads(cfg, params, target, batch, eps)
    # Every branch of the projection runs: below vmin, above vmax, strictly inside.
    z = extra["z_t"]
    assert (z < cfg.vmin).any() and (z > cfg.vmax).any()
    assert ((z > cfg.vmin) & (z < cfg.vmax)).any()
    _rel(out["critic_loss"], cl, 1e-10, "critic_loss")
    _rel(out["policy_loss"], pl, 1e-10, "policy_loss")
    for k, v in extra.items():
        _rel(out[k], v, 1e-10, k)
    assert set(out["stats"]) == set(stats)
    for k, v in stats.items():
        assert np.shape(out["stats"][k]) == np.shape(v) or np.size(v) == 1, k
        _rel(out["stats"][k], v, 1e-10, k)
    assert set(g) == set(gt) == {n for n, _ in O.dmpo_tensor_shapes(cfg)}
    for k in g:
        assert g[k].shape == gt[k].shape, k
        _rel(g[k], gt[k], 1e-10, k)


def test_golden_fixture_reproduces():
    """tests/golden/dmpo_step_b8.npz (made by tests/golden/make_dmpo_golden.py from this oracle)
    regenerates: the inputs bit for bit, the float64 outputs to 1e-12 (they pass through the
    host library's BLAS products).  B = 8, N = 3, K = 5; it stays the size of mpo_step_b8.npz."""
    from tests.golden.make_dmpo_golden import compute, golden_cfg, make_inputs
    z = np.load(GOLDEN)
    cfg = golden_cfg()
    assert (cfg.num_samples, cfg.num_atoms) == (3, 5)
    ins = make_inputs(cfg)
    assert set(ins) == {k for k in z.files if k.startswith("in/")}
    assert ins["in/eps"].shape == (3, 8, 6)
    for k, v in ins.items():
        assert v.dtype == z[k].dtype, k
        np.testing.assert_array_equal(v, z[k], err_msg=k)
    got = compute(cfg, z)
    assert {"out/" + k for k in got} == {k for k in z.files if k.startswith("out/")}
    for k, v in got.items():
        np.testing.assert_allclose(v, z["out/" + k], rtol=1e-12, atol=1e-15, err_msg=k)
    assert z["out/sampled_logits"].shape == (3, 8, 5) and z["out/mixture"].shape == (8, 5)
    assert os.path.getsize(GOLDEN) <= 1.05 * os.path.getsize(MPO_GOLDEN)


# ------------------------------------------------------------------ the mixture


def test_mixture_of_one_sample_is_its_softmax():
    rng = np.random.default_rng(0)
    logits = 3.0 * rng.standard_normal((1, 6, 9))
    mix = O.softmax(O.mixture_logits(logits))
    np.testing.assert_allclose(mix, O.softmax(logits[0]), rtol=1e-14)
    # N = 1 through the whole loss: the step's bootstrap distribution is the sample's softmax.
    cfg = _small_cfg(num_samples=1)
    out, _ = O.dmpo_loss_and_grads(cfg, _params(cfg, 0), _params(cfg, 1), _batch(cfg, 6, 2),
                                   _eps(cfg, 6, 3))
    np.testing.assert_allclose(out["mixture"], O.softmax(out["sampled_logits"][0]), rtol=1e-13)


def test_mixture_sums_to_one_and_is_the_mean_of_the_softmaxes():
    rng = np.random.default_rng(1)
    logits = 4.0 * rng.standard_normal((5, 7, 11))
    lse = O.mixture_logits(logits)
    mix = O.softmax(lse)
    np.testing.assert_allclose(mix.sum(axis=1), 1.0, rtol=1e-14)
    # log N is not subtracted (learning.py:217): exp(lse) sums to N; the softmax removes it.
    np.testing.assert_allclose(np.exp(lse).sum(axis=1), 5.0, rtol=1e-13)
    mean = np.mean([O.softmax(logits[n]) for n in range(5)], axis=0)
    np.testing.assert_allclose(mix, mean, rtol=1e-13)


def test_mixture_of_identical_rows_is_that_row():
    rng = np.random.default_rng(2)
    row = 2.0 * rng.standard_normal((4, 8))
    logits = np.broadcast_to(row[None], (6, 4, 8)).copy()
    np.testing.assert_allclose(O.softmax(O.mixture_logits(logits)), O.softmax(row), rtol=1e-14)


def test_float32_oracle_tracks_float64():
    """The float32 mode (the bar of the GPU tests' derived allowances) stays near float64."""
    cfg = _small_cfg()
    args = (_params(cfg, 0), _params(cfg, 1), _batch(cfg, 6, 2), _eps(cfg, 6, 3))
    o64, g64 = O.dmpo_loss_and_grads(cfg, *args, np.float64)
    o32, g32 = O.dmpo_loss_and_grads(cfg, *args, np.float32)
    assert o32["mixture"].dtype == np.float32 and o32["dlogits"].dtype == np.float32
    _rel(o32["critic_loss"], o64["critic_loss"], 1e-5, "critic_loss")
    for k in g64:
        _rel(g32[k], g64[k], 1e-3, k)
