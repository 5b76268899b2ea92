"""MPO oracle (tests/mpo_oracle.py) checked against an independent torch-autograd restatement
of MPOLearner._step's losses (acme/agents/tf/mpo/learning.py:193-238) and of losses.MPO
(acme/tf/losses/mpo.py:145-430) that takes its log-probabilities and KLs from
torch.distributions.Normal, so the two restatements share no formulas, and against the
properties the loss's structure implies.  Parity with TF / TFP / Sonnet themselves is UNPINNED
(none is installed and the reference holds no MPO golden value)."""

import os

import numpy as np
import pytest
import torch

from tests import mpo_oracle as O

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "mpo_step_b8.npz")
DDPG_GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ddpg_step_b8.npz")


def _small_cfg(**kw):
    base = dict(obs_dim=5, act_dim=3, policy_sizes=(16, 12, 8), critic_sizes=(20, 12, 8),
                num_samples=4)
    base.update(kw)
    return O.MPOConfig(**base)


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


def _batch(cfg, B, seed):
    rng = np.random.default_rng(seed)
    return dict(o_tm1=rng.standard_normal((B, cfg.obs_dim)).astype(np.float32),
                a_tm1=rng.uniform(-1, 1, (B, cfg.act_dim)).astype(np.float32),
                r_t=rng.uniform(-3, 3, B).astype(np.float32),
                d_t=np.where(rng.random(B) < 0.2, 0.0, 0.99 ** 4).astype(np.float32),
                o_t=rng.standard_normal((B, cfg.obs_dim)).astype(np.float32))


def _eps(cfg, B, seed):
    return np.random.default_rng(seed).standard_normal(
        (cfg.num_samples, B, cfg.act_dim)).astype(np.float32)


def _state(params, target, num_steps=0):
    z = {k: np.zeros_like(v) for k, v in params.items()}
    return dict(params=params, target=target, m=z, v=dict(z), num_steps=num_steps)


# ------------------------------------------------------------------ torch restatement


def _t_lnmlp(p, prefix, x, n, eps):
    pre = f"{prefix}/layer_norm_mlp"
    z = x @ p[f"{pre}/linear/w"] + p[f"{pre}/linear/b"]
    y = torch.nn.functional.layer_norm(z, (z.shape[1],), p[f"{pre}/layer_norm/scale"],
                                       p[f"{pre}/layer_norm/offset"], eps)
    h = torch.tanh(y)
    for i in range(n - 1):
        h = torch.nn.functional.elu(h @ p[f"{pre}/mlp/linear_{i}/w"] + p[f"{pre}/mlp/linear_{i}/b"])
    return h


def _t_policy(cfg, p, o):
    h = _t_lnmlp(p, "policy", o, len(cfg.policy_sizes), cfg.ln_eps)
    mean = h @ p[O.HEAD + "/linear/w"] + p[O.HEAD + "/linear/b"]
    sp = torch.nn.functional.softplus
    scale = sp(h @ p[O.HEAD + "/linear_1/w"] + p[O.HEAD + "/linear_1/b"])
    scale = scale * (cfg.init_scale / sp(torch.zeros((), dtype=o.dtype))) + cfg.min_scale
    return mean, scale


def _t_critic(cfg, p, o, a):
    n = len(cfg.critic_sizes)
    h = _t_lnmlp(p, "critic", torch.cat([o, a], 1), n, cfg.ln_eps)
    pre = f"critic/layer_norm_mlp/mlp/linear_{n - 1}"
    return (h @ p[pre + "/w"] + p[pre + "/b"]).squeeze(-1)


def _t_weights_and_temperature_loss(q, epsilon, temperature):
    tq = q.detach() / temperature
    w = torch.softmax(tq, dim=0).detach()
    lse = torch.logsumexp(tq, dim=0)
    loss = temperature * (epsilon + lse.mean() - np.log(q.shape[0]))
    return w, loss


def _t_np_kl(w):
    return (w * torch.log(w.shape[0] * w + 1e-8)).sum(0)


def _torch_losses_and_grads(cfg, params, target, batch, eps):
    Normal, kl = torch.distributions.Normal, torch.distributions.kl_divergence
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    tp = {k: torch.tensor(v, dtype=torch.float64) for k, v in target.items()}
    b = {k: torch.tensor(v, dtype=torch.float64) for k, v in batch.items()}
    N, B = cfg.num_samples, len(batch["r_t"])
    e = torch.tensor(eps, dtype=torch.float64)
    on_mean, on_std = _t_policy(cfg, p, b["o_t"])
    with torch.no_grad():
        t_mean, t_std = _t_policy(cfg, tp, b["o_t"])
        actions = t_mean + t_std * e
        o_tiled = b["o_t"].expand(N, *b["o_t"].shape).reshape(N * B, -1)
        sampled_q = _t_critic(cfg, tp, o_tiled, actions.reshape(N * B, -1)).reshape(N, B)
        q_t = sampled_q.mean(0)
        tgt = b["r_t"] + float(np.float32(cfg.discount)) * b["d_t"] * q_t
    q_tm1 = _t_critic(cfg, p, b["o_tm1"], b["a_tm1"])
    critic_loss = (0.5 * (tgt - q_tm1) ** 2).mean()
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
    ce = lambda d: (-(d.log_prob(actions).sum(-1) * w).sum(0)).mean()  # noqa: E731
    loss_policy = ce(fixed_stddev) + ce(fixed_mean)
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
    return (float(critic_loss.detach()), float(loss.detach()),
            {k: v.detach().numpy() for k, v in stats.items()}, grads, w.numpy())


def _rel(a, b, tol, name):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(float(np.abs(b).max()), 1e-300)
    assert float(np.abs(a - b).max()) <= tol * scale, (name, a, b)


@pytest.mark.parametrize("penal", [True, False])
@pytest.mark.parametrize("per_dim", [True, False])
@pytest.mark.parametrize("seed", [0, 1])
def test_oracle_matches_torch_autograd(seed, per_dim, penal):
    # mean_scale 6: some samples leave [-1, 1], so the penalty weights are not uniform.
    cfg = _small_cfg(per_dim_constraining=per_dim, action_penalization=penal)
    params = _params(cfg, seed, 2.0, 6.0)
    target = _params(cfg, seed + 10, 2.0, 6.0)
    batch, eps = _batch(cfg, 9, seed + 20), _eps(cfg, 9, seed + 30)
    out, g = O.mpo_loss_and_grads(cfg, params, target, batch, eps, np.float64)
    cl, pl, stats, gt, w = _torch_losses_and_grads(cfg, params, target, batch, eps)
    _rel(out["critic_loss"], cl, 1e-10, "critic_loss")
    _rel(out["policy_loss"], pl, 1e-10, "policy_loss")
    _rel(out["weights_sum"], w, 1e-10, "weights")
    assert set(out["stats"]) == set(stats)
    for k, v in stats.items():
        assert np.shape(out["stats"][k]) == np.shape(v) or np.size(v) == 1, k
        _rel(out["stats"][k], v, 1e-10, k)
    assert set(g) == set(gt)
    for k in g:
        assert g[k].shape == gt[k].shape, k
        _rel(g[k], gt[k], 1e-10, k)
    if penal:
        assert np.abs(out["penalty_weights"] - 1.0 / cfg.num_samples).max() > 1e-3


def test_stats_are_the_references():
    """Every entry of the reference's stats dict (mpo.py:285-313), the two per-dimension
    vectors with the duals' shape."""
    for per_dim, penal in ((True, True), (False, False)):
        cfg = _small_cfg(per_dim_constraining=per_dim, action_penalization=penal)
        out, _ = O.mpo_loss_and_grads(cfg, _params(cfg, 0), _params(cfg, 1), _batch(cfg, 4, 2),
                                      _eps(cfg, 4, 3))
        want = {"dual_alpha_mean", "dual_alpha_stddev", "dual_temperature", "loss_policy",
                "loss_alpha", "loss_temperature", "kl_q_rel", "kl_mean_rel", "kl_stddev_rel",
                "q_min", "q_max", "pi_stddev_min", "pi_stddev_max", "pi_stddev_cond"}
        if penal:
            want.add("penalty_kl_q_rel")
        assert set(out["stats"]) == want
        d = (cfg.act_dim,) if per_dim else (1,)
        assert out["stats"]["kl_mean_rel"].shape == d
        assert out["stats"]["kl_stddev_rel"].shape == d


def test_weights_sum_to_one_and_two():
    for penal, total in ((False, 1.0), (True, 2.0)):
        cfg = _small_cfg(action_penalization=penal)
        out, _ = O.mpo_loss_and_grads(cfg, _params(cfg, 0, 2.0, 6.0), _params(cfg, 1, 2.0, 6.0),
                                      _batch(cfg, 7, 2), _eps(cfg, 7, 3))
        np.testing.assert_allclose(out["weights"].sum(axis=0), 1.0, rtol=1e-13)
        np.testing.assert_allclose(out["weights_sum"].sum(axis=0), total, rtol=1e-13)


def test_penalty_weights_uniform_in_bounds():
    """Near-zero head weights keep every sample inside [-1, 1]: the cost is 0 everywhere and
    the penalty weights are exactly 1/N."""
    cfg = _small_cfg()
    t = _params(cfg, 1)
    t[O.HEAD + "/linear/w"] *= 0
    t[O.HEAD + "/linear/b"] *= 0
    t[O.HEAD + "/linear_1/w"] *= 0
    t[O.HEAD + "/linear_1/b"] = np.full(cfg.act_dim, -3.0, np.float32)  # stddev ~ 0.02
    out, _ = O.mpo_loss_and_grads(cfg, _params(cfg, 0), t, _batch(cfg, 7, 2), _eps(cfg, 7, 3))
    assert np.abs(out["actions"]).max() < 1.0
    np.testing.assert_array_equal(out["cost"], 0.0)
    np.testing.assert_array_equal(out["penalty_weights"], 1.0 / cfg.num_samples)


def test_kls_vanish_when_online_equals_target():
    """Online == target: both KLs are 0, the KL-penalty gradient vanishes (the policy gradient
    is the cross entropies' alone, whatever the alphas are), and the alphas' gradients are
    epsilon * softplus'."""
    cfg = _small_cfg()
    p = _params(cfg, 0, 2.0)
    batch, eps = _batch(cfg, 6, 2), _eps(cfg, 6, 3)
    out, g = O.mpo_loss_and_grads(cfg, p, p, batch, eps)
    np.testing.assert_array_equal(out["kl_mean"], 0.0)
    np.testing.assert_allclose(out["kl_stddev"], 0.0, atol=1e-15)
    assert out["loss_kl_penalty"] == pytest.approx(0.0, abs=1e-13)
    p2 = dict(p)
    p2["mpo/log_alpha_mean"] = p["mpo/log_alpha_mean"] + 3.0
    p2["mpo/log_alpha_stddev"] = p["mpo/log_alpha_stddev"] - 5.0
    _, g2 = O.mpo_loss_and_grads(cfg, p2, p, batch, eps)
    for k in g:
        if k.startswith("policy/"):
            np.testing.assert_allclose(g2[k], g[k], rtol=1e-9, atol=1e-15, err_msg=k)
    np.testing.assert_allclose(
        g["mpo/log_alpha_mean"],
        cfg.epsilon_mean * O.sigmoid(p["mpo/log_alpha_mean"].astype(np.float64)), rtol=1e-12)


def test_dual_projection_takes_effect():
    """A log-dual below -18 is assigned -18 before use: the loss is the one at -18, and Adam
    moves the projected value (mpo.py:193-199)."""
    cfg = _small_cfg(target_policy_update_period=100, target_critic_update_period=100)
    p, t = _params(cfg, 0), _params(cfg, 1)
    low, at = dict(p), dict(p)
    low["mpo/log_alpha_stddev"] = np.full(cfg.act_dim, -30.0, np.float32)
    low["mpo/log_temperature"] = np.full(1, -18.5, np.float32)
    at["mpo/log_alpha_stddev"] = np.full(cfg.act_dim, -18.0, np.float32)
    at["mpo/log_temperature"] = np.full(1, -18.0, np.float32)
    batch, eps = _batch(cfg, 5, 2), _eps(cfg, 5, 3)
    o1, _, s1 = O.mpo_step(cfg, _state(low, t, 1), batch, eps)
    o2, _, s2 = O.mpo_step(cfg, _state(at, t, 1), batch, eps)
    assert o1["policy_loss"] == o2["policy_loss"]
    for k in p:
        np.testing.assert_array_equal(s1["params"][k], s2["params"][k], err_msg=k)
    # One Adam step of 1e-2 from -18, not from -30.
    assert np.abs(s1["params"]["mpo/log_alpha_stddev"] + 18.0).max() <= 0.0100001
    # kl_stddev > epsilon_stddev here, so the gradient is negative and the value rises.
    assert (s1["params"]["mpo/log_alpha_stddev"] > -18.0).all()


def test_each_target_period_copies_its_own_network():
    cfg = _small_cfg(target_policy_update_period=2, target_critic_update_period=3)
    params, target = _params(cfg, 0), _params(cfg, 5)
    state = _state(params, target)
    batch, eps = _batch(cfg, 4, 1), _eps(cfg, 4, 2)
    prev = state
    for step in range(4):
        _, _, new = O.mpo_step(cfg, prev, batch, eps)
        for k in params:
            if k.startswith("mpo/"):  # the target's dual slots are never written
                np.testing.assert_array_equal(new["target"][k], target[k], err_msg=k)
                continue
            period = 2 if k.startswith("policy/") else 3
            src = prev["params"] if step % period == 0 else prev["target"]
            np.testing.assert_array_equal(new["target"][k], src[k], err_msg=f"{step}/{k}")
        prev = new
    assert prev["num_steps"] == 4


def test_three_adams_and_unclipped_duals():
    """t = num_steps + 1 for all three optimizers; the duals use dual_lr and their raw
    gradients even when the policy's global norm is clipped."""
    cfg = _small_cfg()
    params, target = _params(cfg, 0, 8.0, 6.0), _params(cfg, 5, 2.0, 6.0)
    rng = np.random.default_rng(3)
    m = {k: 0.01 * rng.standard_normal(v.shape) for k, v in params.items()}
    v = {k: 1e-4 * rng.random(p.shape) for k, p in params.items()}
    batch, eps = _batch(cfg, 4, 1), _eps(cfg, 4, 2)
    out, raw, s = O.mpo_step(cfg, dict(params=params, target=target, m=m, v=v, num_steps=4),
                             batch, eps)
    assert out["norms"][0] > 40.0  # the policy gradients are clipped in this case
    clipped, _ = O.clip_grads(cfg, raw, np.float64)
    proj = O.project_duals(O.split_duals(params))
    for k in params:
        if k.startswith("mpo/"):
            want, _, _ = O.adam_update(proj[k], raw[k], m[k], v[k], 5, cfg.dual_lr)
        else:
            want, _, _ = O.adam_update(params[k], clipped[k], m[k], v[k], 5, cfg.policy_lr)
        np.testing.assert_array_equal(s["params"][k], want, err_msg=k)


def test_golden_fixture_reproduces():
    """tests/golden/mpo_step_b8.npz (made by tests/golden/make_mpo_golden.py from this oracle)
    regenerates: the inputs (a seeded generator and float32 casts, eps included) bit for bit,
    the float64 outputs to 1e-12 (they pass through the host library's BLAS products)."""
    from tests.golden.make_mpo_golden import compute, golden_cfg, make_inputs
    z = np.load(GOLDEN)
    cfg = golden_cfg()
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
    assert os.path.getsize(GOLDEN) <= os.path.getsize(DDPG_GOLDEN)


def test_float32_oracle_tracks_float64():
    """The float32 mode (the bar of the GPU tests' derived tolerances) stays near float64."""
    cfg = _small_cfg()
    args = (_params(cfg, 0), _params(cfg, 1), _batch(cfg, 6, 2), _eps(cfg, 6, 3))
    o64, g64 = O.mpo_loss_and_grads(cfg, *args, np.float64)
    o32, g32 = O.mpo_loss_and_grads(cfg, *args, np.float32)
    assert o32["dmean"].dtype == np.float32
    _rel(o32["policy_loss"], o64["policy_loss"], 1e-5, "policy_loss")
    for k in g64:
        _rel(g32[k], g64[k], 1e-3, k)
