"""ORACLE — test infrastructure only.  Never imported by the product package acme_amd.

numpy restatement of the TF MPO learner step, MPOLearner._step
(acme/agents/tf/mpo/learning.py:145-260), and of the decoupled MPO loss, losses.MPO.__call__
with its four helpers (acme/tf/losses/mpo.py:145-430), in float64 (the accuracy reference) or
float32.  The LayerNormMLP, the scalar critic, the global-norm clip and Adam are those of
tests/ddpg_oracle.py (imported, not copied).

  if num_steps % target_policy_update_period == 0: target policy <- online  learning.py:159-161
  if num_steps % target_critic_update_period == 0: target critic <- online  :163-165
  num_steps += 1                                                            :168
  online / target distributions on o_t                                      :193-194
  a[n] = target.sample(N)   (here: mean_t + stddev_t * eps[n], eps an INPUT) :197
  sampled_q[n, b] = target_critic(o_t[b], a[n, b]); q_t = mean_n sampled_q  :201-209
  critic_loss = mean(trfl.td_learning(q_tm1, r_t, discount * d_t, q_t).loss) :212-217
      (0.5 (stop_grad(r + pcont q_t) - q_tm1)^2, as tests/ddpg_oracle.py)
  policy_loss, stats = losses.MPO(online, target, a, sampled_q)             :220-224
  clip_by_global_norm(40) on the policy and on the critic gradients; the dual
      gradients are never clipped                                           :244-246
  three snt.Adam: critic, policy (1e-4), duals (1e-2)                       :96-98, 249-251

losses.MPO.__call__ (mpo.py):
  log-duals <- max(-18, log-duals) (an assign, before use)                  :193-199, 226-227
  dual = softplus(log-dual) + 1e-8                                          :203-205, 228-229
  weights, temperature loss (compute_weights_and_temperature_loss)          :216-217, 318-354
  out-of-bound cost -|a - clip(a, -1, 1)|_2, its weights and loss; summed   :224-246
  cross entropies against Normal(online_mean, target_stddev) and
      Normal(target_mean, online_stddev)                                    :250-259, 369-396
  KL(target || fixed-stddev), KL(target || fixed-mean), per dimension or summed :262-271
  alpha-weighted KL penalty and the alphas' dual losses                     :274-277, 399-430
  loss and stats                                                            :280-313

Policy head: MultivariateNormalDiagHead (acme/tf/networks/distributional.py:109-118):
mean = h Wm + bm; stddev = softplus(h Ws + bs) * init_scale / softplus(0) + min_scale.

Third-party semantics restated (TFP is not in the reference tree; parity UNPINNED):
Normal.log_prob = -0.5 ((x - mu) / sigma)^2 - log sigma - 0.5 log(2 pi); KL(N(mu_a, s_a) ||
N(mu_b, s_b)) = (mu_a - mu_b)^2 / (2 s_b^2) + 0.5 ((s_a / s_b)^2 - 1 - 2 log(s_a / s_b));
Independent sums them over the action dimension.  tests/test_mpo_oracle_cpu.py checks the
formulas written out below against torch.distributions and torch autograd.
"""

from __future__ import annotations

import dataclasses
from typing import Dict, List, Tuple

import numpy as np

from tests.ddpg_oracle import (_lnmlp_shapes, adam_update, clip_grads, critic_backward,
                               critic_forward, critic_tensor_shapes, lnmlp_backward,
                               lnmlp_forward)

HEAD = "policy/multivariate_normal_diag_head"
DUAL_EPS = 1e-8       # _MPO_FLOAT_EPSILON
MIN_LOG_DUAL = -18.0  # mpo.py:193-194


@dataclasses.dataclass
class MPOConfig:
    obs_dim: int = 24
    act_dim: int = 6
    policy_sizes: Tuple[int, ...] = (256, 256, 256)
    critic_sizes: Tuple[int, ...] = (512, 512, 256)
    discount: float = 0.99
    num_samples: int = 20
    target_policy_update_period: int = 100
    target_critic_update_period: int = 100
    policy_lr: float = 1e-4
    critic_lr: float = 1e-4
    dual_lr: float = 1e-2
    clipping: bool = True
    ln_eps: float = 1e-5
    # losses.MPO as MPOLearner builds it (learning.py:86-93)
    epsilon: float = 1e-1
    epsilon_penalty: float = 1e-3
    epsilon_mean: float = 1e-3
    epsilon_stddev: float = 1e-6
    init_log_temperature: float = 1.0
    init_log_alpha_mean: float = 1.0
    init_log_alpha_stddev: float = 10.0
    per_dim_constraining: bool = True
    action_penalization: bool = True
    # MultivariateNormalDiagHead
    init_scale: float = 0.3
    min_scale: float = 1e-6


def policy_tensor_shapes(cfg: MPOConfig) -> List[Tuple[str, Tuple[int, ...]]]:
    s = list(cfg.policy_sizes)
    return _lnmlp_shapes("policy", cfg.obs_dim, s) + [
        (HEAD + "/linear/w", (s[-1], cfg.act_dim)), (HEAD + "/linear/b", (cfg.act_dim,)),
        (HEAD + "/linear_1/w", (s[-1], cfg.act_dim)), (HEAD + "/linear_1/b", (cfg.act_dim,))]


def dual_tensor_shapes(cfg: MPOConfig) -> List[Tuple[str, Tuple[int, ...]]]:
    d = cfg.act_dim if cfg.per_dim_constraining else 1
    out = [("mpo/log_temperature", (1,)), ("mpo/log_alpha_mean", (d,)),
           ("mpo/log_alpha_stddev", (d,))]
    if cfg.action_penalization:
        out.append(("mpo/log_penalty_temperature", (1,)))
    return out


def mpo_tensor_shapes(cfg: MPOConfig):
    """Flat-buffer order of the product learner: policy, critic, then the dual variables."""
    return policy_tensor_shapes(cfg) + critic_tensor_shapes(cfg) + dual_tensor_shapes(cfg)


def init_duals(cfg: MPOConfig) -> Dict[str, np.ndarray]:
    """create_dual_variables_once (mpo.py:110-143); the penalty temperature starts at
    init_log_temperature too (:139-143)."""
    init = {"mpo/log_temperature": cfg.init_log_temperature,
            "mpo/log_alpha_mean": cfg.init_log_alpha_mean,
            "mpo/log_alpha_stddev": cfg.init_log_alpha_stddev,
            "mpo/log_penalty_temperature": cfg.init_log_temperature}
    return {k: np.full(s, init[k], np.float32) for k, s in dual_tensor_shapes(cfg)}


def softplus(x):
    return np.logaddexp(x.dtype.type(0), x).astype(x.dtype)


def sigmoid(x):
    return (1 / (1 + np.exp(-x))).astype(x.dtype)


def policy_forward(cfg: MPOConfig, p, o, dtype):
    """mean, stddev [B, A] of the Gaussian head (distributional.py:109-118)."""
    f = dtype
    h, cache = lnmlp_forward(p, "policy", o, len(cfg.policy_sizes), f, cfg.ln_eps)
    mean = h @ p[HEAD + "/linear/w"].astype(f) + p[HEAD + "/linear/b"].astype(f)
    pre = (h @ p[HEAD + "/linear_1/w"].astype(f) + p[HEAD + "/linear_1/b"].astype(f)).astype(f)
    scale = softplus(pre)
    scale = scale * (f(cfg.init_scale) / softplus(np.zeros((), f)))
    scale = (scale + f(cfg.min_scale)).astype(f)
    cache.update(h_last=h, pre=pre)
    return mean.astype(f), scale, cache


def policy_backward(cfg: MPOConfig, p, cache, dmean, dstddev, dtype):
    f = dtype
    dpre = (dstddev * sigmoid(cache["pre"]) * (f(cfg.init_scale) / softplus(np.zeros((), f)))).astype(f)
    h = cache["h_last"]
    g = {HEAD + "/linear/w": h.T @ dmean, HEAD + "/linear/b": dmean.sum(axis=0),
         HEAD + "/linear_1/w": h.T @ dpre, HEAD + "/linear_1/b": dpre.sum(axis=0)}
    dh = dmean @ p[HEAD + "/linear/w"].astype(f).T + dpre @ p[HEAD + "/linear_1/w"].astype(f).T
    g2, _ = lnmlp_backward(p, "policy", cache, dh.astype(f), f)
    g.update(g2)
    return g, dpre


def project_duals(duals: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """The assigns of mpo.py:195-199, 226-227."""
    return {k: np.maximum(np.float32(MIN_LOG_DUAL), v.astype(np.float32)) for k, v in duals.items()}


def _weights_and_temperature_loss(q, epsilon, temperature, f):
    """compute_weights_and_temperature_loss (mpo.py:318-354), q [N, B]; also the loss's
    derivative with respect to the temperature (the weights are behind a stop_gradient, the
    log-sum-exp is not)."""
    N = q.shape[0]
    tq = q / temperature
    mx = tq.max(axis=0, keepdims=True)
    e = np.exp(tq - mx)
    s = e.sum(axis=0, keepdims=True)
    w = (e / s).astype(f)
    lse = (mx + np.log(s))[0]
    inner = f(epsilon) + lse.mean() - np.log(f(N))
    loss = temperature * inner
    dtemp = inner - ((w * tq).sum(axis=0)).mean()
    return w, loss, dtemp


def _nonparametric_kl(w, f):
    """compute_nonparametric_kl_from_normalized_weights (mpo.py:357-366)."""
    return (w * np.log(f(w.shape[0]) * w + f(1e-8))).sum(axis=0)


def mpo_loss(cfg: MPOConfig, duals, mean_on, std_on, mean_t, std_t, actions, q, dtype):
    """losses.MPO.__call__ on projected log-duals.  Returns the loss, the stats, the
    gradients with respect to (mean_on, std_on) and to the log-duals, and the weights."""
    f = dtype
    N, B, A = actions.shape
    ld = {k: v.astype(f) for k, v in duals.items()}
    temperature = softplus(ld["mpo/log_temperature"])[0] + f(DUAL_EPS)
    alpha_mean = softplus(ld["mpo/log_alpha_mean"]) + f(DUAL_EPS)      # [A] or [1]
    alpha_stddev = softplus(ld["mpo/log_alpha_stddev"]) + f(DUAL_EPS)
    w, loss_temperature, dtemp = _weights_and_temperature_loss(q, cfg.epsilon, temperature, f)
    kl_np = _nonparametric_kl(w, f)
    out = dict(weights=w)
    dual_grads = {}
    if cfg.action_penalization:
        ptemp = softplus(ld["mpo/log_penalty_temperature"])[0] + f(DUAL_EPS)
        diff = actions - np.clip(actions, f(-1), f(1))
        cost = -np.sqrt((diff * diff).sum(axis=-1))
        pw, ploss, dptemp = _weights_and_temperature_loss(cost, cfg.epsilon_penalty, ptemp, f)
        pkl_np = _nonparametric_kl(pw, f)
        out.update(penalty_weights=pw, cost=cost)
        w = w + pw
        loss_temperature = loss_temperature + ploss
        dual_grads["mpo/log_penalty_temperature"] = np.asarray(
            [dptemp * sigmoid(ld["mpo/log_penalty_temperature"])[0]], f)
    half_log_2pi = f(0.5 * np.log(2 * np.pi))

    def log_prob(x, mu, sd):
        z = (x - mu) / sd
        return (f(-0.5) * z * z - np.log(sd) - half_log_2pi).sum(axis=-1)

    # compute_cross_entropy_loss (mpo.py:369-396)
    loss_policy_mean = (-(log_prob(actions, mean_on[None], std_t[None]) * w).sum(axis=0)).mean()
    loss_policy_stddev = (-(log_prob(actions, mean_t[None], std_on[None]) * w).sum(axis=0)).mean()
    # KL(target || fixed-stddev) and KL(target || fixed-mean), per dimension [B, A]
    klm = (mean_t - mean_on) ** 2 / (2 * std_t * std_t)
    kls = np.log(std_on / std_t) + std_t * std_t / (2 * std_on * std_on) - f(0.5)
    if cfg.per_dim_constraining:
        kl_mean, kl_stddev = klm, kls                     # [B, A]
    else:
        kl_mean, kl_stddev = klm.sum(axis=1, keepdims=True), kls.sum(axis=1, keepdims=True)
    # compute_parametric_kl_penalty_and_dual_loss (mpo.py:399-430)
    mkl_mean, mkl_stddev = kl_mean.mean(axis=0), kl_stddev.mean(axis=0)
    loss_kl_mean = (alpha_mean * mkl_mean).sum()
    loss_alpha_mean = (alpha_mean * (f(cfg.epsilon_mean) - mkl_mean)).sum()
    loss_kl_stddev = (alpha_stddev * mkl_stddev).sum()
    loss_alpha_stddev = (alpha_stddev * (f(cfg.epsilon_stddev) - mkl_stddev)).sum()
    loss_policy = loss_policy_mean + loss_policy_stddev
    loss_kl_penalty = loss_kl_mean + loss_kl_stddev
    loss_dual = loss_alpha_mean + loss_alpha_stddev + loss_temperature
    loss = loss_policy + loss_kl_penalty + loss_dual
    # Gradients.  The duals see only their dual losses; the policy sees the cross entropies
    # and stop_grad(alpha) * KL.
    dual_grads["mpo/log_temperature"] = np.asarray(
        [dtemp * sigmoid(ld["mpo/log_temperature"])[0]], f)
    dual_grads["mpo/log_alpha_mean"] = (
        (f(cfg.epsilon_mean) - mkl_mean) * sigmoid(ld["mpo/log_alpha_mean"])).astype(f)
    dual_grads["mpo/log_alpha_stddev"] = (
        (f(cfg.epsilon_stddev) - mkl_stddev) * sigmoid(ld["mpo/log_alpha_stddev"])).astype(f)
    wsum = w.sum(axis=0)[:, None]                                   # [B, 1]
    s1 = (w[:, :, None] * (actions - mean_on[None])).sum(axis=0)    # [B, A]
    s2 = (w[:, :, None] * (actions - mean_t[None]) ** 2).sum(axis=0)
    dmean = (-s1 / (std_t * std_t) + alpha_mean * (mean_on - mean_t) / (std_t * std_t)) / B
    dstd = (-(s2 / std_on ** 3 - wsum / std_on)
            + alpha_stddev * (1 / std_on - std_t * std_t / std_on ** 3)) / B
    stats = {
        "dual_alpha_mean": alpha_mean.mean(), "dual_alpha_stddev": alpha_stddev.mean(),
        "dual_temperature": temperature,
        "loss_policy": loss, "loss_alpha": loss_alpha_mean + loss_alpha_stddev,
        "loss_temperature": loss_temperature,
        "kl_q_rel": kl_np.mean() / f(cfg.epsilon),
        "kl_mean_rel": mkl_mean / f(cfg.epsilon_mean),
        "kl_stddev_rel": mkl_stddev / f(cfg.epsilon_stddev),
        "q_min": q.min(axis=0).mean(), "q_max": q.max(axis=0).mean(),
        "pi_stddev_min": std_on.min(axis=-1).mean(), "pi_stddev_max": std_on.max(axis=-1).mean(),
        "pi_stddev_cond": (std_on.max(axis=-1) / std_on.min(axis=-1)).mean(),
    }
    if cfg.action_penalization:
        stats["penalty_kl_q_rel"] = pkl_np.mean() / f(cfg.epsilon_penalty)
    out.update(weights_sum=w, loss_policy_mean=loss_policy_mean,
               loss_policy_stddev=loss_policy_stddev, loss_kl_penalty=loss_kl_penalty,
               kl_mean=kl_mean, kl_stddev=kl_stddev)
    return loss, stats, dmean.astype(f), dstd.astype(f), dual_grads, out


def split_duals(params):
    return {k: v for k, v in params.items() if k.startswith("mpo/")}


def mpo_loss_and_grads(cfg: MPOConfig, params, target, batch, eps, dtype=np.float64):
    """Losses, stats and unclipped gradients; `params` hold projected log-duals."""
    f = dtype
    o_tm1, a_tm1 = batch["o_tm1"].astype(f), batch["a_tm1"].astype(f)
    r_t, d_t, o_t = batch["r_t"].astype(f), batch["d_t"].astype(f), batch["o_t"].astype(f)
    B, N, A = len(r_t), cfg.num_samples, cfg.act_dim
    eps = np.asarray(eps).astype(f).reshape(N, B, A)
    mean_on, std_on, p_cache = policy_forward(cfg, params, o_t, f)
    mean_t, std_t, _ = policy_forward(cfg, target, o_t, f)
    actions = (mean_t[None] + std_t[None] * eps).astype(f)                     # [N, B, A]
    tiled = np.broadcast_to(o_t[None], (N, B, o_t.shape[1])).reshape(N * B, -1)
    sq, _ = critic_forward(cfg, target, tiled, actions.reshape(N * B, A), f)
    sampled_q = sq.reshape(N, B)
    q_t = sampled_q.mean(axis=0).astype(f)
    q_tm1, c_cache = critic_forward(cfg, params, o_tm1, a_tm1, f)
    pcont = (f(np.float32(cfg.discount)) * d_t).astype(f)
    td = ((r_t + pcont * q_t) - q_tm1).astype(f)
    critic_loss = (f(0.5) * td * td).mean()
    dq = (-td / B).astype(f)
    cg, _ = critic_backward(cfg, params, c_cache, dq, f)
    loss, stats, dmean, dstd, dg, extra = mpo_loss(cfg, split_duals(params), mean_on, std_on,
                                                   mean_t, std_t, actions, sampled_q, f)
    pg, dpre = policy_backward(cfg, params, p_cache, dmean, dstd, f)
    grads = dict(pg)
    grads.update(cg)
    grads.update(dg)
    out = dict(critic_loss=critic_loss, policy_loss=loss, stats=stats, q_tm1=q_tm1, q_t=q_t,
               sampled_q=sampled_q, td=td, dq=dq, actions=actions, mean_on=mean_on,
               std_on=std_on, mean_t=mean_t, std_t=std_t, dmean=dmean, dstd=dstd, dpre=dpre)
    out.update(extra)
    return out, grads


def mpo_step(cfg: MPOConfig, state: dict, batch: dict, eps, dtype=np.float64):
    """One learner step.  state = {params, target, m, v, num_steps}, the duals being entries
    of params / m / v (and unused entries of target).  Both target copies happen BEFORE the
    losses; the three Adams step with t = num_steps + 1; the dual projection is an assign, so
    Adam updates the projected values."""
    target = dict(state["target"])
    if state["num_steps"] % cfg.target_policy_update_period == 0:
        target.update({k: v.copy() for k, v in state["params"].items() if k.startswith("policy/")})
    if state["num_steps"] % cfg.target_critic_update_period == 0:
        target.update({k: v.copy() for k, v in state["params"].items() if k.startswith("critic/")})
    params = dict(state["params"])
    params.update(project_duals(split_duals(params)))
    out, raw = mpo_loss_and_grads(cfg, params, target, batch, eps, dtype)
    grads, out["norms"] = clip_grads(cfg, raw, dtype)   # policy/ and critic/ only
    grads.update(split_duals(raw))                      # never clipped
    t = state["num_steps"] + 1
    new_p, new_m, new_v = {}, {}, {}
    for k in params:
        lr = cfg.policy_lr if k.startswith("policy/") else \
            cfg.critic_lr if k.startswith("critic/") else cfg.dual_lr
        new_p[k], new_m[k], new_v[k] = adam_update(params[k], grads[k], state["m"][k],
                                                   state["v"][k], t, lr)
    new_state = dict(params=new_p, target=target, m=new_m, v=new_v,
                     num_steps=state["num_steps"] + 1)
    return out, raw, new_state
