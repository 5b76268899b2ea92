"""ORACLE — test infrastructure only.  Never imported by the product package acme_amd.

numpy restatement of the TF CRR learner step, RCRRLearner._step
(acme/agents/tf/crr/recurrent_learning.py:197-377), for stateless (feed-forward) networks, in
float64 (the accuracy reference) or float32.  The Gaussian policy is MPO's (tests/mpo_oracle.py),
the bootstrap mixture DMPO's (tests/dmpo_oracle.py), the categorical critic, l2_project and the
global-norm clip D4PG's (oracle/d4pg_oracle.py); all are imported, not copied.

  for t in 1 .. T-1 over the [T, B] sequence (initial_state empty: nothing is carried):  :229-234
    q_tm1 = critic(o_tm1, a_tm1); target distribution at o_t                    :248-251
    a[n] = target.sample(N_td)   (here: mean_t + stddev_t * eps[n], eps an INPUT) :253
    sampled logits [N_td, B, K] = target_critic(tiled o_t, a)                   :256-268
    averaged_logits = logsumexp_n(log_softmax(sampled logits))                  :269-270
    critic_loss_t = mean(categorical(q_tm1, r_t, discount * d_t, q_t))          :273-276
    online distribution at o_tm1; q_tm1_mean = q_tm1.mean()                     :279-281
    a'[n] = online.sample(N_pw); v[n] = critic(tiled o_tm1, a'[n]).mean()       :285-294
    v_estimate = mean / max / min over n                                        :298-303
    policy_loss_batch = -log_prob(a_tm1)                                        :309
    advantage = q_tm1_mean - v_estimate; coef = min(exp(adv / beta), bound) |
        (adv > 0) | 1, behind a stop_gradient                                   :311-320
    policy_loss_t = mean(policy_loss_batch * coef)                              :322-323
  the three sums over t are divided by T (the sequence length, NOT the T - 1 steps) :331-334
  clip_by_global_norm(40) per network; two Adams                                :351-359
  AFTER the update: target <- online when num_steps % period == 0; num_steps += 1 :361-371

Two forms of the losses: `crr_sequence_loss_and_grads` loops over t exactly as above;
`crr_loss_and_grads` takes the R = B (T - 1) transitions the loop unrolls into (row
b (T - 1) + (t - 1)) and sums rows with the scale (T - 1) / (R T).  tests/test_crr_oracle_cpu.py
holds them equal to 1e-12.

The sampling noise is one array eps [N_td + N_pw, R, A]: rows n < N_td sample the target policy
at o_t, the others the online policy at o_tm1.

Third-party semantics restated (TFP is not in the reference tree; parity UNPINNED):
MultivariateNormalDiag.log_prob = sum_d [-0.5 ((x - mu) / sigma)^2 - log sigma] - 0.5 A log(2 pi);
tests/test_crr_oracle_cpu.py checks the formulas below against torch.distributions and autograd.
"""

from __future__ import annotations

import dataclasses
from typing import Tuple

import numpy as np

from oracle.d4pg_oracle import (clip_grads, critic_backward, critic_forward,
                                critic_tensor_shapes, l2_project, softmax, support)
from tests import mpo_oracle as M
from tests.dmpo_oracle import log_softmax, mixture_logits
from tests.mpo_oracle import HEAD, adam_update, policy_tensor_shapes  # noqa: F401

REDUCE = ("mean", "max", "min")
MODES = ("exp", "binary", "all")


@dataclasses.dataclass
class CRRConfig:
    obs_dim: int = 24
    act_dim: int = 6
    policy_sizes: Tuple[int, ...] = (256, 256, 256)
    critic_sizes: Tuple[int, ...] = (512, 512, 256)
    num_atoms: int = 51
    vmin: float = -150.0
    vmax: float = 150.0
    discount: float = 0.99
    target_update_period: int = 100
    num_action_samples_td_learning: int = 1
    num_action_samples_policy_weight: int = 4
    baseline_reduce_function: str = "mean"
    policy_improvement_modes: str = "exp"
    ratio_upper_bound: float = 20.0
    beta: float = 1.0
    sequence_length: int = 2
    policy_lr: float = 1e-4
    critic_lr: float = 1e-4
    clipping: bool = True
    ln_eps: float = 1e-5
    init_scale: float = 0.3
    min_scale: float = 1e-6


def crr_tensor_shapes(cfg: CRRConfig):
    """Flat-buffer order of the product learner: policy, (categorical) critic; no duals."""
    return policy_tensor_shapes(cfg) + critic_tensor_shapes(cfg)


def flatten_sequences(seq):
    """[B, T, ...] -> the R = B (T - 1) transitions, row b (T - 1) + (t - 1)."""
    o, a, r, d = seq["observation"], seq["action"], seq["reward"], seq["discount"]
    B, T = a.shape[:2]
    R = B * (T - 1)
    return dict(o_tm1=o[:, :-1].reshape(R, -1), a_tm1=a[:, :-1].reshape(R, -1),
                r_t=r[:, :-1].reshape(R), d_t=d[:, :-1].reshape(R), o_t=o[:, 1:].reshape(R, -1))


def coefficient(cfg: CRRConfig, advantage, f):
    if cfg.policy_improvement_modes == "exp":
        with np.errstate(over="ignore"):  # an overflowing exp is +inf: the minimum is the bound
            return np.minimum(np.exp(advantage / f(cfg.beta)), f(cfg.ratio_upper_bound)).astype(f)
    if cfg.policy_improvement_modes == "binary":
        return (advantage > 0).astype(f)
    assert cfg.policy_improvement_modes == "all"
    return np.ones_like(advantage)


def _rows_loss_and_grads(cfg: CRRConfig, params, target, batch, eps, div, f):
    """The loop body (:230-323) over the rows of `batch`, every batch mean written as
    sum_rows / div.  Returns the per-row quantities, the three sums and the gradients."""
    o_tm1, a_tm1 = batch["o_tm1"].astype(f), batch["a_tm1"].astype(f)
    r_t, d_t, o_t = batch["r_t"].astype(f), batch["d_t"].astype(f), batch["o_t"].astype(f)
    n, A, K = len(r_t), cfg.act_dim, cfg.num_atoms
    Ntd, Npw = cfg.num_action_samples_td_learning, cfg.num_action_samples_policy_weight
    eps = np.asarray(eps).astype(f).reshape(Ntd + Npw, n, A)
    div = f(div)
    values = support(cfg, f)
    # ---- critic learning
    q_tm1, c_cache = critic_forward(cfg, params, o_tm1, a_tm1, f)                  # :248
    mean_t, std_t, _ = M.policy_forward(cfg, target, o_t, f)                      # :250
    actions_t = (mean_t[None] + std_t[None] * eps[:Ntd]).astype(f)                # :253
    tiled_t = np.broadcast_to(o_t[None], (Ntd, n, o_t.shape[1])).reshape(Ntd * n, -1)
    sl, _ = critic_forward(cfg, target, tiled_t, actions_t.reshape(Ntd * n, A), f)  # :262
    sampled_logits = sl.reshape(Ntd, n, K).astype(f)
    averaged_logits = mixture_logits(sampled_logits).astype(f)                    # :269-270
    disc = (f(np.float32(cfg.discount)) * d_t).astype(f)
    z_t = r_t[:, None] + disc[:, None] * values[None, :]
    mixture = softmax(averaged_logits).astype(f)
    tgt = l2_project(z_t, mixture, values)
    ce = -(tgt * log_softmax(q_tm1)).sum(axis=1)                                  # :275
    critic_sum = ce.sum() / div
    dlogits = ((softmax(q_tm1) - tgt) / div).astype(f)
    cg, _ = critic_backward(cfg, params, c_cache, dlogits, f)
    sampled_q = (softmax(sl) * values[None, :]).sum(axis=1).reshape(Ntd, n).astype(f)
    # ---- actor learning
    mean_on, std_on, p_cache = M.policy_forward(cfg, params, o_tm1, f)            # :279
    q_tm1_mean = (softmax(q_tm1) * values[None, :]).sum(axis=1).astype(f)         # :281
    actions_on = (mean_on[None] + std_on[None] * eps[Ntd:]).astype(f)             # :289
    tiled_tm1 = np.broadcast_to(o_tm1[None], (Npw, n, o_tm1.shape[1])).reshape(Npw * n, -1)
    pl, _ = critic_forward(cfg, params, tiled_tm1, actions_on.reshape(Npw * n, A), f)  # :291
    tiled_v = (softmax(pl) * values[None, :]).sum(axis=1).reshape(Npw, n).astype(f)   # :293
    v_estimate = {"mean": tiled_v.mean, "max": tiled_v.max,
                  "min": tiled_v.min}[cfg.baseline_reduce_function](axis=0).astype(f)
    z = (a_tm1 - mean_on) / std_on
    half_log_2pi = f(0.5 * np.log(2 * np.pi))
    logp = ((f(-0.5) * z * z - np.log(std_on)).sum(axis=-1) - f(A) * half_log_2pi).astype(f)  # :309
    advantage = (q_tm1_mean - v_estimate).astype(f)                               # :311
    coef = coefficient(cfg, advantage, f)                                         # :312-320
    policy_sum = (-logp * coef).sum() / div                                       # :322-323
    coef_sum = coef.sum() / div
    g = (coef / div)[:, None]
    dmean = (-g * z / std_on).astype(f)
    dstd = (g * (1 - z * z) / std_on).astype(f)
    pg, dpre = M.policy_backward(cfg, params, p_cache, dmean, dstd, f)
    grads = dict(pg)
    grads.update(cg)
    out = dict(critic_loss=critic_sum, policy_loss=policy_sum, policy_loss_coef=coef_sum,
               logits_tm1=q_tm1, sampled_logits=sampled_logits,
               policy_sampled_logits=pl.reshape(Npw, n, K), averaged_logits=averaged_logits,
               mixture=mixture, target_dist=tgt, z_t=z_t, ce=ce, dlogits=dlogits,
               sampled_q=sampled_q, actions=np.concatenate([actions_t, actions_on]),
               mean_on=mean_on, std_on=std_on, pre_on=p_cache["pre"], mean_t=mean_t, std_t=std_t,
               q_tm1_mean=q_tm1_mean, tiled_v=tiled_v, v_estimate=v_estimate,
               advantage=advantage, coef=coef, logp=logp, dmean=dmean, dstd=dstd, dpre=dpre)
    return out, grads


def crr_loss_and_grads(cfg: CRRConfig, params, target, batch, eps, dtype=np.float64):
    """Transition form: `batch` holds the R = B (T - 1) rows, eps [N_td + N_pw, R, A]; every
    reference mean is sum_rows (T - 1) / (R T).  Unclipped gradients."""
    R, T = len(batch["r_t"]), cfg.sequence_length
    assert R % (T - 1) == 0
    return _rows_loss_and_grads(cfg, params, target, batch, eps, R * T / (T - 1), dtype)


def crr_sequence_loss_and_grads(cfg: CRRConfig, params, target, seq, eps, dtype=np.float64):
    """Sequence form, the reference's loop: seq = {observation [B, T, od], action [B, T, A],
    reward [B, T], discount [B, T]}; per t the batch means over B, summed over t and divided
    by T.  eps is the transition form's [N, B (T - 1), A].  Returns the three losses and the
    gradients (no per-row quantities)."""
    f = dtype
    B, T = seq["action"].shape[:2]
    assert T == cfg.sequence_length
    N = cfg.num_action_samples_td_learning + cfg.num_action_samples_policy_weight
    eps = np.asarray(eps).reshape(N, B, T - 1, cfg.act_dim)
    losses = dict(critic_loss=f(0), policy_loss=f(0), policy_loss_coef=f(0))
    grads = None
    for t in range(1, T):                                                         # :229
        step = dict(o_tm1=seq["observation"][:, t - 1], a_tm1=seq["action"][:, t - 1],
                    r_t=seq["reward"][:, t - 1], d_t=seq["discount"][:, t - 1],
                    o_t=seq["observation"][:, t])                                 # :230-234
        out, g = _rows_loss_and_grads(cfg, params, target, step, eps[:, :, t - 1], B, f)
        for k in losses:
            losses[k] = losses[k] + out[k]                                        # :327-329
        grads = g if grads is None else {k: grads[k] + g[k] for k in g}
    return ({k: v / f(T) for k, v in losses.items()},                             # :332-334
            {k: v / f(T) for k, v in grads.items()})


def crr_step(cfg: CRRConfig, state: dict, batch: dict, eps, dtype=np.float64):
    """One learner step over the R transitions of `batch`.  state = {params, target, m, v,
    num_steps}; both Adams step with t = num_steps + 1; the target copy follows the update."""
    out, raw = crr_loss_and_grads(cfg, state["params"], state["target"], batch, eps, dtype)
    grads, out["norms"] = clip_grads(cfg, raw, dtype)
    t = state["num_steps"] + 1
    new_p, new_m, new_v = {}, {}, {}
    for k in state["params"]:
        lr = cfg.policy_lr if k.startswith("policy/") else cfg.critic_lr
        new_p[k], new_m[k], new_v[k] = adam_update(state["params"][k], grads[k], state["m"][k],
                                                   state["v"][k], t, lr)
    target = state["target"]
    if state["num_steps"] % cfg.target_update_period == 0:                        # :368-370
        target = {k: np.asarray(v).copy() for k, v in new_p.items()}
    new_state = dict(params=new_p, target=target, m=new_m, v=new_v,
                     num_steps=state["num_steps"] + 1)
    return out, raw, new_state
