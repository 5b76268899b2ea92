"""ORACLE — test infrastructure only.  Never imported by the product package acme_amd.

numpy restatement of the TF DDPG learner step, DDPGLearner._step
(acme/agents/tf/ddpg/learning.py:143-237), in float64 (the accuracy reference) or float32.
It is D4PG's step (oracle/d4pg_oracle.py, whose layers, clips and Adam it imports) with a
scalar critic and the TD loss:

  if num_steps % period == 0: target <- online  (at the START)           :158-160
  num_steps += 1                                                         :161
  q_tm1 = critic(o_tm1, a_tm1); q_t = target_critic(o_t, target_policy(o_t))  [B]  :185-190
  critic_loss = mean(trfl.td_learning(q_tm1, r_t, discount * d_t, q_t).loss)      :193-194
      (trfl is not in the reference tree; restated: target = stop_grad(r + pcont * q_t),
       td = target - q_tm1, loss = 0.5 td^2 — tests/test_ddpg_oracle_cpu.py checks the
       gradients of this form against torch autograd)
  dpg_a_t = policy(o_t); dpg_q_t = critic(o_t, dpg_a_t)                  :197-198
  policy_loss = mean(dpg(dpg_q_t, dpg_a_t, dqda_clipping=1, clip_norm))  :201-208
  policy grads <- policy_loss; critic grads <- critic_loss               :211-219
  tf.clip_by_global_norm(grads, 40) per group when clipping              :226-228
  two snt.Adam(1e-4)                                                     :230-231

Networks: policy = LayerNormMLP(sizes, activate_final=True) -> NearZeroInitializedLinear ->
TanhToSpec (D4PG's); critic = CriticMultiplexer -> LayerNormMLP(critic_sizes + (1,)): the
last linear has no activation and one output, squeezed to [B]
(acme/agents/tf/ddpg/agent_test.py:41-47).
"""

from __future__ import annotations

import dataclasses
from typing import List, Sequence, Tuple

import numpy as np

from oracle.d4pg_oracle import (_lnmlp_shapes, adam_update, clip_grads,  # noqa: F401
                                global_norm_clip, lnmlp_backward, lnmlp_forward,
                                policy_backward, policy_forward, policy_tensor_shapes)


@dataclasses.dataclass
class DDPGConfig:
    obs_dim: int = 24
    act_dim: int = 6
    policy_sizes: Tuple[int, ...] = (256, 256, 256)
    critic_sizes: Tuple[int, ...] = (512, 512, 256)
    action_min: Sequence[float] = (-1.0,) * 6
    action_max: Sequence[float] = (1.0,) * 6
    discount: float = 0.99
    target_update_period: int = 100
    policy_lr: float = 1e-4
    critic_lr: float = 1e-4
    clipping: bool = True
    ln_eps: float = 1e-5


def _head(cfg: DDPGConfig) -> str:
    return f"critic/layer_norm_mlp/mlp/linear_{len(cfg.critic_sizes) - 1}"


def critic_tensor_shapes(cfg: DDPGConfig) -> List[Tuple[str, Tuple[int, ...]]]:
    s = list(cfg.critic_sizes)
    return _lnmlp_shapes("critic", cfg.obs_dim + cfg.act_dim, s) + [
        (_head(cfg) + "/w", (s[-1], 1)), (_head(cfg) + "/b", (1,))]


def ddpg_tensor_shapes(cfg: DDPGConfig):
    """Flat-buffer order of the product learner: policy tensors, then critic tensors."""
    return policy_tensor_shapes(cfg) + critic_tensor_shapes(cfg)


def critic_forward(cfg: DDPGConfig, p, o, a, dtype):
    """q [B] of the scalar critic."""
    f = dtype
    x = np.concatenate([o.astype(f), a.astype(f)], axis=1)
    h, cache = lnmlp_forward(p, "critic", x, len(cfg.critic_sizes), f, cfg.ln_eps)
    q = h @ p[_head(cfg) + "/w"].astype(f) + p[_head(cfg) + "/b"].astype(f)
    cache.update(h_last=h)
    return q[:, 0].astype(f), cache


def critic_backward(cfg: DDPGConfig, p, cache, dq, dtype, want_dx=False):
    """Gradients given dLoss/dq [B]."""
    f = dtype
    dq = dq.astype(f)[:, None]
    g = {_head(cfg) + "/w": cache["h_last"].T @ dq, _head(cfg) + "/b": dq.sum(axis=0)}
    dh = dq @ p[_head(cfg) + "/w"].astype(f).T
    g2, dx = lnmlp_backward(p, "critic", cache, dh, f, want_dx)
    g.update(g2)
    return g, dx


def ddpg_loss_and_grads(cfg: DDPGConfig, params, target, batch, dtype=np.float64):
    f = dtype
    o_tm1, a_tm1 = batch["o_tm1"].astype(f), batch["a_tm1"].astype(f)
    r_t, d_t, o_t = batch["r_t"].astype(f), batch["d_t"].astype(f), batch["o_t"].astype(f)
    B = len(r_t)
    # Critic loss.
    q_tm1, c_cache = critic_forward(cfg, params, o_tm1, a_tm1, f)
    a_targ, _ = policy_forward(cfg, target, o_t, f)
    q_t, _ = critic_forward(cfg, target, o_t, a_targ, f)
    pcont = (f(np.float32(cfg.discount)) * d_t).astype(f)
    td = ((r_t + pcont * q_t) - q_tm1).astype(f)
    critic_loss = (f(0.5) * td * td).mean()
    dq = (-td / B).astype(f)
    cg, _ = critic_backward(cfg, params, c_cache, dq, f)
    # Policy loss: the scalar output is q itself, so d dpg_q / d head output = 1.
    dpg_a, p_cache = policy_forward(cfg, params, o_t, f)
    dpg_q, d_cache = critic_forward(cfg, params, o_t, dpg_a, f)
    dpg_dq = np.ones(B, f)
    _, dx = critic_backward(cfg, params, d_cache, dpg_dq, f, want_dx=True)
    dqda = dx[:, cfg.obs_dim:]
    if cfg.clipping:
        n = np.sqrt((dqda * dqda).sum(axis=1, keepdims=True))
        dqda = dqda * f(1.0) / np.maximum(n, f(1.0))
    policy_loss = (f(0.5) * (dqda * dqda).sum(axis=1)).mean()
    pg = policy_backward(cfg, params, p_cache, (-dqda / B).astype(f), f)
    grads = dict(pg)
    grads.update(cg)
    out = dict(critic_loss=critic_loss, policy_loss=policy_loss, q_tm1=q_tm1, q_t=q_t, td=td,
               dq=np.concatenate([dq, dpg_dq]), dpg_q=dpg_q, dpg_a=dpg_a, a_target=a_targ,
               dqda=dqda)
    return out, grads  # unclipped; ddpg_step applies clip_by_global_norm


def ddpg_step(cfg: DDPGConfig, state: dict, batch: dict, dtype=np.float64):
    """One learner step.  state = {params, target, m, v, num_steps}; the target copy happens
    BEFORE the losses (learning.py:158-161); both Adams step with t = num_steps + 1."""
    target = state["target"]
    if state["num_steps"] % cfg.target_update_period == 0:
        target = {k: v.copy() for k, v in state["params"].items()}
    out, raw = ddpg_loss_and_grads(cfg, state["params"], target, batch, dtype)
    grads, out["norms"] = clip_grads(cfg, raw, dtype)
    t = state["num_steps"] + 1
    new_p, new_m, new_v = {}, {}, {}
    for k in state["params"]:
        lr = cfg.policy_lr if k.startswith("policy/") else cfg.critic_lr
        new_p[k], new_m[k], new_v[k] = adam_update(state["params"][k], grads[k], state["m"][k],
                                                   state["v"][k], t, lr)
    new_state = dict(params=new_p, target=target, m=new_m, v=new_v,
                     num_steps=state["num_steps"] + 1)
    return out, raw, new_state
