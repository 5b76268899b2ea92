"""Numpy restatement of the AlphaZero learner step (AZLearner._step,
acme/agents/tf/mcts/learning.py:53-82) and of the network evaluation the MCTS actor uses
(acting.py:67-77), in the dtype the caller picks (float64 is the reference of the GPU tests).

Network: Flatten -> snt.nets.MLP(hidden, activate_final) -> PolicyValueHead(A): ReLU between
the trunk layers (after the last only with activate_final), logits = h Wp + bp, v = h wv + bv.
Tensor names are the native learner's (include/acme_hip.h, acme_az_*):
  mlp/linear_i/{w,b}, policy_value_network/linear/{w,b}, policy_value_network/linear_1/{w,b}.

Step:  logits, v = net(o_t); _, v' = net(o_tp1) under stop-gradient
       loss = mean_b[(r + discount d v' - v)^2 - sum_a pi log_softmax(logits)_a]
       snt.optimizers.Adam(lr, b1, b2, eps) with t = num_steps + 1.
"""

from __future__ import annotations

import dataclasses
from typing import Dict, Tuple

import numpy as np

PW, PB = "policy_value_network/linear/w", "policy_value_network/linear/b"
VW, VB = "policy_value_network/linear_1/w", "policy_value_network/linear_1/b"


@dataclasses.dataclass
class AZConfig:
    obs_dim: int
    hidden: Tuple[int, ...]
    num_actions: int
    activate_final: bool = False
    discount: float = 0.99
    lr: float = 1e-3
    b1: float = 0.9
    b2: float = 0.999
    eps: float = 1e-8


def az_tensor_shapes(cfg: AZConfig):
    out, d = [], cfg.obs_dim
    for i, h in enumerate(cfg.hidden):
        out += [(f"mlp/linear_{i}/w", (d, h)), (f"mlp/linear_{i}/b", (h,))]
        d = h
    return out + [(PW, (d, cfg.num_actions)), (PB, (cfg.num_actions,)), (VW, (d, 1)), (VB, (1,))]


def forward(cfg: AZConfig, params: Dict[str, np.ndarray], obs, f=np.float64):
    """(logits [rows, A], value [rows], cache) for obs [rows, D]."""
    x = np.asarray(obs, f).reshape(len(obs), -1)
    acts = [x]
    nl = len(cfg.hidden)
    for i in range(nl):
        z = x @ params[f"mlp/linear_{i}/w"].astype(f) + params[f"mlp/linear_{i}/b"].astype(f)
        x = np.maximum(z, 0) if (i + 1 < nl or cfg.activate_final) else z
        acts.append(x)
    logits = x @ params[PW].astype(f) + params[PB].astype(f)
    value = (x @ params[VW].astype(f) + params[VB].astype(f))[:, 0]
    return logits, value, acts


def log_softmax(logits):
    z = logits - logits.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))


def evaluate(cfg: AZConfig, params, obs, f=np.float64):
    """(probs [rows, A], value [rows]): what acme_az_evaluate returns."""
    logits, value, _ = forward(cfg, params, obs, f)
    return np.exp(log_softmax(logits)), value


def az_loss_and_grads(cfg: AZConfig, params, batch, f=np.float64):
    """out (losses and the step's intermediates), grads (one per tensor)."""
    o_t, o_tp1 = np.asarray(batch["o_t"], f), np.asarray(batch["o_tp1"], f)
    r, d, pi = (np.asarray(batch[k], f) for k in ("r_t", "d_t", "pi"))
    B, nl = len(r), len(cfg.hidden)
    logits, v, acts = forward(cfg, params, o_t, f)
    _, v2, _ = forward(cfg, params, o_tp1, f)  # stop-gradient: nothing flows back through it
    td = (r + f(cfg.discount) * d * v2) - v
    logp = log_softmax(logits)
    ce = -(pi * logp).sum(axis=1)
    value_loss, policy_loss = (td * td).mean(), ce.mean()
    dlogits = (np.exp(logp) * pi.sum(axis=1, keepdims=True) - pi) / B
    dv = -2.0 * td / B
    h = acts[-1]
    grads = {PW: h.T @ dlogits, PB: dlogits.sum(axis=0), VW: h.T @ dv[:, None],
             VB: dv.sum(keepdims=True)}
    dh = dlogits @ params[PW].astype(f).T + dv[:, None] * params[VW].astype(f)[:, 0][None, :]
    if cfg.activate_final:
        dh = dh * (h > 0)
    dh_last = dh
    for i in range(nl - 1, -1, -1):
        grads[f"mlp/linear_{i}/w"] = acts[i].T @ dh
        grads[f"mlp/linear_{i}/b"] = dh.sum(axis=0)
        if i > 0:
            dh = (dh @ params[f"mlp/linear_{i}/w"].astype(f).T) * (acts[i] > 0)
    out = dict(loss=value_loss + policy_loss, value_loss=value_loss, policy_loss=policy_loss,
               logits=logits, v=np.concatenate([v, v2]), td=td, dlogits=dlogits, dv=dv,
               dh=dh_last, ce=ce)
    return out, grads


def adam_update(p, g, m, v, t, cfg: AZConfig, f=np.float64):
    """snt.optimizers.Adam, the product kernel's form (oracle/dqn_oracle.py adam_update)."""
    p, g, m, v = (np.asarray(x, f) for x in (p, g, m, v))
    b1, b2, lr, eps = f(cfg.b1), f(cfg.b2), f(cfg.lr), f(cfg.eps)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * (g * g)
    upd = (lr * (m / (1 - b1 ** t))) / (np.sqrt(v / (1 - b2 ** t)) + eps)
    return p - upd, m, v


def init_state(params) -> dict:
    z = lambda: {k: np.zeros_like(np.asarray(p, np.float64)) for k, p in params.items()}  # noqa
    return dict(params={k: np.asarray(p, np.float64) for k, p in params.items()}, m=z(), v=z(),
                num_steps=0)


def az_step(cfg: AZConfig, state: dict, batch: dict, f=np.float64):
    """One learner step.  state = {params, m, v, num_steps}; returns out, grads, new state."""
    out, grads = az_loss_and_grads(cfg, state["params"], batch, f)
    t = state["num_steps"] + 1
    new = dict(params={}, m={}, v={}, num_steps=t)
    for k in state["params"]:
        new["params"][k], new["m"][k], new["v"][k] = adam_update(
            state["params"][k], grads[k], state["m"][k], state["v"][k], t, cfg, f)
    return out, grads, new
