"""The R2D2 step on networks.R2D2MLPNetwork in torch float64 on the CPU: a restatement of
acme/agents/tf/r2d2/learning.py:112-200 for snt.DeepRNN([Flatten, LSTM, MLP]) through autograd.
The loss arithmetic is oracle/r2d2_oracle.py's (transformed_loss, compute_priority,
importance_weights).  Shared by tests/test_r2d2_mlp_*.py; batch-major [B, T, ...] inputs."""

import numpy as np
import torch

from oracle import r2d2_oracle as O


def forward(p, obs, h, c):
    """One network step in float64: (q, h, c, the MLP's hidden pre-activations)."""
    gi, gf, gg, go = (obs @ p["lstm/w_i"] + h @ p["lstm/w_h"] + p["lstm/b"]).chunk(4, dim=-1)
    c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)  # forget bias folded into b
    h = torch.sigmoid(go) * torch.tanh(c)
    x, pre = h, []
    nl = sum(1 for k in p if k.startswith("mlp/") and k.endswith("/w"))
    for i in range(nl):
        x = x @ p[f"mlp/linear_{i}/w"] + p[f"mlp/linear_{i}/b"]
        if i + 1 < nl:  # snt.nets.MLP: activate_final=False
            pre.append(x)
            x = torch.relu(x)
    return x, h, c, pre


def unroll(cfg, p, batch):
    """q [L, B, A] over the suffix (time-major) from the stored core state, the burn-in outside
    the tape (learning.py:134-137), and the hidden pre-activations of the suffix."""
    f = lambda x: torch.as_tensor(np.asarray(x, np.float64))  # noqa: E731
    obs = f(batch["observation"])
    B, T = batch["action"].shape
    H = p["lstm/w_h"].shape[0]
    if cfg.store_lstm_state:
        h, c = f(batch["h0"]), f(batch["c0"])
    else:
        h, c = torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64)
    q, pres = [], []
    for t in range(T):
        if t == cfg.burn_in_length:
            h, c = h.detach(), c.detach()
        x, h, c, pre = forward(p, obs[:, t].reshape(B, -1), h, c)
        if t >= cfg.burn_in_length:
            q.append(x)
            pres += pre
    return torch.stack(q, 0), pres


def step(cfg, params, target, batch, g=None):
    """cfg: an oracle.r2d2_oracle.R2D2Config (num_actions, burn_in_length, n_step, discount, the
    replay numbers, store_lstm_state).  Returns q / target_q [L, B, A], the float64 errors
    [L - 1, B], loss, priorities, the gradients per tensor of sum_{t, b} g[t, b] q[t, b, a_t]
    (g [L - 1, B]: d loss / d q[a]; None: the oracle's own) and two margins: relu_margin, the
    smallest |hidden pre-activation| of the online network over its layer's largest, and q_gap,
    the smallest gap between the two largest online q values of a suffix row over the q scale."""
    f = lambda x: torch.as_tensor(np.asarray(x, np.float64))  # noqa: E731
    p = {k: f(v).requires_grad_(True) for k, v in params.items()}
    q, pres = unroll(cfg, p, batch)
    with torch.no_grad():
        tq, _ = unroll(cfg, {k: f(v) for k, v in target.items()}, batch)
    qn, tqn = q.detach().numpy(), tq.numpy()
    errors, _ = O.transformed_loss(cfg, qn, tqn, batch, np.float64)
    w = O.importance_weights(np.asarray(batch["probabilities"]), cfg.max_replay_size,
                             cfg.importance_sampling_exponent).astype(np.float64)
    B = errors.shape[1]
    if g is None:
        g = errors * w[None, :] / B
    act = torch.as_tensor(np.asarray(batch["action"], np.int64))[:, cfg.burn_in_length:].T
    qa = q[:-1].gather(-1, act[:-1, :, None])[..., 0]
    (qa * f(g)).sum().backward()
    top = np.sort(qn, axis=-1)
    margin = min([float(z.detach().abs().min() / z.detach().abs().max()) for z in pres] + [np.inf])
    return dict(q=qn, target_q=tqn, errors=errors,
                loss=float(np.mean(0.5 * np.sum(errors ** 2, axis=0) * w)),
                priorities=O.compute_priority(errors.astype(np.float32), cfg.max_priority_weight),
                grads={k: v.grad.numpy() for k, v in p.items()}, relu_margin=margin,
                q_gap=float((top[..., -1] - top[..., -2]).min() / np.abs(qn).max()))
