"""The IMPALA step on networks.IMPALAMLPNetwork in torch float64 on the CPU: a restatement of
acme/agents/tf/impala/learning.py:97-169 for snt.DeepRNN([Flatten, MLP, LSTM, PolicyValueHead])
through autograd, V-trace (trfl.vtrace_from_importance_weights, both thresholds 1) under
no_grad.  Shared by tests/test_impala_mlp_gpu.py; batch-major [B, T, ...] inputs."""

import numpy as np
import torch


def forward(p, obs, h, c):
    """One network step in float64: (logits, value, h, c, the MLP's hidden pre-activations)."""
    x, pre = obs, []
    nl = sum(1 for k in p if k.startswith("mlp/") and k.endswith("/w"))
    for i in range(nl):
        x = x @ p[f"mlp/linear_{i}/w"] + p[f"mlp/linear_{i}/b"]
        if i + 1 < nl:  # snt.nets.MLP: activate_final=False
            pre.append(x)
            x = torch.relu(x)
    gi, gf, gg, go = (x @ p["lstm/w_i"] + h @ p["lstm/w_h"] + p["lstm/b"]).chunk(4, dim=-1)
    c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)  # forget bias folded into b
    h = torch.sigmoid(go) * torch.tanh(c)
    logits = h @ p["policy_value_network/linear/w"] + p["policy_value_network/linear/b"]
    value = (h @ p["policy_value_network/linear_1/w"] + p["policy_value_network/linear_1/b"])[:, 0]
    return logits, value, h, c, pre


def step(params, batch, discount, entropy_cost, baseline_cost, max_abs_reward=np.inf):
    """batch: observation [B, T, D], action, reward, discount [B, T], logits [B, T, A], h0, c0
    [B, H].  Returns logits, values [B, T], vs, pg_adv [T-1, B], the four losses, the gradients
    per tensor, their global norm and relu_margin: the smallest |hidden pre-activation| over its
    layer's largest."""
    f = lambda x: torch.as_tensor(np.asarray(x, np.float64))  # noqa: E731
    p = {k: f(v).requires_grad_(True) for k, v in params.items()}
    obs, T = f(batch["observation"]), batch["action"].shape[1]
    act = torch.as_tensor(np.asarray(batch["action"], np.int64))[:, :-1]
    h, c = f(batch["h0"]), f(batch["c0"])
    logits, values, margin = [], [], np.inf
    for t in range(T):
        lg, v, h, c, pre = forward(p, obs[:, t], h, c)
        logits.append(lg)
        values.append(v)
        for z in pre:
            margin = min(margin, float(z.detach().abs().min() / z.detach().abs().max()))
    logits, values = torch.stack(logits, 1), torch.stack(values, 1)
    logp = torch.log_softmax(logits[:, :-1], -1)
    lpa = logp.gather(-1, act[..., None])[..., 0]
    with torch.no_grad():
        lmu = torch.log_softmax(f(batch["logits"])[:, :-1], -1).gather(-1, act[..., None])[..., 0]
        rho = torch.exp(lpa - lmu).clamp(max=1.0)  # clipped rhos and cs: both thresholds 1
        r = f(batch["reward"])[:, :-1].clamp(-max_abs_reward, max_abs_reward)
        g = discount * f(batch["discount"])[:, :-1]
        v, boot = values[:, :-1], values[:, -1]
        v1 = torch.cat([v[:, 1:], boot[:, None]], 1)
        deltas = rho * (r + g * v1 - v)
        acc, vs_minus_v = torch.zeros_like(boot), []
        for t in reversed(range(T - 1)):
            acc = deltas[:, t] + g[:, t] * rho[:, t] * acc
            vs_minus_v.append(acc)
        vs = torch.stack(vs_minus_v[::-1], 1) + v
        vs1 = torch.cat([vs[:, 1:], boot[:, None]], 1)
        pg_adv = rho * (r + g * vs1 - v)
    critic = (vs - values[:, :-1]) ** 2
    pg = -lpa * pg_adv
    entropy = (torch.exp(logp) * logp).sum(-1)  # trfl.policy_entropy_loss: minus the entropy
    loss = (pg + baseline_cost * critic + entropy_cost * entropy).mean()
    loss.backward()
    grads = {k: v.grad.numpy() for k, v in p.items()}
    return dict(logits=logits.detach().numpy(), values=values.detach().numpy(),
                vs=vs.numpy().T, pg_adv=pg_adv.numpy().T, grads=grads,
                norm=float(np.sqrt(sum((g * g).sum() for g in grads.values()))),
                losses=np.array([float(x.detach()) for x in
                                 (loss, critic.mean(), entropy.mean(), pg.mean())]),
                relu_margin=margin, clipped_rewards=int((f(batch["reward"])[:, :-1].abs()
                                                         > max_abs_reward).sum()))
