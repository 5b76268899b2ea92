"""The learned-model oracle's gradients (tests/mlp_model_oracle.py) against torch.autograd in
float64, on a shape whose D, widths and A are all odd."""

import numpy as np
import torch

from tests import mlp_model_oracle as O


def test_oracle_gradients_match_autograd():
    cfg = O.Config(obs_dim=7, hidden=(5, 9), num_actions=3)
    rng = np.random.default_rng(0)
    B, D, A, L = 5, cfg.obs_dim, cfg.num_actions, len(cfg.hidden) + 1
    params = {k: rng.standard_normal(s) / np.sqrt(s[0]) for k, s in O.tensor_shapes(cfg)}
    batch = dict(o_t=rng.standard_normal((B, D)), a=rng.integers(0, A, B),
                 r=rng.uniform(-1, 1, B), d=(rng.random(B) < 0.5).astype(np.float64),
                 o_tp1=rng.standard_normal((B, D)))
    out, grads = O.loss_and_grads(cfg, params, batch)

    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    e = torch.cat([torch.tensor(batch["o_t"]),
                   torch.nn.functional.one_hot(torch.tensor(batch["a"]), A).double()], dim=1)
    outs = []
    for tower in O.TOWERS:
        x = e
        for i in range(L):
            x = x @ p[f"{tower}/linear_{i}/w"] + p[f"{tower}/linear_{i}/b"]
            if i + 1 < L:
                x = torch.relu(x)
        outs.append(x)
    F = torch.nn.functional
    loss = (F.mse_loss(outs[0], torch.tensor(batch["o_tp1"])) + F.mse_loss(outs[1][:, 0], torch.tensor(batch["r"]))
            + F.binary_cross_entropy_with_logits(outs[2][:, 0], torch.tensor(batch["d"])))
    loss.backward()
    np.testing.assert_allclose(out["loss"], loss.item(), rtol=1e-12)
    for k, g in grads.items():
        ref = p[k].grad.numpy()
        assert np.abs(g - ref).max() <= 1e-10 * np.abs(ref).max(), k
