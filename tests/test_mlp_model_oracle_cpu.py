"""The learned-model oracle (tests/mlp_model_oracle.py): its gradients against torch.autograd in
float64, on a shape whose D, widths and A are all odd, with actions inside and outside [0, A);
its forward on such actions; batch_of's index clamp."""

import numpy as np
import torch

from tests import mlp_model_oracle as O


def _setup(seed=0):
    cfg = O.Config(obs_dim=7, hidden=(5, 9), num_actions=3)
    rng = np.random.default_rng(seed)
    params = {k: rng.standard_normal(s) / np.sqrt(s[0]) for k, s in O.tensor_shapes(cfg)}
    return cfg, rng, params


def _towers_on(cfg, params, e):
    """The three towers on a given input e = [obs, one-hot part]."""
    L, outs = len(cfg.hidden) + 1, []
    for tower in O.TOWERS:
        x = e
        for i in range(L):
            x = x @ params[f"{tower}/linear_{i}/w"] + params[f"{tower}/linear_{i}/b"]
            if i + 1 < L:
                x = np.maximum(x, 0)
        outs.append(x)
    return outs[0], outs[1][:, 0], outs[2][:, 0]


def test_oracle_gradients_match_autograd():
    cfg, rng, params = _setup()
    B, D, A, L = 5, cfg.obs_dim, cfg.num_actions, len(cfg.hidden) + 1
    batch = dict(o_t=rng.standard_normal((B, D)), a=rng.integers(0, A, B),
                 r=rng.uniform(-1, 1, B), d=(rng.random(B) < 0.5).astype(np.float64),
                 o_tp1=rng.standard_normal((B, D)))
    for actions in (batch["a"], np.array([-1, 1, A, A + 100, 0])):
        batch["a"] = actions
        out, grads = O.loss_and_grads(cfg, params, batch)

        p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
        inside = torch.tensor((actions >= 0) & (actions < A))
        onehot = torch.nn.functional.one_hot(torch.tensor(np.clip(actions, 0, A - 1)), A).double()
        e = torch.cat([torch.tensor(batch["o_t"]), onehot * inside[:, None]], dim=1)
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


def test_forward_on_actions_inside_and_outside():
    cfg, rng, params = _setup(1)
    D, A = cfg.obs_dim, cfg.num_actions
    obs = rng.standard_normal((6, D))
    inside = np.array([0, 2, 1, 1, 0, 2])
    e = np.concatenate([obs, np.eye(A)[inside]], axis=1)  # the forward as it was
    s, r, x, acts = O.forward(cfg, params, obs, inside)
    for got, ref in zip((s, r, x, acts[O.TOWERS[0]][0]), (*_towers_on(cfg, params, e), e)):
        np.testing.assert_array_equal(got, ref)
    mixed = np.array([-1, 2, A, A + 100, 0, -7])
    e = np.concatenate([obs, np.eye(A)[np.clip(mixed, 0, A - 1)]], axis=1)
    e[(mixed < 0) | (mixed >= A), D:] = 0.0
    assert e[:, D:].sum() == 2.0
    s, r, x, acts = O.forward(cfg, params, obs, mixed)
    for got, ref in zip((s, r, x, acts[O.TOWERS[2]][0]), (*_towers_on(cfg, params, e), e)):
        np.testing.assert_array_equal(got, ref)


def test_batch_of_clamps_indices():
    cfg, rng, _ = _setup(2)
    R = 11
    ring = rng.standard_normal((R, 2 * cfg.obs_dim + 5))
    idx = np.array([-1, 0, 3, R - 1, R, R + 7, -8, 5])
    got = O.batch_of(cfg, ring, idx, clamp=True)
    ref = O.batch_of(cfg, ring, np.clip(idx, 0, R - 1))
    assert got.keys() == ref.keys()
    for k in ref:
        np.testing.assert_array_equal(got[k], ref[k])
    assert (got["o_t"][0] == ring[0, :cfg.obs_dim]).all()  # -1 is row 0, not the last row
    assert (got["o_t"][5] == ring[R - 1, :cfg.obs_dim]).all()
