"""tests/az_oracle.py against torch autograd in float64: the loss, every gradient and the Adam
update of the AlphaZero step as the reference writes it (acme/agents/tf/mcts/learning.py:53-82),
and the properties the GPU tests lean on."""

import numpy as np
import pytest
import torch

from tests import az_oracle as O


def _setup(activate_final, A=5, B=7, hidden=(6, 9), D=4, seed=0):
    cfg = O.AZConfig(obs_dim=D, hidden=hidden, num_actions=A, activate_final=activate_final,
                     discount=0.9)
    rng = np.random.default_rng(seed)
    params = {n: rng.standard_normal(s) / np.sqrt(s[0]) for n, s in O.az_tensor_shapes(cfg)}
    batch = dict(o_t=rng.standard_normal((B, D)), r_t=rng.standard_normal(B),
                 d_t=(rng.random(B) < 0.8).astype(np.float64),
                 o_tp1=rng.standard_normal((B, D)), pi=rng.dirichlet(np.ones(A), B))
    return cfg, params, batch


def _torch_net(cfg, p, x):
    nl = len(cfg.hidden)
    for i in range(nl):
        x = x @ p[f"mlp/linear_{i}/w"] + p[f"mlp/linear_{i}/b"]
        if i + 1 < nl or cfg.activate_final:
            x = torch.relu(x)
    return x @ p[O.PW] + p[O.PB], (x @ p[O.VW] + p[O.VB])[:, 0]


def _torch_loss(cfg, p, batch, detach_target=True):
    t = {k: torch.as_tensor(v) for k, v in batch.items()}
    logits, v = _torch_net(cfg, p, t["o_t"])
    _, v2 = _torch_net(cfg, p, t["o_tp1"])
    if detach_target:
        v2 = v2.detach()
    value_loss = (t["r_t"] + cfg.discount * t["d_t"] * v2 - v) ** 2
    policy_loss = -(t["pi"] * torch.log_softmax(logits, dim=1)).sum(dim=1)
    return (value_loss + policy_loss).mean(), value_loss.mean(), policy_loss.mean()


@pytest.mark.parametrize("activate_final", [False, True])
def test_loss_and_gradients_match_autograd(activate_final):
    cfg, params, batch = _setup(activate_final)
    p = {k: torch.tensor(v, requires_grad=True) for k, v in params.items()}
    loss, vl, pl = _torch_loss(cfg, p, batch)
    loss.backward()
    out, grads = O.az_loss_and_grads(cfg, params, batch)
    np.testing.assert_allclose(out["loss"], loss.item(), rtol=1e-12)
    np.testing.assert_allclose(out["value_loss"], vl.item(), rtol=1e-12)
    np.testing.assert_allclose(out["policy_loss"], pl.item(), rtol=1e-12)
    assert set(grads) == set(params)
    for k in params:
        np.testing.assert_allclose(grads[k], p[k].grad.numpy().reshape(grads[k].shape),
                                   rtol=1e-10, atol=1e-13, err_msg=k)
    if activate_final:  # the flag changes the function
        other, _ = O.az_loss_and_grads(
            O.AZConfig(**{**cfg.__dict__, "activate_final": False}), params, batch)
        assert abs(other["loss"] - out["loss"]) > 1e-6


def test_no_gradient_through_the_next_observation():
    cfg, params, batch = _setup(False)
    _, grads = O.az_loss_and_grads(cfg, params, batch)
    # The oracle's gradients are autograd's under stop-gradient (the test above) and not those
    # of the loss differentiated through v' as well.
    p = {k: torch.tensor(v, requires_grad=True) for k, v in params.items()}
    _torch_loss(cfg, p, batch, detach_target=False)[0].backward()
    leaked = {k: p[k].grad.numpy() for k in params}
    assert any(np.abs(leaked[k].reshape(grads[k].shape) - grads[k]).max() > 1e-6 for k in params)
    # With every d_t = 0 the target is r alone, so o_tp1 must change nothing at all.
    zero_d = dict(batch, d_t=np.zeros_like(batch["d_t"]))
    other = dict(zero_d, o_tp1=batch["o_tp1"] * 3.0 + 1.0)
    _, g0 = O.az_loss_and_grads(cfg, params, zero_d)
    _, g1 = O.az_loss_and_grads(cfg, params, other)
    for k in params:
        np.testing.assert_array_equal(g0[k], g1[k])


def test_one_action_has_no_policy_loss():
    cfg, params, batch = _setup(False, A=1)
    out, grads = O.az_loss_and_grads(cfg, params, batch)
    assert out["policy_loss"] == 0.0 and (out["ce"] == 0.0).all()
    assert (out["dlogits"] == 0.0).all()
    assert (grads[O.PW] == 0.0).all() and (grads[O.PB] == 0.0).all()
    assert np.abs(grads[O.VW]).max() > 0


def test_adam_matches_torch():
    cfg, params, batch = _setup(False)
    cfg.lr = 1e-2
    p = {k: torch.tensor(v, requires_grad=True) for k, v in params.items()}
    opt = torch.optim.Adam(list(p.values()), lr=cfg.lr, betas=(cfg.b1, cfg.b2), eps=cfg.eps)
    state = O.init_state(params)
    for _ in range(3):
        opt.zero_grad()
        _torch_loss(cfg, p, batch)[0].backward()
        opt.step()
        _, _, state = O.az_step(cfg, state, batch)
    assert state["num_steps"] == 3
    for k in params:
        # torch divides by (sqrt(v) / sqrt(bc2) + eps): the same update to O(eps).
        np.testing.assert_allclose(state["params"][k], p[k].detach().numpy(), rtol=0, atol=1e-7,
                                   err_msg=k)


def test_evaluate_is_the_softmax_of_the_logits():
    cfg, params, batch = _setup(True)
    probs, value = O.evaluate(cfg, params, batch["o_t"])
    q = {k: torch.as_tensor(v) for k, v in params.items()}
    logits, v = _torch_net(cfg, q, torch.as_tensor(batch["o_t"]))
    np.testing.assert_allclose(probs, torch.softmax(logits, dim=1).numpy(), rtol=1e-12)
    np.testing.assert_allclose(value, v.numpy(), rtol=1e-12)
    np.testing.assert_allclose(probs.sum(axis=1), 1.0, rtol=1e-12)


def test_descriptor_matches_the_oracle_layout():
    from acme_amd.networks import PolicyValueMLP
    net = PolicyValueMLP(4, (6, 9), 5)
    cfg = O.AZConfig(obs_dim=4, hidden=(6, 9), num_actions=5)
    assert net.tensor_shapes() == O.az_tensor_shapes(cfg)
    assert net.activate_final is False
    p = net.init(3)
    for name, shape in net.tensor_shapes():
        assert p[name].shape == shape and p[name].dtype == np.float32
        if name.endswith("/b"):
            assert (p[name] == 0).all()
        else:
            assert np.abs(p[name]).max() <= 2.0 / np.sqrt(shape[0]) + 1e-6
    assert net.from_sonnet(net.to_sonnet(p)).keys() == p.keys()
    with pytest.raises(ValueError):
        PolicyValueMLP(4, (), 5)
