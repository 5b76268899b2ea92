"""CRR oracle (tests/crr_oracle.py) checked against a torch-autograd restatement in float64 of
RCRRLearner._step's losses over the [B, T] sequence form
(acme/agents/tf/crr/recurrent_learning.py:197-334: the same formulas in torch ops with
torch.distributions, gradients from autograd instead of the oracle's hand-written backward),
against its golden fixture, and its sequence form (the reference's loop over t) against its
transition form (what the HIP step computes).  The bar is tests/test_mpo_oracle_cpu.py's: 1e-10
of each tensor's scale.  Parity with TF / TFP / Sonnet themselves is UNPINNED (none is installed
and the reference holds no CRR golden value).

Also here, without a GPU: the conditions tests/test_crr_gpu.py puts on its inputs (the binary
mode's advantage margin, the exp batch that overflows), checked on the oracle's output for the
seeds tests/crr_cases.py fixes."""

import os

import numpy as np
import pytest
import torch

from tests import crr_cases as C
from tests import crr_oracle as O
from tests.test_dmpo_oracle_cpu import _t_critic_logits, _t_l2_project
from tests.test_mpo_oracle_cpu import _rel, _t_policy

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "crr_step_b4.npz")


def _small_cfg(**kw):
    base = dict(obs_dim=5, act_dim=3, policy_sizes=(16, 12, 8), critic_sizes=(20, 12, 8),
                num_atoms=7, vmin=-2.0, vmax=3.0, num_action_samples_td_learning=2,
                num_action_samples_policy_weight=3, sequence_length=4, init_scale=1.0)
    base.update(kw)
    return O.CRRConfig(**base)


def _inputs(cfg, B, seed):
    T = cfg.sequence_length
    return (C.random_params(cfg, seed, 2.0), C.random_params(cfg, seed + 10, 2.0),
            C.sequences(cfg, B, seed + 20, -3.0, 3.0), C.noise(cfg, B * (T - 1), seed + 30))


# ------------------------------------------------------------------ torch restatement


def _torch_losses_and_grads(cfg, params, target, seq, eps):
    """_step over [T, B] tensors, looping over t as the reference does."""
    tfd = torch.distributions
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    tp = {k: torch.tensor(v, dtype=torch.float64) for k, v in target.items()}
    s = {k: torch.tensor(v, dtype=torch.float64).transpose(0, 1) for k, v in seq.items()}  # :199
    T, B = s["reward"].shape
    Ntd, Npw = cfg.num_action_samples_td_learning, cfg.num_action_samples_policy_weight
    K = cfg.num_atoms
    e = torch.tensor(eps, dtype=torch.float64).reshape(Ntd + Npw, B, T - 1, cfg.act_dim)
    values = torch.tensor(O.support(cfg, np.float64))
    discount = float(np.float32(cfg.discount))
    critic_loss = policy_loss = policy_loss_coef = 0.0
    for t in range(1, T):
        o_tm1, a_tm1, r_t, d_t = (s[k][t - 1] for k in ("observation", "action", "reward",
                                                        "discount"))
        o_t = s["observation"][t]
        q_tm1 = _t_critic_logits(cfg, p, o_tm1, a_tm1)
        with torch.no_grad():
            t_mean, t_std = _t_policy(cfg, tp, o_t)
            sampled_actions_t = t_mean + t_std * e[:Ntd, :, t - 1]                # sample(N_td)
            tiled_o_t = o_t.expand(Ntd, *o_t.shape).reshape(Ntd * B, -1)
            sampled_logits = _t_critic_logits(
                cfg, tp, tiled_o_t, sampled_actions_t.reshape(Ntd * B, -1)).reshape(Ntd, B, K)
            averaged_logits = torch.logsumexp(torch.log_softmax(sampled_logits, -1), dim=0)
            z_t = r_t[:, None] + (discount * d_t)[:, None] * values
            tgt = _t_l2_project(z_t, torch.softmax(averaged_logits, -1), values)
        critic_loss_t = (-(tgt * torch.log_softmax(q_tm1, -1)).sum(-1)).mean()
        on_mean, on_std = _t_policy(cfg, p, o_tm1)
        dist = tfd.Independent(tfd.Normal(on_mean, on_std), 1)
        q_tm1_mean = (torch.softmax(q_tm1, -1) * values).sum(-1)
        tiled_o_tm1 = o_tm1.expand(Npw, *o_tm1.shape).reshape(Npw * B, -1)
        action_tm1 = on_mean + on_std * e[Ntd:, :, t - 1]                         # sample(N_pw)
        tiled_z = _t_critic_logits(cfg, p, tiled_o_tm1, action_tm1.reshape(Npw * B, -1))
        tiled_v = (torch.softmax(tiled_z, -1) * values).sum(-1).reshape(Npw, B)
        v = {"mean": lambda x: x.mean(0), "max": lambda x: x.max(0).values,
             "min": lambda x: x.min(0).values}[cfg.baseline_reduce_function](tiled_v)
        policy_loss_batch = -dist.log_prob(a_tm1)
        advantage = q_tm1_mean - v
        if cfg.policy_improvement_modes == "exp":
            coef = torch.minimum(torch.exp(advantage / cfg.beta),
                                 torch.tensor(cfg.ratio_upper_bound, dtype=torch.float64))
        elif cfg.policy_improvement_modes == "binary":
            coef = (advantage > 0).to(torch.float64)
        else:
            coef = torch.ones_like(advantage)
        coef = coef.detach()
        critic_loss = critic_loss + critic_loss_t
        policy_loss = policy_loss + (policy_loss_batch * coef).mean()
        policy_loss_coef = policy_loss_coef + coef.mean()
    critic_loss, policy_loss, policy_loss_coef = (x / T for x in (critic_loss, policy_loss,
                                                                  policy_loss_coef))
    pn = [k for k in p if k.startswith("policy/")]
    cn = [k for k in p if k.startswith("critic/")]
    gc = torch.autograd.grad(critic_loss, [p[k] for k in cn], retain_graph=True)
    gp = torch.autograd.grad(policy_loss, [p[k] for k in pn])
    grads = {k: g.numpy() for k, g in zip(cn + pn, list(gc) + list(gp))}
    return dict(critic_loss=float(critic_loss.detach()), policy_loss=float(policy_loss.detach()),
                policy_loss_coef=float(policy_loss_coef)), grads


@pytest.mark.parametrize("mode", O.MODES)
@pytest.mark.parametrize("reduce", O.REDUCE)
@pytest.mark.parametrize("seed", [0, 1])
def test_oracle_matches_torch_autograd(seed, reduce, mode):
    cfg = _small_cfg(baseline_reduce_function=reduce, policy_improvement_modes=mode)
    params, target, seq, eps = _inputs(cfg, 6, seed)
    losses, g = O.crr_sequence_loss_and_grads(cfg, params, target, seq, eps, np.float64)
    tl, gt = _torch_losses_and_grads(cfg, params, target, seq, eps)
    for k in tl:
        _rel(losses[k], tl[k], 1e-10, k)
    assert set(g) == set(gt) == {n for n, _ in O.crr_tensor_shapes(cfg)}
    for k in g:
        assert g[k].shape == gt[k].shape, k
        _rel(g[k], gt[k], 1e-10, k)
    if mode == "all":
        assert tl["policy_loss_coef"] == pytest.approx((cfg.sequence_length - 1) /
                                                       cfg.sequence_length, rel=1e-14)


@pytest.mark.parametrize("T", [2, 3, 5])
@pytest.mark.parametrize("reduce,mode", [("mean", "exp"), ("max", "binary"), ("min", "all")])
def test_sequence_form_equals_transition_form(T, reduce, mode):
    """The reference's loop over t with per-t batch means, summed and divided by T, against the
    flattened R = B (T - 1) rows with the scale (T - 1) / (R T): losses and gradients to 1e-12."""
    cfg = _small_cfg(sequence_length=T, baseline_reduce_function=reduce,
                     policy_improvement_modes=mode, ratio_upper_bound=2.0)
    params, target, seq, eps = _inputs(cfg, 5, 3)
    ls, gs = O.crr_sequence_loss_and_grads(cfg, params, target, seq, eps)
    batch = O.flatten_sequences(seq)
    assert len(batch["r_t"]) == 5 * (T - 1)
    out, gt = O.crr_loss_and_grads(cfg, params, target, batch, eps)
    for k in ls:
        _rel(out[k], ls[k], 1e-12, k)
    for k in gs:
        _rel(gt[k], gs[k], 1e-12, k)
    if mode == "exp":
        assert (out["coef"] == 2.0).any() and (out["coef"] < 2.0).any()


def test_flatten_order():
    """Row b (T - 1) + (t - 1) is (o[b, t-1], a[b, t-1], r[b, t-1], d[b, t-1], o[b, t])."""
    B, T = 3, 4
    seq = dict(observation=np.arange(B * T * 2, dtype=np.float32).reshape(B, T, 2),
               action=np.arange(B * T, dtype=np.float32).reshape(B, T, 1) + 100,
               reward=np.arange(B * T, dtype=np.float32).reshape(B, T) + 200,
               discount=np.arange(B * T, dtype=np.float32).reshape(B, T) + 300)
    flat = O.flatten_sequences(seq)
    for b in range(B):
        for t in range(1, T):
            i = b * (T - 1) + (t - 1)
            np.testing.assert_array_equal(flat["o_tm1"][i], seq["observation"][b, t - 1])
            np.testing.assert_array_equal(flat["o_t"][i], seq["observation"][b, t])
            assert flat["a_tm1"][i, 0] == seq["action"][b, t - 1, 0]
            assert flat["r_t"][i] == seq["reward"][b, t - 1]
            assert flat["d_t"][i] == seq["discount"][b, t - 1]


def test_step_copies_the_target_after_the_update():
    """Step 0 ends with target == the UPDATED online parameters; a step off the period leaves
    the target alone (recurrent_learning.py:361-371)."""
    cfg = _small_cfg(target_update_period=2, sequence_length=3)
    params, target, seq, eps = _inputs(cfg, 4, 5)
    z = {k: np.zeros_like(v) for k, v in params.items()}
    state = dict(params=params, target=target, m=z, v=dict(z), num_steps=0)
    for s in range(3):
        _, _, new = O.crr_step(cfg, state, O.flatten_sequences(seq), eps)
        for k in params:
            if s % 2 == 0:
                np.testing.assert_array_equal(new["target"][k], new["params"][k])
                assert np.abs(new["target"][k] - state["params"][k]).max() > 0
            else:
                np.testing.assert_array_equal(new["target"][k], state["target"][k])
        state = new
    assert state["num_steps"] == 3


def test_golden_fixture_reproduces():
    """tests/golden/crr_step_b4.npz (made by tests/golden/make_crr_golden.py from this oracle)
    regenerates: the inputs bit for bit, the float64 outputs to 1e-12.  B = 4, T = 3, N_td = 2,
    N_pw = 3, A = 2, K = 5."""
    from tests.golden.make_crr_golden import compute, golden_cfg, make_inputs
    z = np.load(GOLDEN)
    cfg = golden_cfg()
    assert (cfg.num_action_samples_td_learning, cfg.num_action_samples_policy_weight,
            cfg.act_dim, cfg.num_atoms, cfg.sequence_length) == (2, 3, 2, 5, 3)
    ins = make_inputs(cfg)
    assert set(ins) == {k for k in z.files if k.startswith("in/")}
    assert ins["in/action"].shape == (4, 3, 2) and ins["in/eps"].shape == (5, 8, 2)
    for k, v in ins.items():
        assert v.dtype == z[k].dtype, k
        np.testing.assert_array_equal(v, z[k], err_msg=k)
    got = compute(cfg, z)
    assert {"out/" + k for k in got} == {k for k in z.files if k.startswith("out/")}
    for k, v in got.items():
        np.testing.assert_allclose(v, z["out/" + k], rtol=1e-12, atol=1e-15, err_msg=k)
    assert os.path.getsize(GOLDEN) < 64 * 1024


def test_float32_oracle_tracks_float64():
    """The float32 mode (the bar of the GPU tests' derived allowances) stays near float64."""
    cfg = _small_cfg()
    params, target, seq, eps = _inputs(cfg, 6, 0)
    batch = O.flatten_sequences(seq)
    o64, g64 = O.crr_loss_and_grads(cfg, params, target, batch, eps, np.float64)
    o32, g32 = O.crr_loss_and_grads(cfg, params, target, batch, eps, np.float32)
    assert o32["mixture"].dtype == np.float32 and o32["dmean"].dtype == np.float32
    for k in ("critic_loss", "policy_loss", "policy_loss_coef"):
        _rel(o32[k], o64[k], 1e-5, k)
    for k in g64:
        _rel(g32[k], g64[k], 1e-3, k)


# ------------------------------------------------------------------ the GPU tests' inputs


@pytest.mark.parametrize("reduce", O.REDUCE)
def test_binary_inputs_have_an_advantage_margin(reduce):
    cfg, params, target, batch, eps = C.mode_case(reduce, "binary")
    C.assert_projection_branches(cfg, batch)
    out, _ = O.crr_loss_and_grads(cfg, params, target, batch, eps)
    C.assert_binary_margin(cfg, out)
    assert 0 < out["coef"].sum() < len(out["coef"])  # both values of the indicator occur


@pytest.mark.parametrize("reduce", O.REDUCE)
def test_exp_inputs_cross_the_bound(reduce):
    """The nine-combination batch has coefficients on both sides of its bound."""
    cfg, params, target, batch, eps = C.mode_case(reduce, "exp")
    out, _ = O.crr_loss_and_grads(cfg, params, target, batch, eps)
    assert (out["coef"] == cfg.ratio_upper_bound).any()
    assert (out["coef"] < cfg.ratio_upper_bound).any()


def test_overflow_batch_overflows_float32():
    cfg, params, target, batch, eps = C.mode_case("mean", "exp", C.OVERFLOW_SEEDS, **C.OVERFLOW)
    C.assert_projection_branches(cfg, batch)
    out, _ = O.crr_loss_and_grads(cfg, params, target, batch, eps)
    C.assert_overflow_batch(cfg, out)
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp((out["advantage"] / cfg.beta).astype(np.float32))).any()
    # The float32 oracle gives exactly the bound there too.
    o32, _ = O.crr_loss_and_grads(cfg, params, target, batch, eps, np.float32)
    x = out["advantage"] / cfg.beta
    assert (o32["coef"][x > np.log(cfg.ratio_upper_bound) + 1.0] == cfg.ratio_upper_bound).all()
    assert np.isfinite(o32["policy_loss"])
