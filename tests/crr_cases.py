"""The inputs of the CRR parity tests, shared by tests/test_crr_gpu.py (which steps the HIP
learner on them) and tests/test_crr_oracle_cpu.py (which checks, without a GPU, the conditions
the GPU tests put on them).  Test infrastructure only.

The small cases follow tests/test_dmpo_gpu.py: a narrow asymmetric support ([-1, 5] with rewards
in [-3, 5]) so that r + discount d z falls below vmin, above vmax and strictly inside in every
batch; the critic heads scaled 4x and init_scale 1.0, so that the sampled distributions of a
state differ and the advantages are not near-ties.
"""

from __future__ import annotations

import numpy as np

from tests import crr_oracle as O

# (B, T, N_td, N_pw, A, K, steps, target_update_period) of test_steps_match_oracle.
SHAPES = [(5, 2, 1, 4, 3, 51, 1, 100), (19, 3, 3, 2, 6, 21, 1, 100), (8, 2, 1, 64, 1, 64, 1, 100),
          (3, 3, 64, 1, 16, 2, 1, 100), (4, 5, 2, 3, 2, 5, 3, 2)]
# The shape all nine reduce x mode combinations run at.
MODE_SHAPE = (19, 3, 3, 2, 6, 21)
MODE_SEEDS = (3, 30)  # parameters, batch
MODE_BOUND = 2.0       # ratio_upper_bound there: exp's coefficients fall on both sides of it
# The exp batch (mean baseline) whose advantages run past the bound and past the overflow of a
# float32 exp.
OVERFLOW = dict(beta=0.01, ratio_upper_bound=20.0)
OVERFLOW_SEEDS = (12, 73)
F32_EXP_OVERFLOW = 88.73  # exp(x) is +inf in float32 above log(FLT_MAX) = 88.7228


def small_cfg(T, Ntd, Npw, A, K, **kw):
    base = dict(obs_dim=7, act_dim=A, policy_sizes=(36, 100), critic_sizes=(64, 132, 44),
                num_atoms=K, vmin=-1.0, vmax=5.0, init_scale=1.0, sequence_length=T,
                num_action_samples_td_learning=Ntd, num_action_samples_policy_weight=Npw)
    base.update(kw)
    return O.CRRConfig(**base)


def random_params(cfg, seed, critic_scale=4.0):
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in O.crr_tensor_shapes(cfg):
        if name.endswith("/scale"):
            v = 1.0 + 0.1 * rng.standard_normal(shape)
        elif name.endswith("/b") or name.endswith("/offset"):
            v = 0.1 * rng.standard_normal(shape)
        else:
            v = rng.standard_normal(shape) / np.sqrt(shape[0])
        out[name] = v.astype(np.float32)
    k = "critic/discrete_valued_head/linear/w"
    out[k] = out[k] * np.float32(critic_scale)
    return out


def sequences(cfg, B, seed, r_lo=-3.0, r_hi=5.0):
    """[B, T] sequences: rewards spread over [r_lo, r_hi] with one low and one high value
    pinned at t = 0, the last sequence terminal at its first transition (d = 0)."""
    rng = np.random.default_rng(seed)
    T = cfg.sequence_length
    d = np.where(rng.random((B, T)) < 0.05, 0.0, 0.99).astype(np.float32)
    r = rng.uniform(r_lo, r_hi, (B, T)).astype(np.float32)
    r[0, 0], r[min(1, B - 1), T - 2] = r_lo + 0.5, r_hi - 0.5
    d[0, 0] = d[min(1, B - 1), T - 2] = np.float32(0.99)
    d[-1, 0] = 0.0
    return dict(observation=rng.standard_normal((B, T, cfg.obs_dim)).astype(np.float32),
                action=rng.uniform(-1, 1, (B, T, cfg.act_dim)).astype(np.float32),
                reward=r, discount=d)


def noise(cfg, R, seed):
    n = cfg.num_action_samples_td_learning + cfg.num_action_samples_policy_weight
    return np.random.default_rng(seed).standard_normal((n, R, cfg.act_dim)).astype(np.float32)


def assert_projection_branches(cfg, batch):
    """At least one r + discount d z below vmin, one above vmax, a quarter strictly inside, and
    a terminal row."""
    z = O.support(cfg, np.float64)
    zt = batch["r_t"][:, None].astype(np.float64) + \
        (np.float64(np.float32(cfg.discount)) * batch["d_t"].astype(np.float64))[:, None] * z[None]
    assert (zt < cfg.vmin).any() and (zt > cfg.vmax).any()
    assert ((zt > cfg.vmin) & (zt < cfg.vmax)).mean() >= 0.25
    assert (batch["d_t"] == 0).any()


def mode_case(reduce, mode, seeds=MODE_SEEDS, **kw):
    """(cfg, params, target, batch, eps) of one reduce x mode combination."""
    B, T, Ntd, Npw, A, K = MODE_SHAPE
    kw.setdefault("ratio_upper_bound", MODE_BOUND)
    cfg = small_cfg(T, Ntd, Npw, A, K, baseline_reduce_function=reduce,
                    policy_improvement_modes=mode, **kw)
    pseed, bseed = seeds
    batch = O.flatten_sequences(sequences(cfg, B, bseed))
    return (cfg, random_params(cfg, pseed), random_params(cfg, pseed + 1), batch,
            noise(cfg, B * (T - 1), bseed + 100))


def assert_binary_margin(cfg, out):
    """Every row of the oracle's output has |advantage| at least 1e-3 of the support's width:
    the indicator advantage > 0 is then the same in float32 (a condition on the inputs; no row
    is left out of the comparison)."""
    assert np.abs(out["advantage"]).min() >= 1e-3 * (cfg.vmax - cfg.vmin), \
        np.abs(out["advantage"]).min()


def assert_overflow_batch(cfg, out):
    """The exp batch: some advantages above beta log(bound) whose float32 exp is finite, some
    whose float32 exp overflows, some below the bound; the coefficient is exactly the bound on
    the first two.  exp(adv / beta) multiplies the float32 rounding of the advantage (1e-6 of
    the support's width) by 1 / beta = 100, so a coefficient between 0.2 and the bound cannot
    meet a 1e-5 bar whatever computes it: the inputs are chosen so that no row has one (again a
    condition on the inputs, asserted on the oracle's output)."""
    x = out["advantage"] / cfg.beta
    lb = np.log(cfg.ratio_upper_bound)
    assert ((x > lb + 1.0) & (x < F32_EXP_OVERFLOW - 8.0)).any()
    assert (x > F32_EXP_OVERFLOW + 8.0).any()
    assert (x < lb).any()
    assert not ((x > np.log(0.2)) & (x <= lb + 1.0)).any(), np.sort(x)
    assert (out["coef"][x > lb] == cfg.ratio_upper_bound).all()
