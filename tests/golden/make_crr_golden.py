"""Generates tests/golden/crr_step_b4.npz: one CRR learner step (B = 4 sequences of T = 3, so
R = 8 transitions; N_td = 2, N_pw = 3 samples, A = 2, K = 5 atoms on [-2, 3], 7-dim
observations, small hidden widths) from the float64 restatement tests/crr_oracle.py (which
tests/test_crr_oracle_cpu.py pins against torch autograd).  The reference's own tests hold no
CRR values, so this fixture pins regressions of the restatement and is the common input of the
CPU and GPU parity tests.

    python -m tests.golden.make_crr_golden
"""

import os

import numpy as np

from tests import crr_oracle as O
from tests.golden.make_mpo_golden import _grid

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "crr_step_b4.npz")
B, T = 4, 3
FIELDS = ("observation", "action", "reward", "discount")
KEYS = ("logits_tm1", "sampled_logits", "policy_sampled_logits", "mixture", "target_dist", "ce",
        "dlogits", "sampled_q", "actions", "mean_on", "std_on", "mean_t", "std_t", "q_tm1_mean",
        "v_estimate", "advantage", "coef", "logp", "dmean", "dpre")


def golden_cfg():
    return O.CRRConfig(obs_dim=7, act_dim=2, policy_sizes=(16, 12), critic_sizes=(24, 16),
                       num_atoms=5, vmin=-2.0, vmax=3.0, num_action_samples_td_learning=2,
                       num_action_samples_policy_weight=3, sequence_length=T,
                       target_update_period=100, init_scale=1.0)


def random_params(cfg, rng):
    out = {}
    for name, shape in O.crr_tensor_shapes(cfg):
        if name.endswith("/scale"):
            v = 1.0 + 0.1 * rng.standard_normal(shape)
        elif name.endswith("/b") or name.endswith("/offset"):
            v = 0.1 * rng.standard_normal(shape)
        else:
            v = rng.standard_normal(shape) / np.sqrt(shape[0])
        out[name] = _grid(v)
    return out


def make_inputs(cfg, seed=0):
    rng = np.random.default_rng(seed)
    z = {}
    for which in ("params", "target"):
        for name, v in random_params(cfg, rng).items():
            z[f"in/{which}/{name}"] = v
    z["in/observation"] = rng.standard_normal((B, T, cfg.obs_dim)).astype(np.float32)
    z["in/action"] = rng.uniform(-1, 1, (B, T, cfg.act_dim)).astype(np.float32)
    z["in/reward"] = rng.uniform(-3, 5, (B, T)).astype(np.float32)
    d = np.full((B, T), 0.99, np.float32)
    d[2, 1] = 0.0
    z["in/discount"] = d
    n = cfg.num_action_samples_td_learning + cfg.num_action_samples_policy_weight
    z["in/eps"] = rng.standard_normal((n, B * (T - 1), cfg.act_dim)).astype(np.float32)
    return z


def unpack(cfg, z):
    names = [n for n, _ in O.crr_tensor_shapes(cfg)]
    params = {n: z[f"in/params/{n}"] for n in names}
    target = {n: z[f"in/target/{n}"] for n in names}
    return params, target, {k: z[f"in/{k}"] for k in FIELDS}, z["in/eps"]


def compute(cfg, z):
    params, target, seq, eps = unpack(cfg, z)
    zeros = {k: np.zeros_like(v) for k, v in params.items()}
    # num_steps = 1: no target copy after the update, Adam t = 2.
    state = dict(params=params, target=target, m=zeros, v=dict(zeros), num_steps=1)
    out, raw, new = O.crr_step(cfg, state, O.flatten_sequences(seq), eps, np.float64)
    res = {k: np.float64(out[k]) for k in ("critic_loss", "policy_loss", "policy_loss_coef")}
    res["norms"] = np.asarray(out["norms"], np.float64)
    for k in KEYS:
        res[k] = out[k]
    for k, g in raw.items():
        res["grad/" + k] = g
    for k, p in new["params"].items():
        res["new/" + k] = p
    return res


def main():
    cfg = golden_cfg()
    z = make_inputs(cfg)
    res = compute(cfg, z)
    z.update({"out/" + k: v for k, v in res.items()})
    np.savez_compressed(OUT, **z)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
