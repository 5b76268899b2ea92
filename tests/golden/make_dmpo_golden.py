"""Generates tests/golden/dmpo_step_b8.npz: one distributional MPO learner step (B = 8, N = 3
samples, K = 5 atoms on [-2, 3], 24-dim observations, 6-dim actions, the reduced hidden widths of
mpo_step_b8.npz) from the float64 restatement tests/dmpo_oracle.py (which
tests/test_dmpo_oracle_cpu.py pins against torch autograd).  The reference's own tests hold no
DMPO values, so this fixture pins regressions of the restatement and is the common input of the
CPU and GPU parity tests.  Inputs are drawn as for mpo_step_b8.npz; the narrow asymmetric
support with rewards in [0, 5] puts projected atoms below vmin, above vmax and inside.

    python -m tests.golden.make_dmpo_golden
"""

import os

import numpy as np

from tests import dmpo_oracle as O
from tests.golden.make_mpo_golden import _grid

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dmpo_step_b8.npz")


def golden_cfg():
    return O.DMPOConfig(obs_dim=24, act_dim=6, policy_sizes=(32, 32, 32),
                        critic_sizes=(64, 64, 32), num_samples=3, num_atoms=5, vmin=-2.0,
                        vmax=3.0, target_policy_update_period=100,
                        target_critic_update_period=100)


def random_params(cfg, rng):
    out = {}
    for name, shape in O.policy_tensor_shapes(cfg) + O.critic_tensor_shapes(cfg):
        if name.endswith("/scale"):
            v = 1.0 + 0.1 * rng.standard_normal(shape)
        elif name.endswith("/b") or name.endswith("/offset"):
            v = 0.1 * rng.standard_normal(shape)
        else:
            v = rng.standard_normal(shape) / np.sqrt(shape[0])
        out[name] = _grid(v)
    for name, v in O.init_duals(cfg).items():
        out[name] = _grid(v + 0.3 * rng.standard_normal(v.shape))
    return out


def make_inputs(cfg, B=8, seed=0):
    rng = np.random.default_rng(seed)
    z = {}
    for which in ("params", "target"):
        for name, v in random_params(cfg, rng).items():
            z[f"in/{which}/{name}"] = v
    z["in/o_tm1"] = rng.standard_normal((B, cfg.obs_dim)).astype(np.float32)
    z["in/a_tm1"] = rng.uniform(-1, 1, (B, cfg.act_dim)).astype(np.float32)
    z["in/r_t"] = rng.uniform(-3, 5, B).astype(np.float32)
    d = np.full(B, 0.99 ** 4, np.float32)
    d[3] = 0.0
    z["in/d_t"] = d
    z["in/o_t"] = rng.standard_normal((B, cfg.obs_dim)).astype(np.float32)
    z["in/eps"] = rng.standard_normal((cfg.num_samples, B, cfg.act_dim)).astype(np.float32)
    return z


def unpack(cfg, z):
    names = [n for n, _ in O.dmpo_tensor_shapes(cfg)]
    params = {n: z[f"in/params/{n}"] for n in names}
    target = {n: z[f"in/target/{n}"] for n in names}
    batch = {k: z[f"in/{k}"] for k in ("o_tm1", "a_tm1", "r_t", "d_t", "o_t")}
    return params, target, batch, z["in/eps"]


def compute(cfg, z):
    params, target, batch, eps = unpack(cfg, z)
    zeros = {k: np.zeros_like(v) for k, v in params.items()}
    # num_steps = 1: neither target copy happens, Adam t = 2.
    state = dict(params=params, target=target, m=zeros, v=dict(zeros), num_steps=1)
    out, raw, new = O.dmpo_step(cfg, state, batch, eps, np.float64)
    res = {"critic_loss": np.float64(out["critic_loss"]),
           "policy_loss": np.float64(out["policy_loss"]),
           "norms": np.asarray(out["norms"], np.float64)}
    for k in ("logits_tm1", "sampled_logits", "mixture", "target_dist", "ce", "dlogits",
              "sampled_q", "actions", "mean_on", "std_on", "mean_t", "std_t", "weights",
              "penalty_weights", "dmean", "dpre"):
        res[k] = out[k]
    for k, v in out["stats"].items():
        res["stats/" + k] = np.asarray(v, np.float64)
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
