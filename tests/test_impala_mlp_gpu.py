"""The IMPALA step on IMPALAMLPNetwork (acme_impala_mlp_*: three launches) and its one-launch
policy step against the float64 oracle (tests/impala_mlp_oracle.py), at DESIGN.md 5.3's bars:
  logits, values, vs, pg advantages, losses, norm: rtol 1e-5 + 2e-6 x the tensor's largest value
  gradients, per tensor: |g - g_ref| <= 1e-4 |g_ref| + 2e-5 max|g_ref|
  Adam applied to the kernel's own (clipped) gradients, in float32 as snt.Adam runs it: 1e-6.
"""

import functools

import numpy as np
import pytest
import torch

from acme_amd.networks import IMPALAMLPNetwork
from tests import impala_mlp_oracle as oracle

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
GAMMA, ENTROPY_COST, BASELINE_COST = 0.97, 0.01, 0.5

# (obs, hidden, H, A, B, T, max_abs_reward, max_gradient_norm, seed): every dimension off the
# 4-wide k step and the 16-wide tile with one live row and one loss step; the reference example
# on exactly one tile; three layers and a second tile with one live row (rewards clipped); the
# width limits over three tiles (the norm clipped).  The seeds were chosen on the CPU: no hidden
# pre-activation of the oracle within 1e-5 of its layer's scale of zero.
CASES = [(5, (7,), 3, 2, 1, 2, None, None, 0),
         (10, (50, 50), 20, 3, 16, 3, None, None, 0),
         (33, (17, 40, 9), 20, 5, 17, 5, 0.5, None, 0),
         (64, (256,), 128, 64, 37, 20, None, 0.05, 0)]


def _net(i):
    D, hidden, H, A = CASES[i][:4]
    return IMPALAMLPNetwork(D, hidden, H, A)


def _data(i, B=None, T=None):
    """Parameters and a batch: a nonzero core state, behaviour logits of their own, zeros among
    the discounts in mid-sequence."""
    D, hidden, H, A, B0, T0, _, _, seed = CASES[i]
    B, T = B or B0, T or T0
    rng = np.random.default_rng(1000 * seed + 7 * B + T)
    params = {k: (0.1 * rng.standard_normal(s) if k.endswith("/b") else
                  rng.standard_normal(s) / np.sqrt(s[0])).astype(np.float32)
              for k, s in _net(i).tensor_shapes()}
    disc = (rng.random((B, T)) > 0.25).astype(np.float32)
    disc[:, T // 2] = 0.0 if T > 2 else disc[:, T // 2]
    batch = dict(observation=rng.standard_normal((B, T, D)).astype(np.float32),
                 action=rng.integers(0, A, (B, T)).astype(np.int32),
                 reward=rng.standard_normal((B, T)).astype(np.float32), discount=disc,
                 logits=rng.standard_normal((B, T, A)).astype(np.float32),
                 h0=(0.5 * rng.standard_normal((B, H))).astype(np.float32),
                 c0=(0.5 * rng.standard_normal((B, H))).astype(np.float32))
    return params, batch


@functools.lru_cache(None)
def _reference(i):
    params, batch = _data(i)
    ref = oracle.step(params, batch, GAMMA, ENTROPY_COST, BASELINE_COST,
                      np.inf if CASES[i][6] is None else CASES[i][6])
    assert ref["relu_margin"] > 1e-5, ref["relu_margin"]
    return ref


def _native(i, B=None, T=None):
    from acme_amd.native import NativeIMPALAMLP
    D, hidden, H, A, B0, T0, clip_r, clip_g, _ = CASES[i]
    return NativeIMPALAMLP(obs_dim=D, hidden=hidden, lstm_size=H, num_actions=A,
                           max_batch=B or B0, max_sequence_length=T or T0, discount=GAMMA,
                           entropy_cost=ENTROPY_COST, baseline_cost=BASELINE_COST,
                           max_abs_reward=clip_r, max_gradient_norm=clip_g, learning_rate=LR,
                           adam_beta1=B1, adam_beta2=B2, adam_epsilon=EPS)


def _step(n, batch):
    d = {k: torch.as_tensor(v).cuda() for k, v in batch.items()}
    n.step(d["observation"], d["action"], d["reward"], d["discount"], d["logits"], d["h0"],
           d["c0"])
    torch.cuda.synchronize()


def _state(n):
    """Everything a step writes, as bytes-comparable arrays."""
    out = {w + "/" + k: v for w in ("params", "grads", "m", "v")
           for k, v in n.get_params(w).items()}
    out["metrics"] = n.metrics.cpu().numpy()
    for name in ("pv", "dpv", "vs", "pg_adv", "h", "grad_norm"):
        out[name] = n.debug_buffer(name)
    return out


def _close(got, ref, name):
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    scale = float(np.abs(ref).max())
    print(f"{name}: max |err| {float(np.abs(got - ref).max()):.3e}, scale {scale:.3e}")
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=2e-6 * scale, err_msg=name)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_step_matches_oracle(i):
    A, clip_r, clip_g = CASES[i][3], CASES[i][6], CASES[i][7]
    params, batch = _data(i)
    ref = _reference(i)
    if clip_r is not None:
        assert ref["clipped_rewards"] > 0
    if clip_g is not None:
        assert ref["norm"] > clip_g  # clipping binds
    n = _native(i)
    n.set_params(params)
    _step(n, batch)
    pv = n.debug_buffer("pv").reshape(ref["values"].shape + (A + 1,))
    _close(pv[..., :A], ref["logits"], "logits")
    _close(pv[..., A], ref["values"], "values")
    _close(n.debug_buffer("vs"), ref["vs"], "vs")
    _close(n.debug_buffer("pg_adv"), ref["pg_adv"], "pg_adv")
    _close(n.metrics.cpu().numpy(), ref["losses"], "losses")
    norm = float(n.debug_buffer("grad_norm")[0])
    _close([norm], [ref["norm"]], "norm")
    grads = n.get_params("grads")
    for k, g_ref in ref["grads"].items():
        err = np.abs(grads[k].astype(np.float64) - g_ref)
        bar = 1e-4 * np.abs(g_ref) + 2e-5 * np.abs(g_ref).max()
        print(f"{k}: worst err / bar {float((err / bar).max()):.3f}")
        assert (err <= bar).all(), k
    # snt.Adam in float32 at t = 1 from zero moments, on the kernel's own clipped gradients.
    f, one = np.float32, np.float32(1)
    clip = f(1e10 if clip_g is None else clip_g)
    scale = clip * min(one / f(norm), one / clip)
    got = n.get_params("params")
    for k, g in grads.items():
        g = g * scale
        m, v = (one - f(B1)) * g, (one - f(B2)) * (g * g)
        upd = (f(LR) * (m / (one - f(B1)))) / (np.sqrt(v / (one - f(B2))) + f(EPS))
        np.testing.assert_allclose(got[k], params[k] - upd, rtol=1e-6, atol=1e-9, err_msg=k)


def test_step_repeats_bit_for_bit():
    params, batch = _data(2)
    runs = []
    for _ in range(2):
        n = _native(2)
        n.set_params(params)
        _step(n, batch)
        runs.append(_state(n))
    for k, v in runs[0].items():
        assert v.tobytes() == runs[1][k].tobytes(), k


def test_small_step_after_large_equals_fresh_learner():
    params, big = _data(3)
    _, small = _data(3, 5, 4)
    used, fresh = _native(3), _native(3, 5, 4)
    used.set_params(params)
    _step(used, big)
    start = used.get_params("params")
    fresh.set_params(start)
    for w in ("m", "v"):
        fresh._copy_in(getattr(fresh, w), used.get_params(w))  # noqa: SLF001
    fresh.num_steps = used.num_steps
    _step(used, small)
    _step(fresh, small)
    a, b = _state(used), _state(fresh)
    for k, v in a.items():
        assert v.tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("rows", [1, 17])
def test_policy_step_matches_oracle(rows):
    i = 2
    D, _, H, A = CASES[i][:4]
    params, _ = _data(i)
    rng = np.random.default_rng(rows)
    obs, h, c = (rng.standard_normal(s).astype(np.float32) for s in ((rows, D), (rows, H), (rows, H)))
    with torch.no_grad():
        f = lambda x: torch.as_tensor(np.asarray(x, np.float64))  # noqa: E731
        ref = oracle.forward({k: f(v) for k, v in params.items()}, f(obs), f(h), f(c))
    for z in ref[4]:
        assert float(z.abs().min() / z.abs().max()) > 1e-5
    n = _native(i, B=rows, T=2)
    n.set_params(params)
    got = n.policy_step(*(torch.as_tensor(x).cuda() for x in (obs, h, c)))
    for name, g, r in zip(("logits", "values", "h", "c"), got, ref):
        _close(g.cpu().numpy(), r.numpy(), name)


def test_agent_runs_on_vector_observations():
    from acme_amd import environment_loop, specs
    from acme_amd.agents.impala import IMPALA
    from acme_amd.testing import fakes
    from acme_amd.utils import loggers
    env = fakes.DiscreteEnvironment(num_actions=3, obs_shape=(10,), episode_length=10)
    spec = specs.make_environment_spec(env)
    agent = IMPALA(spec, IMPALAMLPNetwork(10, (50, 50), 20, spec.actions.num_values),
                   sequence_length=3, sequence_period=3, batch_size=2,
                   logger=loggers.NoOpLogger())
    environment_loop.EnvironmentLoop(env, agent, logger=loggers.NoOpLogger()).run(num_episodes=2)
    assert agent._learner.num_steps >= 1  # noqa: SLF001
    assert np.isfinite(agent._learner.native.metrics.cpu().numpy()).all()  # noqa: SLF001
