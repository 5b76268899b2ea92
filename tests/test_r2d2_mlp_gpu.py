"""The R2D2 step on R2D2MLPNetwork (acme_r2d2_mlp_*: three launches), its one-launch acting step
and the agent against the float64 oracle (tests/r2d2_mlp_oracle.py), at the bars of the R2D2 and
IMPALA-MLP tests:
  q, target q, h, c: rtol 1e-5 + 2e-6 x the tensor's largest value
  errors, priorities, d loss / d q[a]: bit-equal to the oracle's f32 loss arithmetic on the
    kernel's own q; errors end to end 2.5e-4 absolute, the loss 2e-4 relative
  gradients, per tensor, against the f64 backward fed the kernel's own d loss / d q:
    |g - g_ref| <= 1e-4 |g_ref| + 2e-5 max|g_ref|
  Adam in float32 on the kernel's own gradients: 1e-6; the target copy byte for byte.
"""

import functools

import numpy as np
import pytest
import torch

from acme_amd.networks import R2D2MLPNetwork
from oracle import r2d2_oracle as O
from tests import r2d2_act_oracle, r2d2_mlp_oracle as oracle

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-3
PERIOD = 2  # target_update_period: the copy is due at steps 1, 3, ...

# (obs, H, hidden, A, B, T, burn_in, n, store_state): every width off the 4-wide k step with one
# live row, no burn-in and n larger than the two loss steps (the padded-target branch); the
# reference test on one tile; three layers, a second tile with one live row, zero initial
# state; the width limits over three tiles.
CASES = [(5, 3, (7,), 2, 1, 3, 0, 5, True),
         (40, 20, (50, 50), 5, 10, 9, 2, 5, True),
         (33, 20, (17, 40, 9), 5, 17, 7, 3, 3, False),
         (256, 128, (256,), 64, 37, 20, 8, 5, True)]
# Chosen on the CPU: the oracle's ReLU margin exceeds 1e-5 and its top-two q gap 1e-4.
SEEDS = [0, 0, 0, 91]


def _cfg(i):
    _, H, _, A, _, _, BI, n, store = CASES[i]
    return O.R2D2Config(num_actions=A, lstm_size=H, burn_in_length=BI, n_step=n, discount=0.97,
                        target_update_period=PERIOD, learning_rate=LR, adam_epsilon=EPS,
                        store_lstm_state=store, max_replay_size=1000)


def _data(i, B=None, T=None):
    """Parameters of both networks and a batch: a nonzero core state, zeros among the discounts
    in mid-sequence, probabilities that differ per row."""
    D, H, hidden, A, B0, T0 = CASES[i][:6]
    B, T = B or B0, T or T0
    rng = np.random.default_rng(1000 * SEEDS[i] + 7 * B + T)
    shapes = R2D2MLPNetwork(D, H, hidden, A).tensor_shapes()
    draw = lambda: {k: (0.1 * rng.standard_normal(s) if k.endswith("/b") else  # noqa: E731
                        rng.standard_normal(s) / np.sqrt(s[0])).astype(np.float32)
                    for k, s in shapes}
    params, target = draw(), draw()
    disc = (rng.random((B, T)) > 0.25).astype(np.float32)
    disc[:, (CASES[i][6] + T) // 2] = 0.0
    batch = dict(observation=rng.standard_normal((B, T, D)).astype(np.float32),
                 action=rng.integers(0, A, (B, T)).astype(np.int32),
                 reward=rng.standard_normal((B, T)).astype(np.float32), discount=disc,
                 probabilities=rng.uniform(1e-4, 1e-2, B),
                 h0=(0.5 * rng.standard_normal((B, H))).astype(np.float32),
                 c0=(0.5 * rng.standard_normal((B, H))).astype(np.float32))
    return params, target, batch


@functools.lru_cache(None)
def _reference(i):
    ref = oracle.step(_cfg(i), *_data(i))
    assert ref["relu_margin"] > 1e-5 and ref["q_gap"] > 1e-4, (ref["relu_margin"], ref["q_gap"])
    return ref


def _native(i, B=None, T=None):
    from acme_amd.native import NativeR2D2MLP
    D, H, hidden, A, B0, T0, BI, n, store = CASES[i]
    c = _cfg(i)
    return NativeR2D2MLP(obs_dim=D, lstm_size=H, hidden=hidden, num_actions=A, max_batch=B or B0,
                         max_sequence_length=T or T0, burn_in_length=BI, n_step=n,
                         discount=c.discount, max_replay_size=c.max_replay_size,
                         target_update_period=PERIOD, learning_rate=LR, adam_beta1=B1,
                         adam_beta2=B2, adam_epsilon=EPS, store_lstm_state=store)


def _step(n, batch):
    d = {k: torch.as_tensor(v).cuda() for k, v in batch.items()}
    n.step(d["observation"], d["action"], d["reward"], d["discount"], d["probabilities"],
           d["h0"], d["c0"])
    torch.cuda.synchronize()


def _suffix(n, name, i, B, T):
    """A debug buffer's suffix rows, time-major [L, B, A]."""
    A, BI = CASES[i][3], CASES[i][6]
    return np.swapaxes(n.debug_buffer(name).reshape(B, T, A)[:, BI:], 0, 1)


def _state(n, i, B, T):
    """Everything a step writes, as bytes-comparable arrays."""
    out = {w + "/" + k: v for w in ("params", "target", "grads", "m", "v")
           for k, v in n.get_params(w).items()}
    out.update(loss=n.loss.cpu().numpy(), errors=n.errors.cpu().numpy(),
               priorities=n.priorities[:B].cpu().numpy(), g=n.debug_buffer("g"),
               q=_suffix(n, "q", i, B, T), target_q=_suffix(n, "target_q", i, B, T))
    return out


def _close(got, ref, name):
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    scale = float(np.abs(ref).max())
    print(f"{name}: max |err| {float(np.abs(got - ref).max()):.3e}, scale {scale:.3e}")
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=2e-6 * scale, err_msg=name)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_step_matches_oracle(i):
    B, T = CASES[i][4:6]
    cfg = _cfg(i)
    params, target, batch = _data(i)
    ref = _reference(i)
    n = _native(i)
    n.set_params(params, target)
    _step(n, batch)
    q, tq = _suffix(n, "q", i, B, T), _suffix(n, "target_q", i, B, T)
    _close(q, ref["q"], "q")
    _close(tq, ref["target_q"], "target_q")
    # The loss bit for bit against TF's f32 arithmetic on the kernel's own q values.
    err_tf, _ = O.transformed_loss(cfg, q, tq, batch)
    errors = n.errors.cpu().numpy()
    np.testing.assert_array_equal(errors, err_tf)
    np.testing.assert_array_equal(n.priorities[:B].cpu().numpy(),
                                  O.compute_priority(err_tf, cfg.max_priority_weight))
    w32 = O.importance_weights(batch["probabilities"], cfg.max_replay_size,
                               cfg.importance_sampling_exponent)
    g = n.debug_buffer("g").reshape(-1, B)
    np.testing.assert_array_equal(g[:-1], (w32[None, :] * err_tf) * np.float32(1.0 / B))
    assert not g[-1].any()
    # End to end against the f64 networks and loss.
    print(f"errors: max |err| {np.abs(errors - ref['errors']).max():.3e}; loss {n.loss.item()!r} "
          f"against {ref['loss']!r}")
    np.testing.assert_allclose(errors, ref["errors"], atol=2.5e-4, rtol=0)
    np.testing.assert_allclose(n.loss.item(), ref["loss"], rtol=2e-4)
    # Gradients: the f64 backward from the kernel's own d loss / d q.
    grads = n.get_params("grads")
    for k, g_ref in oracle.step(cfg, params, target, batch, g=g[:-1])["grads"].items():
        err = np.abs(grads[k].astype(np.float64) - g_ref)
        bar = 1e-4 * np.abs(g_ref) + 2e-5 * np.abs(g_ref).max()
        print(f"{k}: worst err / bar {float((err / bar).max()):.3f}")
        assert (err <= bar).all(), k
    # snt.Adam in float32 at t = 1 from zero moments, on the kernel's own gradients.
    f, one = np.float32, np.float32(1)
    got = n.get_params("params")
    for k, gk in grads.items():
        m, v = (one - f(B1)) * gk, (one - f(B2)) * (gk * gk)
        upd = (f(LR) * (m / (one - f(B1)))) / (np.sqrt(v / (one - f(B2))) + f(EPS))
        np.testing.assert_allclose(got[k], params[k] - upd, rtol=1e-6, atol=1e-9, err_msg=k)
    # The target: copied after the first update (0 % 2 == 0), kept by the second step.
    for k, v in n.get_params("target").items():
        assert v.tobytes() == got[k].tobytes(), k
    _step(n, batch)
    for k, v in n.get_params("target").items():
        assert v.tobytes() == got[k].tobytes(), k
    assert any(v.tobytes() != got[k].tobytes() for k, v in n.get_params("params").items())


def test_step_repeats_bit_for_bit():
    i = 2
    B, T = CASES[i][4:6]
    params, target, batch = _data(i)
    runs = []
    for _ in range(2):
        n = _native(i)
        n.set_params(params, target)
        _step(n, batch)
        runs.append(_state(n, i, B, T))
    for k, v in runs[0].items():
        assert v.tobytes() == runs[1][k].tobytes(), k


def test_small_step_after_large_equals_fresh_learner():
    i, B, T = 3, 5, CASES[3][6] + 5  # five suffix steps behind the burn-in
    params, target, big = _data(i)
    small = _data(i, B, T)[2]
    used, fresh = _native(i), _native(i, B, T)
    used.set_params(params, target)
    _step(used, big)
    fresh.set_params(used.get_params("params"), used.get_params("target"))
    for w in ("m", "v"):
        fresh._copy_in(getattr(fresh, w), used.get_params(w))  # noqa: SLF001
    fresh.num_steps = used.num_steps
    _step(used, small)
    _step(fresh, small)
    a, b = _state(used, i, B, T), _state(fresh, i, B, T)
    for k, v in a.items():
        assert v.tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("use_target", [False, True])
@pytest.mark.parametrize("rows", [1, 17])
def test_q_step_matches_oracle(rows, use_target):
    i = 2
    D, H, _, A = CASES[i][:4]
    params, target, _ = _data(i)
    rng = np.random.default_rng(rows)
    obs, h, c = (rng.standard_normal(s).astype(np.float32) for s in ((rows, D), (rows, H), (rows, H)))
    with torch.no_grad():
        f = lambda x: torch.as_tensor(np.asarray(x, np.float64))  # noqa: E731
        ref = oracle.forward({k: f(v) for k, v in (target if use_target else params).items()},
                             f(obs), f(h), f(c))
    n = _native(i, B=rows, T=CASES[i][6] + 2)
    n.set_params(params, target)
    dev = [torch.as_tensor(x).cuda() for x in (obs, h, c)]
    q, actions, h1, c1 = n.q_step(*dev, epsilon=0.3, seed=11, step=5, use_target=use_target)
    for name, got, r in zip(("q", "h", "c"), (q, h1, c1), ref):
        _close(got.cpu().numpy(), r.numpy(), name)
    want = r2d2_act_oracle.select(q.cpu().numpy(), 0.3, 11, 5)
    np.testing.assert_array_equal(actions.cpu().numpy(), want)
    # The state advanced in place gives the same bytes.
    n.q_step(*dev, epsilon=0.3, seed=11, step=5, use_target=use_target,
             out=[None, None, dev[1], dev[2]])
    assert dev[1].cpu().numpy().tobytes() == h1.cpu().numpy().tobytes()
    assert dev[2].cpu().numpy().tobytes() == c1.cpu().numpy().tobytes()


def test_agent_runs_on_vector_observations():
    from acme_amd import environment_loop, specs
    from acme_amd.agents.r2d2 import R2D2
    from acme_amd.testing import fakes
    from acme_amd.utils import loggers
    env = fakes.DiscreteEnvironment(num_actions=5, obs_shape=(10, 4), episode_length=10)
    spec = specs.make_environment_spec(env)
    agent = R2D2(spec, R2D2MLPNetwork(40, 20, (50, 50), 5), batch_size=10, samples_per_insert=2,
                 min_replay_size=10, burn_in_length=2, trace_length=6, replay_period=4,
                 checkpoint=False, logger=loggers.NoOpLogger())
    # min_observations = replay_period * max(batch_size, min_replay_size) = 40 steps: the
    # reference test's five episodes of ten steps pass the gate.
    environment_loop.EnvironmentLoop(env, agent, logger=loggers.NoOpLogger()).run(num_episodes=5)
    assert agent.learner.num_steps >= 1
    assert np.isfinite(agent.learner.native.loss.item())
