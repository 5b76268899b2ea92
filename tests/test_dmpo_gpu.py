"""HIP distributional MPO learner step vs the numpy oracle (tests/dmpo_oracle.py, float64).

Reference: DistributionalMPOLearner._step (acme/agents/tf/dmpo/learning.py:147-276).  Every
step here is teacher-forced with explicit eps unless it says otherwise; online and target
parameters are drawn independently, so no KL is zero.

Tolerances: those of tests/test_mpo_gpu.py and tests/test_d4pg_gpu.py, fp32
kernels against an fp64 restatement:
  losses, stats, logits, sampled q, the mixture, ce, dlogits, actions, weights, global norms:
      rtol 1e-5 (+ an atol of 2e-6 times the tensor's largest magnitude)
  gradients: per tensor |g - g_ref| <= 1e-4 |g_ref| + 2e-5 max|g_ref|
  Adam-updated params: every element within 2 lr of the oracle's and 99% within 1e-5 relative
MPO's allowance applies to MPO's cancelling quantities and to nothing else (dmean, dpre, the
policy gradients, the parametric KLs with loss_alpha and the alphas' gradients, the *_kl_q_rel
stats): they may miss the criterion above only by 4x the float32 oracle's own error against
float64 at that shape.  Nothing of the critic side (sampled logits, sampled q, mixture, ce,
dlogits, critic gradients) has an allowance.

The supports of the small cases are narrow and asymmetric ([-1, 5] with rewards in [-3, 5]), so
that r + discount d z falls below vmin, above vmax and strictly inside in every case; the test
asserts that on its own batch before it steps.

The small cases are also set up so that the N sampled distributions of a state differ (see
test_steps_match_oracle), and so that no scalar without an allowance is a near-total
cancellation in the oracle itself: loss_temperature is T (epsilon + mean_b logmeanexp_n(q / T)),
which moves one for one with the mean sampled value and crossed zero on [-2, 3] (1e-3 at
(37, 20, 6, 21), where fp32 rounding of its O(1) terms is all that is left); on [-1, 5] the
sampled values average above zero.  _run_steps asserts |loss_temperature| >= 0.05 on the
oracle's output of every step.
"""

import ctypes
import os

import numpy as np
import pytest
import torch

from tests import dmpo_oracle as O
from tests.test_mpo_gpu import (SCALARS, _MISSES, _check_params, _close, _dev,  # noqa: F401
                                _report_all_misses, _state)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "dmpo_step_b8.npz")


def _native(cfg, B, **kw):
    from acme_amd.native import NativeDMPO
    args = dict(obs_dim=cfg.obs_dim, act_dim=cfg.act_dim, max_batch=B,
                policy_sizes=cfg.policy_sizes, critic_sizes=cfg.critic_sizes,
                num_samples=cfg.num_samples, discount=cfg.discount,
                target_policy_update_period=cfg.target_policy_update_period,
                target_critic_update_period=cfg.target_critic_update_period,
                policy_learning_rate=cfg.policy_lr, critic_learning_rate=cfg.critic_lr,
                dual_learning_rate=cfg.dual_lr, clipping=cfg.clipping, epsilon=cfg.epsilon,
                epsilon_mean=cfg.epsilon_mean, epsilon_stddev=cfg.epsilon_stddev,
                epsilon_penalty=cfg.epsilon_penalty,
                init_log_temperature=cfg.init_log_temperature,
                init_log_alpha_mean=cfg.init_log_alpha_mean,
                init_log_alpha_stddev=cfg.init_log_alpha_stddev,
                per_dim_constraining=cfg.per_dim_constraining,
                action_penalization=cfg.action_penalization, init_scale=cfg.init_scale,
                min_scale=cfg.min_scale, num_atoms=cfg.num_atoms, vmin=cfg.vmin, vmax=cfg.vmax)
    args.update(kw)
    return NativeDMPO(**args)


def _random_params(cfg, seed, mean_scale=1.0, critic_scale=1.0):
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in O.policy_tensor_shapes(cfg) + O.critic_tensor_shapes(cfg):
        if name.endswith("/scale"):
            v = 1.0 + 0.1 * rng.standard_normal(shape)
        elif name.endswith("/b") or name.endswith("/offset"):
            v = 0.1 * rng.standard_normal(shape)
        else:
            v = rng.standard_normal(shape) / np.sqrt(shape[0])
        out[name] = v.astype(np.float32)
    out[O.HEAD + "/linear/w"] = out[O.HEAD + "/linear/w"] * np.float32(mean_scale)
    k = "critic/discrete_valued_head/linear/w"
    out[k] = out[k] * np.float32(critic_scale)
    for name, v in O.init_duals(cfg).items():
        out[name] = (v + 0.3 * rng.standard_normal(v.shape)).astype(np.float32)
    return out


def _batch(cfg, B, seed, r_lo=-3.0, r_hi=5.0):
    """Rewards spread over [r_lo, r_hi] with one low and one high value pinned, the last row
    terminal (d_t = 0)."""
    rng = np.random.default_rng(seed)
    d = np.where(rng.random(B) < 0.05, 0.0, 0.99 ** 4).astype(np.float32)
    d[-1] = 0.0
    r = rng.uniform(r_lo, r_hi, B).astype(np.float32)
    r[0], r[1] = r_lo + 0.5, r_hi - 0.5
    d[0] = d[1] = np.float32(0.99 ** 4)
    return dict(o_tm1=rng.standard_normal((B, cfg.obs_dim)).astype(np.float32),
                a_tm1=rng.uniform(-1, 1, (B, cfg.act_dim)).astype(np.float32),
                r_t=r, d_t=d, o_t=rng.standard_normal((B, cfg.obs_dim)).astype(np.float32))


def _assert_projection_branches(cfg, batch):
    """At least one r + discount d z below vmin, one above vmax, a quarter strictly inside, and
    a terminal row."""
    z = O.support(cfg, np.float64)
    zt = batch["r_t"][:, None].astype(np.float64) + \
        (np.float64(np.float32(cfg.discount)) * batch["d_t"].astype(np.float64))[:, None] * z[None]
    assert (zt < cfg.vmin).any() and (zt > cfg.vmax).any()
    assert ((zt > cfg.vmin) & (zt < cfg.vmax)).mean() >= 0.25
    assert (batch["d_t"] == 0).any()


def _sample_spread(out):
    """How far the N sampled distributions of a state are from their mixture, from the oracle's
    output: min over states of max over samples of the total variation distance."""
    p = np.stack([O.softmax(x) for x in out["sampled_logits"]])
    return float((0.5 * np.abs(p - out["mixture"][None]).sum(axis=-1)).max(axis=0).min())


def _eps(cfg, B, seed):
    return np.random.default_rng(seed).standard_normal(
        (cfg.num_samples, B, cfg.act_dim)).astype(np.float32)


class _Ref:
    """One oracle step in float64, and in float32 for the allowance of the cancelling sums."""

    def __init__(self, cfg, state, batch, eps):
        self.out, self.raw, self.state = O.dmpo_step(cfg, state, batch, eps, np.float64)
        self.out32, self.raw32, _ = O.dmpo_step(cfg, state, batch, eps, np.float32)

    def f32_err(self, key, grad=False, stat=False):
        """4x the float32 oracle's own max error against float64 for one quantity."""
        pick = (lambda o, r: r[key]) if grad else (lambda o, r: o["stats"][key]) if stat else \
            (lambda o, r: o[key])
        a, b = pick(self.out32, self.raw32), pick(self.out, self.raw)
        return 4.0 * float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def _check_buffers(n, ref, cfg, B, tag=""):
    """Losses, stats and every debug buffer of the step against the oracle's `out`: the MPO
    buffers tests/test_mpo_gpu.py checks (without the scalar critic's) and the categorical
    critic's."""
    N, A, K, out = cfg.num_samples, cfg.act_dim, cfg.num_atoms, ref.out
    buf = n.debug_buffer
    _close(n.critic_loss.item(), out["critic_loss"], name=f"critic_loss{tag}")
    _close(n.policy_loss.item(), out["policy_loss"], name=f"policy_loss{tag}")
    stats = n.stats.cpu().numpy()
    for i, k in enumerate(n.stat_names):
        assert k == SCALARS[i]
        if k == "penalty_kl_q_rel" and not cfg.action_penalization:
            assert stats[i] == 0.0 and k not in out["stats"]
            continue
        cancels = k in ("loss_alpha", "kl_q_rel", "penalty_kl_q_rel")
        extra = ref.f32_err(k, stat=True) if cancels else 0.0
        _close(stats[i], out["stats"][k], name=f"stats/{k}{tag}", extra=extra)
    for k, got in (("kl_mean_rel", n.kl_mean_rel), ("kl_stddev_rel", n.kl_stddev_rel)):
        _close(got.cpu().numpy(), out["stats"][k], name=f"{k}{tag}",
               extra=ref.f32_err(k, stat=True))
    for name in ("mean_on", "std_on", "mean_t", "std_t"):
        _close(buf(name)[:B * A], out[name], name=f"{name}{tag}")
    _close(buf("actions")[:N * B * A], out["actions"], name=f"actions{tag}")
    # The categorical critic: no allowance.
    _close(buf("logits_tm1")[:B * K], out["logits_tm1"], name=f"logits_tm1{tag}")
    _close(buf("sampled_logits")[:N * B * K], out["sampled_logits"], name=f"sampled_logits{tag}")
    _close(buf("sampled_q")[:N * B], out["sampled_q"], name=f"sampled_q{tag}")
    _close(buf("mixture")[:B * K], out["mixture"], name=f"mixture{tag}")
    _close(buf("ce")[:B], out["ce"], name=f"ce{tag}")
    _close(buf("dlogits")[:B * K], out["dlogits"], name=f"dlogits{tag}")
    _close(buf("weights")[:N * B], out["weights"], name=f"weights{tag}")
    if cfg.action_penalization:
        _close(buf("cost")[:N * B], out["cost"], name=f"cost{tag}")
        _close(buf("penalty_weights")[:N * B], out["penalty_weights"], name=f"penalty_weights{tag}")
    _close(buf("dmean")[:B * A], out["dmean"], name=f"dmean{tag}", extra=ref.f32_err("dmean"))
    _close(buf("dpre")[:B * A], out["dpre"], name=f"dpre{tag}", extra=ref.f32_err("dpre"))
    _close(buf("norms"), out["norms"], name=f"norms{tag}")


def _check_grads(n, ref):
    g = n.get_params("grads")
    for name, r in ref.raw.items():
        got = g[name].reshape(r.shape).astype(np.float64)
        scale = np.abs(r).max()
        err = np.abs(got - r)
        # The policy's and the alphas' gradients carry MPO's cancelling sums; the critic's none.
        extra = ref.f32_err(name, grad=True) if name.startswith(("policy/", "mpo/log_alpha")) else 0.0
        bound = 1e-4 * np.abs(r) + 2e-5 * scale + 1e-30 + extra
        print(f"grad {name}: max |err| {float(err.max()):.3e}, scale {float(scale):.3e}, "
              f"f32-oracle allowance {extra:.3e}")
        if not (err <= bound).all():
            _MISSES.append(("grad " + name, float(err.max()), float(scale), extra))


def _run_steps(cfg, B, steps, pseed, bseed, mean_scale=1.0, critic_scale=1.0, params=None,
               target=None, start=0, batch_fn=_batch, check_branches=True, min_tv=None,
               max_batch=None, learner=None):
    """`steps` teacher-forced steps against the oracle: after each one the oracle continues
    from the kernel's parameters and moments, so fp32 drift cannot compound.  `min_tv`: what
    _sample_spread of every step's oracle output must reach.  B: the rows of every step, or
    a sequence with the rows of each; max_batch: the learner's creation (default: the largest
    step); learner: an already created learner to step instead (it starts over: these
    parameters, zero moments, step `start`)."""
    sizes = [B] * steps if np.isscalar(B) else list(B)
    assert len(sizes) == steps
    n = learner if learner is not None else _native(cfg, max_batch or max(sizes))
    params = params or _random_params(cfg, pseed, mean_scale, critic_scale)
    target = target or _random_params(cfg, pseed + 1, mean_scale, critic_scale)
    n.set_params(params, target)
    if learner is not None:
        n.m.zero_()
        n.v.zero_()
    n.num_steps = start
    state = _state(params, target, start)
    refs = []
    for s, B in zip(range(start, start + steps), sizes):
        batch, eps = batch_fn(cfg, B, bseed + s), _eps(cfg, B, bseed + 100 + s)
        if check_branches:
            _assert_projection_branches(cfg, batch)
        n.step(*_dev(batch), noise=torch.as_tensor(eps).cuda())
        torch.cuda.synchronize()
        ref = _Ref(cfg, state, batch, eps)
        refs.append(ref)
        if min_tv is not None:
            assert _sample_spread(ref.out) >= min_tv, _sample_spread(ref.out)
        assert abs(ref.out["stats"]["loss_temperature"]) >= 0.05, ref.out["stats"]
        np.testing.assert_array_equal(n.debug_buffer("noise")[:eps.size], eps.ravel())
        _check_buffers(n, ref, cfg, B, tag=f"@{s}")
        _check_grads(n, ref)
        got = n.get_params("params")
        _check_params(cfg, got, ref.state["params"])
        tgt = n.get_params("target")
        for k, r in ref.state["target"].items():
            np.testing.assert_array_equal(tgt[k], np.asarray(r, np.float32), err_msg=k)
        state = dict(params={k: got[k].astype(np.float32) for k in got}, target=tgt,
                     m=n.get_params("m"), v=n.get_params("v"), num_steps=s + 1)
    assert n.num_steps == start + steps
    return n, refs


def _small(**kw):
    base = dict(obs_dim=7, act_dim=3, policy_sizes=(36, 100), critic_sizes=(64, 44),
                num_samples=3, num_atoms=9, vmin=-1.0, vmax=5.0, init_scale=1.0,
                target_policy_update_period=100, target_critic_update_period=100)
    base.update(kw)
    return O.DMPOConfig(**base)


def test_tensor_layout_matches_oracle():
    for per_dim, penal in ((True, True), (False, False)):
        cfg = O.DMPOConfig(per_dim_constraining=per_dim, action_penalization=penal)
        n = _native(cfg, 8)
        assert [(k, s) for k, _, s in n.tensors] == O.dmpo_tensor_shapes(cfg)
        assert n.policy_size == [o for k, o, _ in n.tensors if k.startswith("critic/")][0]
        assert n.dual_offset == [o for k, o, _ in n.tensors if k.startswith("mpo/")][0]
        assert n.flat_size > n.dual_offset > n.policy_size
        p = n.get_params("params")
        for k, v in O.init_duals(cfg).items():
            np.testing.assert_array_equal(p[k], v, err_msg=k)
        np.testing.assert_array_equal(n.values, O.support(cfg, np.float32))
        # The scalar critic's buffers do not exist for this kind, and the lookup says so.
        for name in ("q_tm1", "q_t", "td", "dq"):
            with pytest.raises(ValueError, match="scalar critic"):
                n.debug_buffer(name)
        assert n.debug_buffer("sampled_logits").size == 8 * cfg.num_samples * cfg.num_atoms
        assert n.debug_buffer("mixture").size == 8 * cfg.num_atoms


def test_create_rejects_bad_configurations():
    from acme_amd import _lib
    for kw, msg in ((dict(num_atoms=1), "num_atoms"), (dict(num_atoms=65), "num_atoms"),
                    (dict(vmin=1.0, vmax=1.0), "vmax must exceed vmin"),
                    (dict(vmin=2.0, vmax=-2.0), "vmax must exceed vmin"),
                    (dict(num_samples=65), "num_samples")):
        with pytest.raises(ValueError, match=msg):
            _native(O.DMPOConfig(**kw), 8)
    with pytest.raises(Exception, match="max_batch \\* num_samples"):
        _native(O.DMPOConfig(num_samples=64), _lib.MPO_MAX_ROWS // 64 + 1)


def test_golden_step():
    from tests.golden.make_dmpo_golden import golden_cfg, unpack
    z = np.load(GOLDEN)
    cfg = golden_cfg()
    params, target, batch, eps = unpack(cfg, z)
    _assert_projection_branches(cfg, batch)
    B = len(batch["r_t"])
    n = _native(cfg, B)
    n.set_params(params, target)
    n.num_steps = 1  # neither start-of-step target copy; Adam t = 2
    n.step(*_dev(batch), noise=torch.as_tensor(eps).cuda())
    torch.cuda.synchronize()
    ref = _Ref(cfg, _state(params, target, 1), batch, eps)
    # The fixture is what the oracle computes (tests/test_dmpo_oracle_cpu.py checks every entry).
    np.testing.assert_allclose(ref.out["critic_loss"], z["out/critic_loss"], rtol=1e-12)
    np.testing.assert_allclose(ref.out["mixture"], z["out/mixture"], rtol=1e-10, atol=1e-15)
    _check_buffers(n, ref, cfg, B)
    _check_grads(n, ref)
    _check_params(cfg, n.get_params("params"),
                  {k[len("out/new/"):]: z[k] for k in z.files if k.startswith("out/new/")})


@pytest.mark.parametrize("B,N,A,K", [(5, 3, 3, 51), (37, 20, 6, 21), (8, 64, 1, 64), (6, 1, 16, 2)])
def test_steps_match_oracle(B, N, A, K):
    """Three steps with target periods (2, 3): step 0 copies both networks, step 1 neither,
    step 2 the policy only.  (5, 3, 3, 51): rows not a multiple of the row kernels' 4, N not a
    power of two; (8, 64, 1, 64): a full wave of atoms and the largest N; (6, 1, 16, 2): the
    smallest support with one sample (the mixture is the sample's softmax).

    The mixture is only exercised where the N distributions of a state differ: with the default
    stddev of 0.3 and unit-scale head weights the samples of a state are near-copies (total
    variation from their mixture 0.01 to 0.07 in the float64 oracle), and a kernel that weighed
    the samples wrongly would stay within tolerance.  So the policies' init_scale is 1.0 and the
    critic heads are scaled 4x, and every step asserts on the oracle's output that in every
    state some sample is at least 0.1 in total variation from the mixture."""
    cfg = O.DMPOConfig(obs_dim=7, act_dim=A, policy_sizes=(36, 100), critic_sizes=(64, 132, 44),
                       num_samples=N, num_atoms=K, vmin=-1.0, vmax=5.0, init_scale=1.0,
                       target_policy_update_period=2, target_critic_update_period=3)
    _run_steps(cfg, B, 3, 1, 10, critic_scale=4.0, min_tv=0.1 if N > 1 else None)


def test_full_size_step_matches_oracle():
    """The reference's shapes: B = 256, N = 20 (5,120 target-critic rows), 51 atoms on
    [-150, 150], policy 256x3, critic 512/512/256; one step."""
    cfg = O.DMPOConfig(target_policy_update_period=2, target_critic_update_period=3)
    _run_steps(cfg, 256, 1, 3, 30, batch_fn=lambda c, B, s: _batch(c, B, s, 0.0, 5.0),
               check_branches=False)


@pytest.mark.parametrize("penal", [True, False])
@pytest.mark.parametrize("per_dim", [True, False])
def test_loss_options(per_dim, penal):
    """per_dim_constraining x action_penalization at (5, 3, 3, 9); the mean layer scaled up so
    that samples leave [-1, 1] and the penalty weights are not uniform."""
    cfg = _small(per_dim_constraining=per_dim, action_penalization=penal)
    n, refs = _run_steps(cfg, 5, 2, 5, 40, mean_scale=3.0, critic_scale=4.0, start=1)
    assert np.abs(refs[0].out["kl_mean"]).min() > 0 and np.abs(refs[0].out["kl_stddev"]).min() > 0
    d = 3 if per_dim else 1
    assert n.kl_mean_rel.shape == (d,) and n.get_params("params")["mpo/log_alpha_mean"].shape == (d,)
    assert ("mpo/log_penalty_temperature" in n.get_params("params")) == penal
    if penal:
        assert np.abs(refs[0].out["penalty_weights"] - 1.0 / 3).max() > 1e-2


def test_clipping_on_and_off_with_large_critic_norm():
    """The online critic's first linear layer scaled down 250x: the LayerNorm undoes the scale
    in the forward pass (the logits stay O(1)) and multiplies that layer's gradient by it, so
    the critic's global norm exceeds 40 (the oracle gives ~90).  clipping=True scales the
    critic's gradients down, clipping=False leaves them; the dual gradients are never clipped."""
    base = dict(num_samples=4)
    params = _random_params(_small(**base), 5, critic_scale=4.0)
    for k in ("critic/layer_norm_mlp/linear/w", "critic/layer_norm_mlp/linear/b"):
        params[k] = params[k] * np.float32(0.004)
    target = _random_params(_small(**base), 6, critic_scale=4.0)
    new = {}
    for clipping in (False, True):
        cfg = _small(clipping=clipping, **base)
        n, refs = _run_steps(cfg, 16, 1, 0, 60, params=dict(params), target=dict(target), start=1)
        assert refs[0].out["norms"][1] > 40.0, refs[0].out["norms"]
        new[clipping] = n.get_params("m")
    k = "critic/layer_norm_mlp/linear/w"
    assert np.abs(new[True][k]).max() < np.abs(new[False][k]).max()
    for d in ("mpo/log_temperature", "mpo/log_alpha_mean"):
        np.testing.assert_array_equal(new[True][d], new[False][d])


@pytest.mark.parametrize("explicit", [True, False])
def test_graph_replay_matches_eager(explicit):
    """The captured step graphs (default) and the eager launch sequence (forced by the section
    profiler, as in tests/test_mpo_gpu.py) give bit-identical results over 4 steps with both copy
    periods in play, with explicit and with generated noise, and two alternating batch buffers;
    two replayed steps with generated noise differ."""
    from acme_amd import _lib
    cfg = O.DMPOConfig(obs_dim=7, act_dim=6, policy_sizes=(64, 64, 64), critic_sizes=(128, 128, 64),
                       num_samples=8, num_atoms=51, vmin=-2.0, vmax=3.0,
                       target_policy_update_period=2, target_critic_update_period=3)
    params, target = _random_params(cfg, 11), _random_params(cfg, 12)
    batches = [_dev(_batch(cfg, 64, 20 + i)) for i in range(2)]
    eps = [torch.as_tensor(_eps(cfg, 64, 30 + i)).cuda() for i in range(2)]
    results = []
    for eager in (True, False):
        n = _native(cfg, 64, seed=7)
        n.set_params(params, target)
        noises = []
        _lib.lib().acme_profile_enable(1 if eager else 0)
        try:
            for s in range(6):
                # Steps 1 and 5 copy neither network: step 5 replays step 1's graph.
                n.step(*batches[0 if s in (1, 5) else s % 2],
                       noise=eps[0 if s in (1, 5) else s % 2] if explicit else None)
                torch.cuda.synchronize()
                noises.append(n.debug_buffer("noise").copy())
        finally:
            _lib.lib().acme_profile_enable(0)
        results.append((n.get_params("params"), n.get_params("target"), n.get_params("m"),
                        n.stats.cpu().numpy(), n.critic_loss.item(), n.policy_loss.item(),
                        noises, n.debug_buffer("mixture"), n.debug_buffer("sampled_q")))
        if not explicit:
            assert np.abs(noises[1] - noises[5]).max() > 1.0
    a, b = results
    for which in range(3):
        for k in a[which]:
            np.testing.assert_array_equal(a[which][k], b[which][k], err_msg=k)
    np.testing.assert_array_equal(a[3], b[3])
    for x, y in zip(a[6], b[6]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a[7], b[7])
    np.testing.assert_array_equal(a[8], b[8])
    assert a[4] == b[4] and a[5] == b[5]


def test_neighbours_unchanged_beside_dmpo():
    """D4PG, DDPG and MPO learners stepping in turn with a DMPO learner in one process give the
    bits they give alone (the form of test_d4pg_and_ddpg_unchanged_beside_mpo), and each step
    export refuses the other kind's handle."""
    from acme_amd import _lib
    from acme_amd.native import NativeD4PG, NativeDDPG, NativeMPO
    from oracle import d4pg_oracle as O4
    from tests import ddpg_oracle as OD
    from tests import mpo_oracle as OM
    from tests.test_mpo_gpu import _random_params as mpo_params
    sizes = dict(policy_sizes=(64, 64), critic_sizes=(128, 64))
    rng = np.random.default_rng(0)

    def rand(shapes):
        return {name: (1.0 + 0.1 * rng.standard_normal(shape) if name.endswith("/scale") else
                       rng.standard_normal(shape) / np.sqrt(shape[0])).astype(np.float32)
                for name, shape in shapes}

    p4 = rand(O4.d4pg_tensor_shapes(O4.D4PGConfig(**sizes)))
    pd = rand(OD.ddpg_tensor_shapes(OD.DDPGConfig(**sizes)))
    cm = OM.MPOConfig(num_samples=4, **sizes)
    pm, tm = mpo_params(cm, 1), mpo_params(cm, 2)
    cd = O.DMPOConfig(num_samples=4, **sizes)
    batches = [_dev(_batch(cd, 32, 40 + i)) for i in range(3)]

    def make():
        a = NativeD4PG(obs_dim=24, act_dim=6, max_batch=32, target_update_period=2, **sizes)
        a.set_params(p4, p4)
        b = NativeDDPG(obs_dim=24, act_dim=6, max_batch=32, target_update_period=2, **sizes)
        b.set_params(pd, pd)
        c = NativeMPO(obs_dim=24, act_dim=6, max_batch=32, num_samples=4,
                      target_policy_update_period=2, target_critic_update_period=3, seed=5,
                      **sizes)
        c.set_params(pm, tm)
        return a, b, c

    alone = make()
    for bt in batches:
        for x in alone:
            x.step(*bt)
    torch.cuda.synchronize()
    beside, dmpo = make(), _native(cd, 32)
    dmpo.set_params(_random_params(cd, 1), _random_params(cd, 2))
    for bt in batches:
        dmpo.step(*bt)
        for x in beside:
            x.step(*bt)
    dmpo.step(*batches[0])
    torch.cuda.synchronize()
    assert dmpo.num_steps == 4 and np.isfinite(dmpo.critic_loss.item())
    for x, y in zip(alone, beside):
        assert y.num_steps == 3
        for which in ("params", "target", "m", "v"):
            a, b = x.get_params(which), y.get_params(which)
            for k in a:
                np.testing.assert_array_equal(a[k], b[k], err_msg=f"{which}/{k}")
        assert x.critic_loss.item() == y.critic_loss.item()
        assert x.policy_loss.item() == y.policy_loss.item()
    # The wrong entry for a handle: ACME_ERR_INVALID with the right entry's name, nothing stepped.
    L = _lib.lib()
    bt, out = _lib.MPOBatch(), _lib.MPOOutputs()
    mpo = beside[2]
    assert L.acme_mpo_step(dmpo._h, ctypes.byref(bt), ctypes.byref(out), None) == \
        _lib.ACME_ERR_INVALID  # noqa: SLF001
    assert b"acme_dmpo_step" in L.acme_last_error()
    assert L.acme_dmpo_step(mpo._h, ctypes.byref(bt), ctypes.byref(out), None) == \
        _lib.ACME_ERR_INVALID  # noqa: SLF001
    assert b"acme_mpo_step" in L.acme_last_error()
    d4 = _lib.D4PGBatch()
    assert L.acme_d4pg_step(dmpo._h, ctypes.byref(d4), None, None) == _lib.ACME_ERR_INVALID  # noqa: SLF001
    assert b"acme_dmpo_step" in L.acme_last_error()
    assert dmpo.num_steps == 4 and mpo.num_steps == 3


def test_learner_dropin_path():
    """DistributionalMPOLearner through the uniform GPU replay Table + make_reverb_dataset: a
    few steps, the logger's fields, the reference's get_variables contract, and a save ->
    restore round trip to identical parameters, duals, moments and step count."""
    from acme_amd import replay, specs
    from acme_amd.adders import reverb as adders
    from acme_amd.agents.dmpo import DistributionalMPOLearner
    from acme_amd.datasets import make_reverb_dataset
    from acme_amd.networks import make_dmpo_networks
    from acme_amd.optimizers import Adam
    from acme_amd.utils import loggers
    env_spec = specs.EnvironmentSpec(
        observations=specs.Array((24,), np.float32),
        actions=specs.BoundedArray((6,), np.float32, -1.0, 1.0),
        rewards=specs.Array((), np.float32), discounts=specs.BoundedArray((), np.float32, 0, 1))
    table = replay.Table(adders.DEFAULT_PRIORITY_TABLE, replay.selectors.Uniform(),
                         replay.selectors.Fifo(), 4096, replay.rate_limiters.MinSize(1),
                         signature=adders.NStepTransitionAdder.signature(env_spec), seed=7)
    table.native.fill_synthetic(4096, layout=1, num_actions=1, seed=0)
    server = replay.Server([table])
    nets = make_dmpo_networks(24, env_spec.actions, (64, 64), (128, 64), vmin=-10.0, vmax=10.0,
                              num_atoms=21)
    log = loggers.InMemoryLogger()

    def make(seed, logger):
        return DistributionalMPOLearner(
            nets["policy"], nets["critic"], nets["policy"], nets["critic"], discount=0.99,
            num_samples=8, target_policy_update_period=2, target_critic_update_period=3,
            dataset=make_reverb_dataset(server, batch_size=64), dual_optimizer=Adam(2e-2),
            logger=logger, seed=seed)

    learner = make(0, log)
    assert learner.native.cfg.dual_learning_rate == pytest.approx(2e-2)
    assert learner.native.cfg.num_atoms == 21 and learner.native.num_atoms == 21
    for _ in range(3):
        learner.step()
    torch.cuda.synchronize()
    assert learner.num_steps == 3
    row = log.data[-1]
    for k in ("critic_loss", "policy_loss", "steps") + SCALARS:
        assert np.isfinite(row[k]), k
    assert row["kl_mean_rel"].shape == (6,) and row["kl_stddev_rel"].shape == (6,)
    assert row["loss_policy"] == row["policy_loss"]
    crit, pol = learner.get_variables(["critic", "policy"])
    assert all(k.startswith("critic/") for k in crit) and len(crit) == 8
    assert crit["critic/discrete_valued_head/linear/w"].shape == (64, 21)
    assert all(k.startswith("policy/") for k in pol) and len(pol) == 10
    mean, stddev = learner.policy_distribution(np.zeros((2, 24), np.float32))
    assert mean.shape == (2, 6) and stddev.shape == (2, 6) and (stddev > 0).all()
    saved = learner.save()
    assert saved["params"]["mpo/log_temperature"][0] != 1.0
    assert np.abs(saved["optimizer"]["v"]["critic/discrete_valued_head/linear/w"]).max() > 0
    other = make(0, loggers.NoOpLogger())
    for buf in (other.native.params, other.native.target, other.native.m, other.native.v):
        buf.add_(1.0)
    other.restore(saved)
    assert other.num_steps == 3
    for which in ("params", "target", "m", "v"):
        x, y = learner.native.get_params(which), other.native.get_params(which)
        for k in x:
            if which == "target" and k.startswith("mpo/"):
                continue
            np.testing.assert_array_equal(x[k], y[k], err_msg=f"{which}/{k}")
    # The same step from the restored state gives the same bits (generated noise: same seed,
    # same step number).
    batch = _dev(_batch(O.DMPOConfig(), 64, 1))
    learner.native.step(*batch)
    other.native.step(*batch)
    torch.cuda.synchronize()
    for which in ("params", "m", "v"):
        x, y = learner.native.get_params(which), other.native.get_params(which)
        for k in x:
            np.testing.assert_array_equal(x[k], y[k], err_msg=f"{which}/{k}")


def test_agent_runs_in_environment_loop():
    """The reference's agent test (acme/agents/tf/dmpo/agent_test.py), run-only: small networks
    on the fake bounded continuous environment the MPO agent test uses, batch_size 10,
    num_samples 5."""
    from acme_amd import specs
    from acme_amd.agents.dmpo import DistributionalMPO
    from acme_amd.environment_loop import EnvironmentLoop
    from acme_amd.networks import make_dmpo_networks
    from acme_amd.testing import fakes
    from acme_amd.utils import loggers
    env = fakes.ContinuousEnvironment(episode_length=10, bounded=True)
    spec = specs.make_environment_spec(env)
    nets = make_dmpo_networks(24, spec.actions, (12, 12), (12, 12), vmin=-5.0, vmax=5.0,
                              num_atoms=11)
    agent = DistributionalMPO(spec, nets["policy"], nets["critic"], batch_size=10,
                              samples_per_insert=2, min_replay_size=10, num_samples=5,
                              logger=loggers.NoOpLogger())
    loop = EnvironmentLoop(env, agent, logger=loggers.NoOpLogger())
    loop.run(num_episodes=4)
    learner = agent._learner  # noqa: SLF001
    torch.cuda.synchronize()
    assert learner.num_steps >= 1
    assert np.isfinite(learner.native.critic_loss.item())
    assert np.isfinite(learner.native.policy_loss.item())
    assert np.isfinite(learner.native.stats.cpu().numpy()).all()
