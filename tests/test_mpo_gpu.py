"""HIP MPO learner step vs the numpy oracle (tests/mpo_oracle.py, float64).

Reference: MPOLearner._step (acme/agents/tf/mpo/learning.py:145-260) and losses.MPO
(acme/tf/losses/mpo.py:145-430).  Every step here is teacher-forced with explicit eps unless
it says otherwise; online and target parameters are drawn independently, so no KL is zero.

Tolerances (fp32 kernels against an fp64 restatement), those of tests/test_ddpg_gpu.py:
  losses, stats, q values, actions, weights, global norms: rtol 1e-5 (+ an atol of 2e-6 times
      the tensor's largest magnitude, the fp32 rounding floor of its scale)
  gradients: per tensor |g - g_ref| <= 1e-4 |g_ref| + 2e-5 max|g_ref|
  Adam-updated params: every element within 2 lr of the oracle's and 99% within 1e-5 relative
Two kinds of quantity cancel in fp32 whatever computes them: the policy's mean / scale
gradients (dmean, dpre, the policy tensors' gradients) sum terms over the samples that nearly
cancel, and the KLs: the parametric ones (kl_mean_rel, kl_stddev_rel, loss_alpha, the alphas'
gradients) are differences of an online and a target network that are one Adam step apart
after a target copy, the non-parametric ones (kl_q_rel, penalty_kl_q_rel) sum w log(N w) over
weights near 1 / N and are then divided by an epsilon of 1e-1 or 1e-3.  Their bound is never loosened by hand: the oracle is also run in float32 and such a
quantity may miss its criterion above only by 4x the float32 oracle's own error against
float64 at that shape (_Ref.f32_err).

Measured on the MI355X over this file (worst case, error / the tensor's scale; for the
cancelling quantities also the absolute error against the allowance that held):
  losses 3.0e-6, sampled q 4.1e-7, actions 2.0e-7, weights 2.2e-7, norms 6.5e-7, td 1.6e-7,
  critic gradients 4.8e-7, temperature gradient 4.5e-6
  dmean 1.0e-5 (1.95e-6 abs, allowance 8.4e-6), dpre 7.3e-6, policy gradients 9.8e-6
  kl_mean_rel 4.0e-5 (7.0e-6 abs, allowance 2.3e-5), kl_stddev_rel 3.6e-5 (3.5e-4 abs of 9.6,
  allowance 8.8e-2), loss_alpha 1.8e-5, alpha gradients 1.7e-5 / 4.1e-5,
  kl_q_rel 6.2e-3 (5.3e-8 abs, allowance 3.6e-7), penalty_kl_q_rel 3.6e-3 (1.0e-5 abs, allowance
  4.0e-5); generated noise within 4.4e-7 of the float64 restatement (bound 4e-6).
The same figures are in DESIGN.md §4.2 "MPO".
"""

import os

import numpy as np
import pytest
import torch

from tests import mpo_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "mpo_step_b8.npz")
SCALARS = ("dual_alpha_mean", "dual_alpha_stddev", "dual_temperature", "loss_policy", "loss_alpha",
           "loss_temperature", "kl_q_rel", "penalty_kl_q_rel", "q_min", "q_max", "pi_stddev_min",
           "pi_stddev_max", "pi_stddev_cond")


def _native(cfg, B, **kw):
    from acme_amd.native import NativeMPO
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
                min_scale=cfg.min_scale)
    args.update(kw)
    return NativeMPO(**args)


def _dev(batch):
    return [torch.as_tensor(batch[k]).cuda().contiguous()
            for k in ("o_tm1", "a_tm1", "r_t", "d_t", "o_t")]


_MISSES = []  # comparisons that missed their bound in the running test


@pytest.fixture(autouse=True)
def _report_all_misses():
    """Every comparison of a test is made and printed before the test fails on the misses."""
    _MISSES.clear()
    yield
    misses = list(_MISSES)
    _MISSES.clear()
    assert not misses, misses


def _close(got, ref, rtol=1e-5, floor=2e-6, name="", extra=0.0):
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    scale = max(float(np.abs(ref).max()), 1e-30)
    err = np.abs(got - ref)
    bound = rtol * np.abs(ref) + floor * scale + extra
    print(f"{name}: max |err| {float(err.max()):.3e}, scale {scale:.3e}, "
          f"f32-oracle allowance {extra:.3e}")
    if not (err <= bound).all():
        i = int(np.argmax(err - bound))
        _MISSES.append((name, float(err.ravel()[i]), float(bound.ravel()[i])))


def _random_params(cfg, seed, mean_scale=1.0):
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
    for name, v in O.init_duals(cfg).items():
        out[name] = (v + 0.3 * rng.standard_normal(v.shape)).astype(np.float32)
    return out


def _batch(cfg, B, seed):
    rng = np.random.default_rng(seed)
    d = np.where(rng.random(B) < 0.05, 0.0, 0.99 ** 4).astype(np.float32)
    return dict(o_tm1=rng.standard_normal((B, cfg.obs_dim)).astype(np.float32),
                a_tm1=rng.uniform(-1, 1, (B, cfg.act_dim)).astype(np.float32),
                r_t=rng.uniform(0, 5, B).astype(np.float32), d_t=d,
                o_t=rng.standard_normal((B, cfg.obs_dim)).astype(np.float32))


def _eps(cfg, B, seed):
    return np.random.default_rng(seed).standard_normal(
        (cfg.num_samples, B, cfg.act_dim)).astype(np.float32)


class _Ref:
    """One oracle step in float64, and in float32 for the allowance of the cancelling sums."""

    def __init__(self, cfg, state, batch, eps):
        self.out, self.raw, self.state = O.mpo_step(cfg, state, batch, eps, np.float64)
        self.out32, self.raw32, _ = O.mpo_step(cfg, state, batch, eps, np.float32)

    def f32_err(self, key, grad=False, stat=False):
        """4x the float32 oracle's own max error against float64 for one quantity."""
        pick = (lambda o, r: r[key]) if grad else (lambda o, r: o["stats"][key]) if stat else \
            (lambda o, r: o[key])
        a, b = pick(self.out32, self.raw32), pick(self.out, self.raw)
        return 4.0 * float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def _check_buffers(n, ref, cfg, B, tag=""):
    """Losses, stats and every debug buffer of the step against the oracle's `out`."""
    N, A, out = cfg.num_samples, cfg.act_dim, ref.out
    buf = n.debug_buffer
    _close(n.critic_loss.item(), out["critic_loss"], name=f"critic_loss{tag}")
    _close(n.policy_loss.item(), out["policy_loss"], name=f"policy_loss{tag}")
    stats = n.stats.cpu().numpy()
    for i, k in enumerate(n.stat_names):
        assert k == SCALARS[i]
        if k == "penalty_kl_q_rel" and not cfg.action_penalization:
            assert stats[i] == 0.0 and k not in out["stats"]
            continue
        # loss_alpha is a function of the parametric KLs; the non-parametric KLs sum
        # w log(N w) over weights near 1 / N, terms of both signs that cancel.
        cancels = k in ("loss_alpha", "kl_q_rel", "penalty_kl_q_rel")
        extra = ref.f32_err(k, stat=True) if cancels else 0.0
        _close(stats[i], out["stats"][k], name=f"stats/{k}{tag}", extra=extra)
    for k, got in (("kl_mean_rel", n.kl_mean_rel), ("kl_stddev_rel", n.kl_stddev_rel)):
        _close(got.cpu().numpy(), out["stats"][k], name=f"{k}{tag}",
               extra=ref.f32_err(k, stat=True))
    for name, key in (("mean_on", "mean_on"), ("std_on", "std_on"), ("mean_t", "mean_t"),
                      ("std_t", "std_t")):
        _close(buf(name)[:B * A], out[key], name=f"{name}{tag}")
    _close(buf("actions")[:N * B * A], out["actions"], name=f"actions{tag}")
    _close(buf("sampled_q")[:N * B], out["sampled_q"], name=f"sampled_q{tag}")
    _close(buf("q_tm1")[:B], out["q_tm1"], name=f"q_tm1{tag}")
    _close(buf("q_t")[:B], out["q_t"], name=f"q_t{tag}")
    _close(buf("td")[:B], out["td"], name=f"td{tag}")
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
        # The policy's and the alphas' gradients carry the cancelling sums (module docstring).
        extra = ref.f32_err(name, grad=True) if name.startswith(("policy/", "mpo/log_alpha")) else 0.0
        bound = 1e-4 * np.abs(r) + 2e-5 * scale + 1e-30 + extra
        print(f"grad {name}: max |err| {float(err.max()):.3e}, scale {float(scale):.3e}, "
              f"f32-oracle allowance {extra:.3e}")
        if not (err <= bound).all():
            _MISSES.append(("grad " + name, float(err.max()), float(scale), extra))


def _lr(cfg, k):
    return cfg.dual_lr if k.startswith("mpo/") else cfg.policy_lr


def _check_params(cfg, got, want):
    for k, r in want.items():
        gk = got[k].reshape(r.shape).astype(np.float64)
        err = np.abs(gk - r)
        assert err.max() <= 2 * _lr(cfg, k) + 1e-6, (k, float(err.max()))
        frac = np.mean(err <= 1e-5 * np.abs(r) + 1e-7)
        assert frac >= 0.99, (k, frac)


def _state(params, target, num_steps=0):
    z = {k: np.zeros_like(v) for k, v in params.items()}
    return dict(params=params, target=target, m=z, v=dict(z), num_steps=num_steps)


def _run_steps(cfg, B, steps, pseed, bseed, mean_scale=1.0, params=None, target=None, start=0,
               max_batch=None, learner=None):
    """`steps` teacher-forced steps against the oracle: after each one the oracle continues
    from the kernel's parameters and moments, so fp32 drift cannot compound.  `start`: the
    step count to begin at (1: the first step copies no target, whatever the periods).
    B: the rows of every step, or a sequence with the rows of each; max_batch: the learner's
    creation (default: the largest step); learner: an already created learner to step instead
    (it starts over: these parameters, zero moments, step `start`)."""
    sizes = [B] * steps if np.isscalar(B) else list(B)
    assert len(sizes) == steps
    n = learner if learner is not None else _native(cfg, max_batch or max(sizes))
    params = params or _random_params(cfg, pseed, mean_scale)
    target = target or _random_params(cfg, pseed + 1, mean_scale)
    n.set_params(params, target)
    if learner is not None:
        n.m.zero_()
        n.v.zero_()
    n.num_steps = start
    state = _state(params, target, start)
    refs = []
    for s, B in zip(range(start, start + steps), sizes):
        batch, eps = _batch(cfg, B, bseed + s), _eps(cfg, B, bseed + 100 + s)
        n.step(*_dev(batch), noise=torch.as_tensor(eps).cuda())
        torch.cuda.synchronize()
        ref = _Ref(cfg, state, batch, eps)
        refs.append(ref)
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


def test_tensor_layout_matches_oracle():
    for per_dim, penal in ((True, True), (False, False)):
        cfg = O.MPOConfig(per_dim_constraining=per_dim, action_penalization=penal)
        n = _native(cfg, 8)
        assert [(k, s) for k, _, s in n.tensors] == O.mpo_tensor_shapes(cfg)
        assert n.policy_size == [o for k, o, _ in n.tensors if k.startswith("critic/")][0]
        assert n.dual_offset == [o for k, o, _ in n.tensors if k.startswith("mpo/")][0]
        assert n.flat_size > n.dual_offset > n.policy_size
        # The duals start at the loss module's initial values (mpo.py:110-143).
        p = n.get_params("params")
        for k, v in O.init_duals(cfg).items():
            np.testing.assert_array_equal(p[k], v, err_msg=k)


def test_create_rejects_too_many_rows():
    from acme_amd import _lib
    cfg = O.MPOConfig(num_samples=64)
    with pytest.raises(Exception, match="max_batch \\* num_samples"):
        _native(cfg, _lib.MPO_MAX_ROWS // 64 + 1)
    with pytest.raises(ValueError, match="num_samples"):
        _native(O.MPOConfig(num_samples=65), 8)


def test_golden_step():
    from tests.golden.make_mpo_golden import golden_cfg, unpack
    z = np.load(GOLDEN)
    cfg = golden_cfg()
    params, target, batch, eps = unpack(cfg, z)
    B = len(batch["r_t"])
    n = _native(cfg, B)
    n.set_params(params, target)
    n.num_steps = 1  # neither start-of-step target copy; Adam t = 2
    n.step(*_dev(batch), noise=torch.as_tensor(eps).cuda())
    torch.cuda.synchronize()
    ref = _Ref(cfg, _state(params, target, 1), batch, eps)
    # The fixture is what the oracle computes (tests/test_mpo_oracle_cpu.py checks every entry).
    np.testing.assert_allclose(ref.out["policy_loss"], z["out/policy_loss"], rtol=1e-12)
    np.testing.assert_allclose(ref.out["dmean"], z["out/dmean"], rtol=1e-10, atol=1e-15)
    _check_buffers(n, ref, cfg, B)
    _check_grads(n, ref)
    _check_params(cfg, n.get_params("params"),
                  {k[len("out/new/"):]: z[k] for k in z.files if k.startswith("out/new/")})


@pytest.mark.parametrize("B,N,A", [(5, 3, 3), (37, 20, 6), (8, 64, 1), (6, 2, 16)])
def test_steps_match_oracle(B, N, A):
    """Three steps with target periods (2, 3): step 0 copies both networks, step 1 neither,
    step 2 the policy only.  (5, 3, 3): rows not a multiple of the row kernels' 4, N below a
    wave and not a power of two; (8, 64, 1): a full wave of samples, one action; (6, 2, 16): the
    widest action."""
    cfg = O.MPOConfig(obs_dim=7, act_dim=A, policy_sizes=(36, 100), critic_sizes=(64, 132, 44),
                      num_samples=N, target_policy_update_period=2,
                      target_critic_update_period=3)
    _run_steps(cfg, B, 3, 1, 10)


def test_full_size_step_matches_oracle():
    """The reference's shapes: B = 256, N = 20 (5,120 target-critic rows), policy 256x3, critic
    512/512/256; one step."""
    cfg = O.MPOConfig(target_policy_update_period=2, target_critic_update_period=3)
    _run_steps(cfg, 256, 1, 3, 30)


@pytest.mark.parametrize("penal", [True, False])
@pytest.mark.parametrize("per_dim", [True, False])
def test_loss_options(per_dim, penal):
    """per_dim_constraining x action_penalization at (5, 3, 3); the mean layer scaled up so
    that samples leave [-1, 1] and the penalty weights are not uniform."""
    cfg = O.MPOConfig(obs_dim=7, act_dim=3, policy_sizes=(36, 100), critic_sizes=(64, 44),
                      num_samples=3, per_dim_constraining=per_dim, action_penalization=penal,
                      target_policy_update_period=100, target_critic_update_period=100)
    n, refs = _run_steps(cfg, 5, 2, 5, 40, mean_scale=3.0, start=1)
    assert np.abs(refs[0].out["kl_mean"]).min() > 0 and np.abs(refs[0].out["kl_stddev"]).min() > 0
    d = 3 if per_dim else 1
    assert n.kl_mean_rel.shape == (d,) and n.get_params("params")["mpo/log_alpha_mean"].shape == (d,)
    assert ("mpo/log_penalty_temperature" in n.get_params("params")) == penal
    if penal:
        assert np.abs(refs[0].out["penalty_weights"] - 1.0 / 3).max() > 1e-2


def test_dual_projection():
    """A log-dual at -30 comes back projected to -18 before Adam's update, as in the oracle."""
    cfg = O.MPOConfig(obs_dim=7, act_dim=3, policy_sizes=(36, 100), critic_sizes=(64, 44),
                      num_samples=3, target_policy_update_period=100,
                      target_critic_update_period=100)
    params, target = _random_params(cfg, 1), _random_params(cfg, 2)
    params["mpo/log_alpha_stddev"] = np.full(3, -30.0, np.float32)
    params["mpo/log_temperature"] = np.full(1, -18.5, np.float32)
    n, refs = _run_steps(cfg, 5, 1, 0, 50, params=params, target=target, start=1)
    got = n.get_params("params")
    want = refs[0].state["params"]
    for k in ("mpo/log_alpha_stddev", "mpo/log_temperature"):
        assert (np.abs(got[k] + 18.0) <= cfg.dual_lr * 1.001).all(), (k, got[k])
        np.testing.assert_allclose(got[k], want[k], rtol=1e-6, err_msg=k)


def test_step_zero_target_equals_online():
    """Step 0 with both periods 1: the targets are copies of the online networks, so both KLs
    are zero up to an absolute floor (1e-7, an fp32 ulp of the O(1) terms that cancel)."""
    cfg = O.MPOConfig(obs_dim=7, act_dim=3, policy_sizes=(36, 100), critic_sizes=(64, 44),
                      num_samples=5, target_policy_update_period=1,
                      target_critic_update_period=1)
    n = _native(cfg, 9)
    params = _random_params(cfg, 1)
    n.set_params(params, _random_params(cfg, 2))
    batch, eps = _batch(cfg, 9, 3), _eps(cfg, 9, 4)
    n.step(*_dev(batch), noise=torch.as_tensor(eps).cuda())
    torch.cuda.synchronize()
    ref = _Ref(cfg, _state(params, _random_params(cfg, 2)), batch, eps)
    assert np.abs(ref.out["kl_mean"]).max() == 0.0
    assert np.abs(n.kl_mean_rel.cpu().numpy()).max() * cfg.epsilon_mean <= 1e-7
    assert np.abs(n.kl_stddev_rel.cpu().numpy()).max() * cfg.epsilon_stddev <= 1e-7
    _close(n.policy_loss.item(), ref.out["policy_loss"], name="policy_loss")
    _close(n.debug_buffer("dmean")[:27], ref.out["dmean"], name="dmean",
           extra=ref.f32_err("dmean"))
    tgt = n.get_params("target")
    for k, v in params.items():
        if not k.startswith("mpo/"):
            np.testing.assert_array_equal(tgt[k], v, err_msg=k)


def test_no_clipping_and_clipped_policy_norm():
    """A target policy with small stddevs makes the cross entropies steep: the policy's global
    norm exceeds 40.  clipping=True scales its gradients down, clipping=False leaves them; the
    dual gradients are never clipped."""
    base = dict(obs_dim=7, act_dim=3, policy_sizes=(36, 100), critic_sizes=(64, 44),
                num_samples=4, target_policy_update_period=100,
                target_critic_update_period=100)
    params = _random_params(O.MPOConfig(**base), 5)
    target = _random_params(O.MPOConfig(**base), 6)
    target[O.HEAD + "/linear_1/b"] = np.full(3, -4.0, np.float32)
    target[O.HEAD + "/linear_1/w"] *= np.float32(0.1)
    new = {}
    for clipping in (False, True):
        cfg = O.MPOConfig(clipping=clipping, **base)
        n, refs = _run_steps(cfg, 16, 1, 0, 60, params=dict(params), target=dict(target),
                             start=1)
        assert refs[0].out["norms"][0] > 40.0, refs[0].out["norms"]
        new[clipping] = n.get_params("m")
    k = O.HEAD + "/linear/w"
    assert np.abs(new[True][k]).max() < np.abs(new[False][k]).max()
    for d in ("mpo/log_temperature", "mpo/log_alpha_mean"):
        np.testing.assert_array_equal(new[True][d], new[False][d])


# ------------------------------------------------------------------ generated noise


def _philox4x32_10(idx, step, tag, seed):
    """Philox4x32-10 (Salmon et al., SC'11) in uint64 arithmetic: exact."""
    u = np.uint64
    mask = u(0xFFFFFFFF)
    x, y = idx.astype(u), np.full(idx.shape, step & 0xFFFFFFFF, u)
    z, w = np.full(idx.shape, step >> 32, u), np.full(idx.shape, tag, u)
    k0, k1 = u(seed & 0xFFFFFFFF), u(seed >> 32)
    for _ in range(10):
        p0, p1 = u(0xD2511F53) * x, u(0xCD9E8D57) * z
        x, y, z, w = (p1 >> u(32)) ^ y ^ k0, p1 & mask, (p0 >> u(32)) ^ w ^ k1, p0 & mask
        k0, k1 = (k0 + u(0x9E3779B9)) & mask, (k1 + u(0xBB67AE85)) & mask
    return x, y, z, w


def _noise_ref(seed, step, count):
    """include/acme_hip.h "Sampling noise", Box-Muller in float64."""
    idx = np.arange((count + 3) // 4)
    x, y, z, w = _philox4x32_10(idx, step, 0x4D504F4E, seed)

    def pair(a, b):
        u1 = ((a >> np.uint64(8)).astype(np.float64) + 1.0) / 2.0 ** 24
        u2 = (b >> np.uint64(8)).astype(np.float64) / 2.0 ** 24
        rad = np.sqrt(-2.0 * np.log(u1))
        return rad * np.cos(2 * np.pi * u2), rad * np.sin(2 * np.pi * u2)

    z0, z1 = pair(x, y)
    z2, z3 = pair(z, w)
    return np.stack([z0, z1, z2, z3], axis=1).ravel()[:count]


def _noise_cfg():
    return O.MPOConfig(obs_dim=7, act_dim=6, policy_sizes=(32, 32), critic_sizes=(32, 32),
                       num_samples=32, target_policy_update_period=100,
                       target_critic_update_period=100)


def test_generated_noise():
    """noise=None: the "noise" buffer is the documented Philox / Box-Muller stream of (seed,
    step) to 4e-6 absolute (a few ulp of f32 at |z| <= 5.8; the angle is exact through
    sincospif), has the moments of N(0, 1), differs between two graph-replayed steps, and
    passed back as explicit noise reproduces the step bit for bit."""
    cfg, B, seed = _noise_cfg(), 64, 0x123456789ABCDEF
    count = cfg.num_samples * B * cfg.act_dim
    assert count >= 10 ** 4
    params, target = _random_params(cfg, 1), _random_params(cfg, 2)
    batch = _dev(_batch(cfg, B, 3))
    n = _native(cfg, B, seed=seed)
    n.set_params(params, target)
    noises, before = [], None
    for s in range(3):  # step 0 copies the targets; step 1 captures the no-copy graph, step 2 replays it
        if s == 2:
            before = {w: n.get_params(w) for w in ("params", "target", "m", "v")}
        n.step(*batch)
        torch.cuda.synchronize()
        got = n.debug_buffer("noise")[:count].astype(np.float64)
        ref = _noise_ref(seed, s, count)
        print(f"step {s}: max |noise - ref| {np.abs(got - ref).max():.3e}, max |z| {np.abs(got).max():.3f}")
        assert np.abs(got - ref).max() <= 4e-6
        se = 1.0 / np.sqrt(count)
        assert abs(got.mean()) <= 5 * se
        assert abs(got.var() - 1.0) <= 5 * np.sqrt(2.0) * se
        noises.append(got)
    assert np.abs(noises[1] - noises[2]).max() > 1.0
    after = n.get_params("params")
    # The same step from the same state with that buffer as explicit noise.
    m = _native(cfg, B, seed=seed + 1)
    m.set_params(before["params"], before["target"])
    for buf, src in ((m.m, before["m"]), (m.v, before["v"])):
        for k, t in m.views(buf).items():
            t.copy_(torch.as_tensor(src[k]).view(t.shape))
    m.num_steps = 2
    eps = torch.as_tensor(n.debug_buffer("noise")[:count]).cuda()
    m.step(*batch, noise=eps)
    torch.cuda.synchronize()
    for k, v in m.get_params("params").items():
        np.testing.assert_array_equal(v, after[k], err_msg=k)


@pytest.mark.parametrize("explicit", [True, False])
def test_graph_replay_matches_eager(explicit):
    """The captured step graphs (default) and the eager launch sequence (forced by the section
    profiler) give bit-identical results over 4 steps with both copy periods in play, with
    explicit and with generated noise, and the two alternating batch buffers of the dataset."""
    from acme_amd import _lib
    cfg = O.MPOConfig(obs_dim=7, act_dim=6, policy_sizes=(64, 64, 64), critic_sizes=(128, 128, 64),
                      num_samples=8, target_policy_update_period=2,
                      target_critic_update_period=3)
    params, target = _random_params(cfg, 11), _random_params(cfg, 12)
    batches = [_dev(_batch(cfg, 64, 20 + i)) for i in range(2)]
    eps = [torch.as_tensor(_eps(cfg, 64, 30 + i)).cuda() for i in range(2)]
    results = []
    for eager in (True, False):
        n = _native(cfg, 64, seed=7)
        n.set_params(params, target)
        _lib.lib().acme_profile_enable(1 if eager else 0)
        try:
            for s in range(4):
                n.step(*batches[s % 2], noise=eps[s % 2] if explicit else None)
        finally:
            _lib.lib().acme_profile_enable(0)
        torch.cuda.synchronize()
        results.append((n.get_params("params"), n.get_params("target"), n.get_params("m"),
                        n.stats.cpu().numpy(), n.critic_loss.item(), n.policy_loss.item(),
                        n.debug_buffer("noise")))
    a, b = results
    for which in range(3):
        for k in a[which]:
            np.testing.assert_array_equal(a[which][k], b[which][k], err_msg=k)
    np.testing.assert_array_equal(a[3], b[3])
    np.testing.assert_array_equal(a[6], b[6])
    assert a[4] == b[4] and a[5] == b[5]


def test_d4pg_and_ddpg_unchanged_beside_mpo():
    """D4PG and DDPG learners stepping in turn with an MPO learner in one process give the
    bits they give alone: the three share the native object's code, not state."""
    from acme_amd.native import NativeD4PG, NativeDDPG
    from oracle import d4pg_oracle as O4
    from tests import ddpg_oracle as OD
    sizes = dict(policy_sizes=(64, 64), critic_sizes=(128, 64))
    rng = np.random.default_rng(0)

    def rand(shapes):
        return {name: (1.0 + 0.1 * rng.standard_normal(shape) if name.endswith("/scale") else
                       rng.standard_normal(shape) / np.sqrt(shape[0])).astype(np.float32)
                for name, shape in shapes}

    p4 = rand(O4.d4pg_tensor_shapes(O4.D4PGConfig(**sizes)))
    pd = rand(OD.ddpg_tensor_shapes(OD.DDPGConfig(**sizes)))
    cm = O.MPOConfig(num_samples=4, **sizes)
    batches = [_dev(_batch(cm, 32, 40 + i)) for i in range(3)]

    def make():
        a = NativeD4PG(obs_dim=24, act_dim=6, max_batch=32, target_update_period=2, **sizes)
        a.set_params(p4, p4)
        b = NativeDDPG(obs_dim=24, act_dim=6, max_batch=32, target_update_period=2, **sizes)
        b.set_params(pd, pd)
        return a, b

    alone = make()
    for bt in batches:
        for x in alone:
            x.step(*bt)
    torch.cuda.synchronize()
    beside, mpo = make(), _native(cm, 32)
    mpo.set_params(_random_params(cm, 1), _random_params(cm, 2))
    for bt in batches:
        mpo.step(*bt)
        for x in beside:
            x.step(*bt)
    mpo.step(*batches[0])
    torch.cuda.synchronize()
    assert mpo.num_steps == 4 and np.isfinite(mpo.policy_loss.item())
    for x, y in zip(alone, beside):
        assert y.num_steps == 3
        for which in ("params", "target", "m", "v"):
            a, b = x.get_params(which), y.get_params(which)
            for k in a:
                np.testing.assert_array_equal(a[k], b[k], err_msg=f"{which}/{k}")
        assert x.critic_loss.item() == y.critic_loss.item()
        assert x.policy_loss.item() == y.policy_loss.item()


def test_learner_dropin_path():
    """MPOLearner through the uniform GPU replay Table + make_reverb_dataset: step, the
    logger's fields, the reference's get_variables contract, and a save -> restore round trip
    that covers the duals, all moments and num_steps (generated noise on both sides)."""
    from acme_amd import replay, specs
    from acme_amd.adders import reverb as adders
    from acme_amd.agents.mpo import MPOLearner
    from acme_amd.datasets import make_reverb_dataset
    from acme_amd.networks import make_mpo_networks
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
    nets = make_mpo_networks(24, env_spec.actions, (64, 64), (128, 64))
    log = loggers.InMemoryLogger()

    def make(seed, logger):
        return MPOLearner(nets["policy"], nets["critic"], nets["policy"], nets["critic"],
                          discount=0.99, num_samples=8, target_policy_update_period=2,
                          target_critic_update_period=3,
                          dataset=make_reverb_dataset(server, batch_size=64),
                          dual_optimizer=Adam(2e-2), logger=logger, seed=seed)

    learner = make(0, log)
    assert learner.native.cfg.dual_learning_rate == pytest.approx(2e-2)
    for _ in range(2):
        learner.step()
    torch.cuda.synchronize()
    assert learner.num_steps == 2
    row = log.data[-1]
    for k in ("critic_loss", "policy_loss", "steps") + SCALARS:
        assert np.isfinite(row[k]), k
    assert row["kl_mean_rel"].shape == (6,) and row["kl_stddev_rel"].shape == (6,)
    assert row["loss_policy"] == row["policy_loss"]
    crit, pol = learner.get_variables(["critic", "policy"])
    assert all(k.startswith("critic/") for k in crit) and len(crit) == 8
    assert all(k.startswith("policy/") for k in pol) and len(pol) == 10
    tgt = learner.native.get_params("target")  # the exposed variables are the TARGET networks
    np.testing.assert_array_equal(pol["policy/multivariate_normal_diag_head/linear_1/w"],
                                  tgt["policy/multivariate_normal_diag_head/linear_1/w"])
    mean, stddev = learner.policy_distribution(np.zeros((2, 24), np.float32))
    assert mean.shape == (2, 6) and stddev.shape == (2, 6) and (stddev > 0).all()
    np.testing.assert_array_equal(learner.policy(np.zeros((2, 24), np.float32)), mean)
    # The duals moved from their initial values and are part of the saved state.
    saved = learner.save()
    assert saved["params"]["mpo/log_temperature"][0] != 1.0
    assert np.abs(saved["optimizer"]["v"]["mpo/log_alpha_mean"]).max() > 0
    # A fresh learner with the same seed (the key of the generated noise is configuration,
    # not state), its buffers spoiled so that only a full restore can make it agree.
    other = make(0, loggers.NoOpLogger())
    for buf in (other.native.params, other.native.target, other.native.m, other.native.v):
        buf.add_(1.0)
    other.restore(saved)
    assert other.num_steps == 2
    rng = np.random.default_rng(1)
    batch = _dev(dict(o_tm1=rng.standard_normal((64, 24)).astype(np.float32),
                      a_tm1=rng.uniform(-1, 1, (64, 6)).astype(np.float32),
                      r_t=rng.uniform(0, 5, 64).astype(np.float32),
                      d_t=np.full(64, 0.99 ** 4, np.float32),
                      o_t=rng.standard_normal((64, 24)).astype(np.float32)))
    learner.native.step(*batch)  # generated noise: same seed, same step number
    other.native.step(*batch)
    torch.cuda.synchronize()
    for which in ("params", "target", "m", "v"):
        x, y = learner.native.get_params(which), other.native.get_params(which)
        for k in x:
            if which == "target" and k.startswith("mpo/"):
                continue
            np.testing.assert_array_equal(x[k], y[k], err_msg=f"{which}/{k}")


def test_agent_runs_in_environment_loop():
    """The reference's agent test (acme/agents/tf/mpo/agent_test.py:52-77), run-only: small
    networks on the fake bounded continuous environment, batch_size 10, num_samples 5."""
    from acme_amd import specs
    from acme_amd.agents.mpo import MPO
    from acme_amd.environment_loop import EnvironmentLoop
    from acme_amd.networks import make_mpo_networks
    from acme_amd.testing import fakes
    from acme_amd.utils import loggers
    env = fakes.ContinuousEnvironment(episode_length=10, bounded=True)
    spec = specs.make_environment_spec(env)
    nets = make_mpo_networks(24, spec.actions, (12, 12), (12, 12))
    agent = MPO(spec, nets["policy"], nets["critic"], batch_size=10, samples_per_insert=2,
                min_replay_size=10, num_samples=5, logger=loggers.NoOpLogger())
    loop = EnvironmentLoop(env, agent, logger=loggers.NoOpLogger())
    loop.run(num_episodes=2)
    learner = agent._learner  # noqa: SLF001
    torch.cuda.synchronize()
    assert learner.num_steps >= 1
    assert np.isfinite(learner.native.critic_loss.item())
    assert np.isfinite(learner.native.policy_loss.item())
    assert np.isfinite(learner.native.stats.cpu().numpy()).all()
