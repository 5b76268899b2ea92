"""HIP CRR learner step vs the numpy oracle (tests/crr_oracle.py, float64).

Reference: RCRRLearner._step (acme/agents/tf/crr/recurrent_learning.py:197-377) with stateless
networks, over the R = B (T - 1) transitions its loop unrolls into.  Every step here is
teacher-forced with explicit eps unless it says otherwise; online and target parameters are
drawn independently.

Tolerances: those of tests/test_dmpo_gpu.py and tests/test_d4pg_gpu.py, fp32
kernels against an fp64 restatement:
  the three outputs, every debug buffer, both global norms: rtol 1e-5 (+ an atol of 2e-6 times
      the tensor's largest magnitude)
  gradients: per tensor |g - g_ref| <= 1e-4 |g_ref| + 2e-5 max|g_ref|
  Adam-updated params: every element within 2 lr of the oracle's and 99% within 1e-5 relative
MPO's allowance applies to the sums of signed terms on the policy side and to nothing else
(dmean, dpre, the policy gradients): they may miss the criterion above only by 4x the float32
oracle's own error against float64 at that shape.  Nothing of the critic side has an allowance.

The inputs are tests/crr_cases.py's: narrow asymmetric supports so that the projection clips
below, above and not at all in every batch (asserted per batch), critic heads scaled 4x and
init_scale 1.0.  tests/test_crr_oracle_cpu.py checks without a GPU that the binary mode's
batches keep every |advantage| at least 1e-3 of the support's width and that the exp batch
overflows a float32 exp.

Worst values seen on the MI355X over this file are in DESIGN.md §4.2 "CRR".
"""

import ctypes

import numpy as np
import pytest
import torch

from tests import crr_cases as C
from tests import crr_oracle as O
from tests.test_mpo_gpu import (_MISSES, _check_params, _close, _dev, _philox4x32_10,  # noqa: F401
                                _report_all_misses, _state)

pytestmark = pytest.mark.gpu

CRR_NOISE_TAG = 0x4352524E


def _native(cfg, R, **kw):
    from acme_amd.native import NativeCRR
    args = dict(obs_dim=cfg.obs_dim, act_dim=cfg.act_dim, max_batch=R,
                sequence_length=cfg.sequence_length, policy_sizes=cfg.policy_sizes,
                critic_sizes=cfg.critic_sizes, num_atoms=cfg.num_atoms, vmin=cfg.vmin,
                vmax=cfg.vmax, discount=cfg.discount,
                target_update_period=cfg.target_update_period,
                num_action_samples_td_learning=cfg.num_action_samples_td_learning,
                num_action_samples_policy_weight=cfg.num_action_samples_policy_weight,
                baseline_reduce_function=cfg.baseline_reduce_function,
                policy_improvement_modes=cfg.policy_improvement_modes,
                ratio_upper_bound=cfg.ratio_upper_bound, beta=cfg.beta,
                policy_learning_rate=cfg.policy_lr, critic_learning_rate=cfg.critic_lr,
                clipping=cfg.clipping, init_scale=cfg.init_scale, min_scale=cfg.min_scale)
    args.update(kw)
    return NativeCRR(**args)


class _Ref:
    """One oracle step in float64, and in float32 for the allowance of the cancelling sums."""

    def __init__(self, cfg, state, batch, eps):
        self.out, self.raw, self.state = O.crr_step(cfg, state, batch, eps, np.float64)
        self.out32, self.raw32, _ = O.crr_step(cfg, state, batch, eps, np.float32)

    def f32_err(self, key, grad=False):
        """4x the float32 oracle's own max error against float64 for one quantity."""
        a, b = (self.raw32[key], self.raw[key]) if grad else (self.out32[key], self.out[key])
        return 4.0 * float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def _check_buffers(n, ref, cfg, R, tag=""):
    """The three outputs and every debug buffer of the step against the oracle's `out`."""
    Ntd, Npw = cfg.num_action_samples_td_learning, cfg.num_action_samples_policy_weight
    A, K, out = cfg.act_dim, cfg.num_atoms, ref.out
    buf = n.debug_buffer
    for k, got in (("critic_loss", n.critic_loss), ("policy_loss", n.policy_loss),
                   ("policy_loss_coef", n.policy_loss_coef)):
        _close(got.item(), out[k], name=f"{k}{tag}")
    for name in ("mean_on", "std_on", "pre_on", "mean_t", "std_t"):
        _close(buf(name)[:R * A], out[name], name=f"{name}{tag}")
    _close(buf("actions")[:(Ntd + Npw) * R * A], out["actions"], name=f"actions{tag}")
    # The categorical critic and what the coefficient is made of: no allowance.
    sizes = (("logits_tm1", R * K), ("sampled_logits", Ntd * R * K),
             ("policy_sampled_logits", Npw * R * K), ("sampled_q", Ntd * R), ("mixture", R * K),
             ("ce", R), ("dlogits", R * K), ("q_tm1_mean", R), ("v_estimate", R),
             ("advantage", R), ("coef", R), ("logp", R))
    for name, count in sizes:
        got = buf(name)
        assert got.size == count or n.max_batch != R, (name, got.size, count)
        _close(got[:count], out[name], name=f"{name}{tag}")
    _close(buf("dmean")[:R * A], out["dmean"], name=f"dmean{tag}", extra=ref.f32_err("dmean"))
    _close(buf("dpre")[:R * A], out["dpre"], name=f"dpre{tag}", extra=ref.f32_err("dpre"))
    _close(buf("norms"), out["norms"], name=f"norms{tag}")


def _check_grads(n, ref):
    g = n.get_params("grads")
    for name, r in ref.raw.items():
        got = g[name].reshape(r.shape).astype(np.float64)
        scale = np.abs(r).max()
        err = np.abs(got - r)
        # The policy's gradients carry the signed sums of dmean / dpre; the critic's none.
        extra = ref.f32_err(name, grad=True) if name.startswith("policy/") else 0.0
        bound = 1e-4 * np.abs(r) + 2e-5 * scale + 1e-30 + extra
        print(f"grad {name}: max |err| {float(err.max()):.3e}, scale {float(scale):.3e}, "
              f"f32-oracle allowance {extra:.3e}")
        if not (err <= bound).all():
            _MISSES.append(("grad " + name, float(err.max()), float(scale), extra))


def _step_and_check(n, cfg, state, batch, eps, tag="", check_branches=True):
    """One teacher-forced step of `n` from `state` against the oracle; returns the reference and
    the state the next step continues from (the kernel's parameters and moments, so fp32 drift
    cannot compound)."""
    R, s = len(batch["r_t"]), state["num_steps"]
    if check_branches:
        C.assert_projection_branches(cfg, batch)
    before = n.get_params("target")
    n.step(*_dev(batch), noise=torch.as_tensor(eps).cuda())
    torch.cuda.synchronize()
    ref = _Ref(cfg, state, batch, eps)
    np.testing.assert_array_equal(n.debug_buffer("noise")[:eps.size], eps.ravel())
    _check_buffers(n, ref, cfg, R, tag=tag)
    _check_grads(n, ref)
    got, tgt = n.get_params("params"), n.get_params("target")
    _check_params(cfg, got, ref.state["params"])
    # The post-update copy: on the period the target is the UPDATED online network, bit for bit;
    # off it the target is what it was.
    copied = s % cfg.target_update_period == 0
    for k in got:
        np.testing.assert_array_equal(tgt[k], got[k] if copied else before[k], err_msg=k)
        if not copied:
            assert np.abs(tgt[k] - got[k]).max() > 0, k
    assert n.num_steps == s + 1
    new = dict(params={k: got[k].astype(np.float32) for k in got}, target=tgt,
               m=n.get_params("m"), v=n.get_params("v"), num_steps=s + 1)
    return ref, new


def _run_steps(cfg, B, steps, pseed, bseed, start=0, **kw):
    T = cfg.sequence_length
    R = B * (T - 1)
    n = _native(cfg, R)
    params, target = C.random_params(cfg, pseed), C.random_params(cfg, pseed + 1)
    n.set_params(params, target)
    n.num_steps = start
    state = _state(params, target, start)
    refs = []
    for s in range(start, start + steps):
        batch = O.flatten_sequences(C.sequences(cfg, B, bseed + s))
        ref, state = _step_and_check(n, cfg, state, batch, C.noise(cfg, R, bseed + 100 + s),
                                     tag=f"@{s}", **kw)
        refs.append(ref)
    return n, refs


def test_tensor_layout_matches_oracle():
    cfg = O.CRRConfig(sequence_length=3)
    n = _native(cfg, 8)
    assert [(k, s) for k, _, s in n.tensors] == O.crr_tensor_shapes(cfg)
    assert n.policy_size == [o for k, o, _ in n.tensors if k.startswith("critic/")][0]
    assert not any(k.startswith("mpo/") for k, _, _ in n.tensors)  # no dual variables
    np.testing.assert_array_equal(n.values, O.support(cfg, np.float32))
    assert n.debug_buffer("policy_sampled_logits").size == 8 * 4 * cfg.num_atoms
    assert n.debug_buffer("noise").size == 8 * 5 * cfg.act_dim
    assert n.debug_buffer("losses").size == 3  # the outputs' place when the caller passes none
    with pytest.raises(ValueError, match="unknown debug buffer"):
        n.debug_buffer("weights")


def test_create_rejects_too_many_rows():
    from acme_amd import _lib
    with pytest.raises(ValueError, match="max_batch \\* \\(1 \\+ max"):
        _native(O.CRRConfig(num_action_samples_policy_weight=64), _lib.MPO_MAX_ROWS // 65 + 1)
    _native(O.CRRConfig(policy_sizes=(16,), critic_sizes=(16,), num_atoms=2,
                        num_action_samples_policy_weight=64), 2 * (_lib.MPO_MAX_ROWS // 130))


def test_golden_step():
    from tests.golden.make_crr_golden import golden_cfg, unpack
    import os
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "crr_step_b4.npz"))
    cfg = golden_cfg()
    params, target, seq, eps = unpack(cfg, z)
    batch = O.flatten_sequences(seq)
    n = _native(cfg, len(batch["r_t"]))
    n.set_params(params, target)
    n.num_steps = 1  # no target copy; Adam t = 2
    ref, _ = _step_and_check(n, cfg, _state(params, target, 1), batch, eps)
    # The fixture is what the oracle computes (tests/test_crr_oracle_cpu.py checks every entry).
    np.testing.assert_allclose(ref.out["policy_loss"], z["out/policy_loss"], rtol=1e-12)
    np.testing.assert_allclose(ref.out["coef"], z["out/coef"], rtol=1e-10, atol=1e-15)
    _check_params(cfg, n.get_params("params"),
                  {k[len("out/new/"):]: z[k] for k in z.files if k.startswith("out/new/")})


@pytest.mark.parametrize("B,T,Ntd,Npw,A,K,steps,period", C.SHAPES)
def test_steps_match_oracle(B, T, Ntd, Npw, A, K, steps, period):
    """(5, 2, 1, 4, 3, 51): rows not a multiple of the row kernels' 4; (19, 3, 3, 2, 6, 21): more
    than one block, N not a power of two; (8, 2, 1, 64, 1, 64): a full wave of atoms and the
    largest N_pw; (3, 3, 64, 1, 16, 2): the largest N_td, the widest action, the smallest
    support; (4, 5, 2, 3, 2, 5): three steps with period 2, so the post-update copy happens
    after steps 0 and 2 and not after step 1 (asserted bit for bit by _step_and_check)."""
    cfg = C.small_cfg(T, Ntd, Npw, A, K, target_update_period=period)
    _run_steps(cfg, B, steps, 1, 10)


def test_full_size_step_matches_oracle():
    """The timing tool's shapes: B = 128, T = 3 (R = 256), N_td = 1, N_pw = 4, 51 atoms, 24-dim
    observations, policy 256x3, critic 512/512/256; one step, which ends with the copy.  The
    support is the small cases' [-1, 5], so that the projection's three branches run here too
    (on [-150, 150] with rewards in [0, 5] nothing clips)."""
    cfg = O.CRRConfig(sequence_length=3, target_update_period=2, vmin=-1.0, vmax=5.0,
                      init_scale=1.0)
    n = _native(cfg, 256)
    params, target = C.random_params(cfg, 3), C.random_params(cfg, 4)
    n.set_params(params, target)
    batch = O.flatten_sequences(C.sequences(cfg, 128, 30))
    _step_and_check(n, cfg, _state(params, target, 0), batch, C.noise(cfg, 256, 130))


@pytest.mark.parametrize("mode", O.MODES)
@pytest.mark.parametrize("reduce", O.REDUCE)
def test_modes(reduce, mode):
    """All nine reduce x improvement-mode combinations at (19, 3, 3, 2, 6, 21)."""
    cfg, params, target, batch, eps = C.mode_case(reduce, mode)
    n = _native(cfg, len(batch["r_t"]))
    n.set_params(params, target)
    n.num_steps = 1
    ref, _ = _step_and_check(n, cfg, _state(params, target, 1), batch, eps)
    coef = n.debug_buffer("coef")
    if mode == "binary":
        C.assert_binary_margin(cfg, ref.out)
        np.testing.assert_array_equal(coef, ref.out["coef"])  # every row, exactly 0 or 1
    elif mode == "all":
        assert (coef == 1.0).all()
    else:
        clipped = ref.out["coef"] == cfg.ratio_upper_bound
        assert clipped.any() and not clipped.all()


def test_exp_coefficient_is_the_bound_where_exp_overflows():
    """beta = 0.01: some advantages are above beta log(bound), some so large that a float32 exp
    overflows; the coefficient is exactly the bound there, and nothing is NaN."""
    cfg, params, target, batch, eps = C.mode_case("mean", "exp", C.OVERFLOW_SEEDS, **C.OVERFLOW)
    n = _native(cfg, len(batch["r_t"]))
    n.set_params(params, target)
    n.num_steps = 1
    ref, _ = _step_and_check(n, cfg, _state(params, target, 1), batch, eps)
    C.assert_overflow_batch(cfg, ref.out)
    x = n.debug_buffer("advantage") / np.float32(cfg.beta)
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(x.astype(np.float32))).any()
    coef = n.debug_buffer("coef")
    bound = np.float32(cfg.ratio_upper_bound)
    assert (coef[ref.out["coef"] == cfg.ratio_upper_bound] == bound).all()
    assert np.isfinite(coef).all() and np.isfinite(n.policy_loss.item())
    for k, v in n.get_params("params").items():
        assert np.isfinite(v).all(), k


def test_clipping_on_and_off_with_large_norms():
    """The first linear layer of both online networks scaled down 250x: the LayerNorm undoes the
    scale in the forward pass and multiplies that layer's gradient by it, so both global norms
    exceed 40.  clipping=True scales the gradients down, clipping=False leaves them."""
    B, T = 8, 3
    base = C.small_cfg(T, 2, 4, 3, 9)
    params, target = C.random_params(base, 5), C.random_params(base, 6)
    for net in ("policy", "critic"):
        for k in (f"{net}/layer_norm_mlp/linear/w", f"{net}/layer_norm_mlp/linear/b"):
            params[k] = params[k] * np.float32(0.004)
    new = {}
    for clipping in (False, True):
        cfg = C.small_cfg(T, 2, 4, 3, 9, clipping=clipping)
        n = _native(cfg, B * (T - 1))
        n.set_params(dict(params), dict(target))
        n.num_steps = 1
        batch = O.flatten_sequences(C.sequences(cfg, B, 60))
        ref, _ = _step_and_check(n, cfg, _state(dict(params), dict(target), 1), batch,
                                 C.noise(cfg, B * (T - 1), 160))
        assert min(ref.out["norms"]) > 40.0, ref.out["norms"]
        new[clipping] = n.get_params("m")
    for k in ("policy/layer_norm_mlp/linear/w", "critic/layer_norm_mlp/linear/w"):
        assert np.abs(new[True][k]).max() < np.abs(new[False][k]).max()


def _noise_ref(seed, step, count):
    """include/acme_hip.h "Sampling noise" under CRR's tag, Box-Muller in float64."""
    idx = np.arange((count + 3) // 4)
    x, y, z, w = _philox4x32_10(idx, step, CRR_NOISE_TAG, seed)

    def pair(a, b):
        u1 = ((a >> np.uint64(8)).astype(np.float64) + 1.0) / 2.0 ** 24
        u2 = (b >> np.uint64(8)).astype(np.float64) / 2.0 ** 24
        rad = np.sqrt(-2.0 * np.log(u1))
        return rad * np.cos(2 * np.pi * u2), rad * np.sin(2 * np.pi * u2)

    z0, z1 = pair(x, y)
    z2, z3 = pair(z, w)
    return np.stack([z0, z1, z2, z3], axis=1).ravel()[:count]


def test_generated_noise():
    """noise=None: the "noise" buffer is the documented Philox / Box-Muller stream of (seed,
    step) under CRR's own tag to MPO's 4e-6 absolute bound, differs between two consecutive
    (graph-replayed) steps and from MPO's stream, and passed back as explicit noise reproduces
    the step bit for bit."""
    B, T, seed = 32, 3, 0x123456789ABCDEF
    cfg = C.small_cfg(T, 16, 16, 6, 21, policy_sizes=(32, 32), critic_sizes=(32, 32),
                      target_update_period=100)
    R = B * (T - 1)
    count = 32 * R * cfg.act_dim
    assert count >= 10 ** 4
    params, target = C.random_params(cfg, 1), C.random_params(cfg, 2)
    batch = _dev(O.flatten_sequences(C.sequences(cfg, B, 3)))
    n = _native(cfg, R, seed=seed)
    n.set_params(params, target)
    noises, before = [], None
    for s in range(3):  # step 0 copies the target; step 1 captures the no-copy graph, 2 replays it
        if s == 2:
            before = {w: n.get_params(w) for w in ("params", "target", "m", "v")}
        n.step(*batch)
        torch.cuda.synchronize()
        got = n.debug_buffer("noise")[:count].astype(np.float64)
        ref = _noise_ref(seed, s, count)
        print(f"step {s}: max |noise - ref| {np.abs(got - ref).max():.3e}")
        assert np.abs(got - ref).max() <= 4e-6
        noises.append(got)
    assert np.abs(noises[1] - noises[2]).max() > 1.0
    from tests.test_mpo_gpu import _noise_ref as mpo_noise_ref
    assert np.abs(noises[2] - mpo_noise_ref(seed, 2, count)).max() > 1.0
    after = n.get_params("params")
    m = _native(cfg, R, seed=seed + 1)
    m.set_params(before["params"], before["target"])
    for buf, src in ((m.m, before["m"]), (m.v, before["v"])):
        for k, t in m.views(buf).items():
            t.copy_(torch.as_tensor(src[k]).view(t.shape))
    m.num_steps = 2
    m.step(*batch, noise=torch.as_tensor(n.debug_buffer("noise")[:count]).cuda())
    torch.cuda.synchronize()
    for k, v in m.get_params("params").items():
        np.testing.assert_array_equal(v, after[k], err_msg=k)


@pytest.mark.parametrize("explicit", [True, False])
def test_graph_replay_matches_eager(explicit):
    """The captured step graphs (default) and the eager launch sequence (forced by the section
    profiler, as in tests/test_mpo_gpu.py) give bit-identical results over 6 steps with the copy
    period in play, with explicit and with generated noise, and two alternating batch buffers."""
    from acme_amd import _lib
    B, T = 32, 3
    cfg = C.small_cfg(T, 2, 4, 6, 51, policy_sizes=(64, 64, 64), critic_sizes=(128, 128, 64),
                      target_update_period=2)
    R = B * (T - 1)
    params, target = C.random_params(cfg, 11), C.random_params(cfg, 12)
    batches = [_dev(O.flatten_sequences(C.sequences(cfg, B, 20 + i))) for i in range(2)]
    eps = [torch.as_tensor(C.noise(cfg, R, 30 + i)).cuda() for i in range(2)]
    results = []
    for eager in (True, False):
        n = _native(cfg, R, seed=7)
        n.set_params(params, target)
        noises = []
        _lib.lib().acme_profile_enable(1 if eager else 0)
        try:
            for s in range(6):
                # Steps 1 and 5 use the same buffers without a copy: step 5 replays step 1's graph.
                i = 0 if s in (1, 5) else s % 2
                n.step(*batches[i], noise=eps[i] if explicit else None)
                torch.cuda.synchronize()
                noises.append(n.debug_buffer("noise").copy())
        finally:
            _lib.lib().acme_profile_enable(0)
        results.append((n.get_params("params"), n.get_params("target"), n.get_params("m"),
                        n.get_params("v"), noises, n.debug_buffer("coef"),
                        n.debug_buffer("mixture"),
                        (n.critic_loss.item(), n.policy_loss.item(), n.policy_loss_coef.item())))
        if not explicit:
            assert np.abs(noises[1] - noises[5]).max() > 1.0
    a, b = results
    for which in range(4):
        for k in a[which]:
            np.testing.assert_array_equal(a[which][k], b[which][k], err_msg=k)
    for x, y in zip(a[4], b[4]):
        np.testing.assert_array_equal(x, y)
    for i in (5, 6):
        np.testing.assert_array_equal(a[i], b[i])
    assert a[7] == b[7]


def test_neighbours_unchanged_beside_crr():
    """D4PG, DDPG, MPO and DMPO learners stepping in turn with a CRR learner in one process give
    the bits they give alone (the form of test_neighbours_unchanged_beside_dmpo)."""
    from acme_amd.native import NativeD4PG, NativeDDPG, NativeDMPO, NativeMPO
    from oracle import d4pg_oracle as O4
    from tests import ddpg_oracle as OD
    from tests import dmpo_oracle as OX
    from tests import mpo_oracle as OM
    from tests.test_dmpo_gpu import _batch as dmpo_batch
    from tests.test_dmpo_gpu import _random_params as dmpo_params
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
    cx = OX.DMPOConfig(num_samples=4, **sizes)
    px, tx = dmpo_params(cx, 1), dmpo_params(cx, 2)
    batches = [_dev(dmpo_batch(cx, 32, 40 + i)) for i in range(3)]

    def make():
        a = NativeD4PG(obs_dim=24, act_dim=6, max_batch=32, target_update_period=2, **sizes)
        a.set_params(p4, p4)
        b = NativeDDPG(obs_dim=24, act_dim=6, max_batch=32, target_update_period=2, **sizes)
        b.set_params(pd, pd)
        kw = dict(obs_dim=24, act_dim=6, max_batch=32, num_samples=4,
                  target_policy_update_period=2, target_critic_update_period=3, seed=5, **sizes)
        c = NativeMPO(**kw)
        c.set_params(pm, tm)
        d = NativeDMPO(**kw)
        d.set_params(px, tx)
        return a, b, c, d

    alone = make()
    for bt in batches:
        for x in alone:
            x.step(*bt)
    torch.cuda.synchronize()
    cc = O.CRRConfig(sequence_length=3, target_update_period=2, **sizes)
    beside, crr = make(), _native(cc, 32)
    crr.set_params(C.random_params(cc, 1), C.random_params(cc, 2))
    for bt in batches:
        crr.step(*bt)
        for x in beside:
            x.step(*bt)
    crr.step(*batches[0])
    torch.cuda.synchronize()
    assert crr.num_steps == 4 and np.isfinite(crr.critic_loss.item())
    for x, y in zip(alone, beside):
        assert y.num_steps == 3
        for which in ("params", "target", "m", "v"):
            a, b = x.get_params(which), y.get_params(which)
            for k in a:
                np.testing.assert_array_equal(a[k], b[k], err_msg=f"{which}/{k}")
        assert x.critic_loss.item() == y.critic_loss.item()
        assert x.policy_loss.item() == y.policy_loss.item()


def test_call_refusals():
    """R not a multiple of T - 1, and a handle of another kind passed to acme_crr_step (or a CRR
    handle to another kind's step): ACME_ERR_INVALID, nothing stepped, parameters unchanged."""
    from acme_amd import _lib
    from tests import dmpo_oracle as OX
    from tests.test_dmpo_gpu import _native as dmpo_native
    from tests.test_dmpo_gpu import _random_params as dmpo_params
    cfg = C.small_cfg(3, 1, 4, 3, 9)
    n = _native(cfg, 8)
    n.set_params(C.random_params(cfg, 1), C.random_params(cfg, 2))
    batch = O.flatten_sequences(C.sequences(cfg, 4, 3))
    before = {w: n.get_params(w) for w in ("params", "target", "m", "v")}
    with pytest.raises(ValueError, match="not a multiple of sequence_length - 1 = 2"):
        n.step(*[t[:5].contiguous() for t in _dev(batch)])
    cx = OX.DMPOConfig(obs_dim=7, act_dim=3, policy_sizes=(36, 100), critic_sizes=(64, 44),
                       num_samples=3, num_atoms=9, vmin=-1.0, vmax=5.0)
    dmpo = dmpo_native(cx, 8)
    dmpo.set_params(dmpo_params(cx, 1), dmpo_params(cx, 2))
    dbefore = dmpo.get_params("params")
    L = _lib.lib()
    bt, out = _lib.MPOBatch(), _lib.CRROutputs()
    dev = _dev(batch)
    bt.o_tm1, bt.a_tm1, bt.r_t, bt.d_t, bt.o_t = [t.data_ptr() for t in dev]
    bt.batch = 8
    assert L.acme_crr_step(dmpo._h, ctypes.byref(bt), ctypes.byref(out), None) == \
        _lib.ACME_ERR_INVALID  # noqa: SLF001
    assert b"acme_dmpo_step" in L.acme_last_error()
    mout = _lib.MPOOutputs()
    h = n._h  # noqa: SLF001
    for fn in (L.acme_mpo_step, L.acme_dmpo_step):
        assert fn(h, ctypes.byref(bt), ctypes.byref(mout), None) == _lib.ACME_ERR_INVALID
        assert b"acme_crr_step" in L.acme_last_error()
    d4 = _lib.D4PGBatch()
    assert L.acme_d4pg_step(h, ctypes.byref(d4), None, None) == _lib.ACME_ERR_INVALID
    assert b"acme_crr_step" in L.acme_last_error()
    torch.cuda.synchronize()
    assert n.num_steps == 0 and dmpo.num_steps == 0
    for w, ref in before.items():
        for k, v in n.get_params(w).items():
            np.testing.assert_array_equal(v, ref[k], err_msg=f"{w}/{k}")
    for k, v in dmpo.get_params("params").items():
        np.testing.assert_array_equal(v, dbefore[k], err_msg=k)
    # The same learner still steps.
    n.step(*dev)
    torch.cuda.synchronize()
    assert n.num_steps == 1 and np.isfinite(n.policy_loss.item())


@pytest.mark.parametrize("outputs", ["none", "coef_null"])
def test_losses_buffer_when_the_caller_passes_no_outputs(outputs):
    """acme_crr_step with out == NULL, or with a null policy_loss_coef only: the sums go to the
    "losses" debug buffer (critic loss, policy loss, mean coefficient) and match the oracle at
    the outputs' bar; the step itself is the one a caller with outputs gets, bit for bit."""
    from acme_amd import _lib
    cfg, params, target, batch, eps = C.mode_case("max", "exp")
    R = len(batch["r_t"])
    ref = _Ref(cfg, _state(params, target, 1), batch, eps)
    dev, noise = _dev(batch), torch.as_tensor(eps).cuda()
    with_out = _native(cfg, R)
    with_out.set_params(params, target)
    with_out.num_steps = 1
    with_out.step(*dev, noise=noise)
    n = _native(cfg, R)
    n.set_params(params, target)
    n.num_steps = 1
    bt = _lib.MPOBatch()
    bt.o_tm1, bt.a_tm1, bt.r_t, bt.d_t, bt.o_t = [t.data_ptr() for t in dev]
    bt.batch, bt.noise = R, noise.data_ptr()
    out = _lib.CRROutputs()
    if outputs == "coef_null":
        out.critic_loss, out.policy_loss = n.critic_loss.data_ptr(), n.policy_loss.data_ptr()
    arg = None if outputs == "none" else ctypes.byref(out)
    _lib.check(_lib.lib().acme_crr_step(n._h, ctypes.byref(bt), arg, None))  # noqa: SLF001
    torch.cuda.synchronize()
    losses = n.debug_buffer("losses")
    assert losses.shape == (3,)
    names = ("critic_loss", "policy_loss", "policy_loss_coef")
    for i, k in enumerate(names):
        if outputs == "coef_null" and i < 2:
            _close(getattr(n, k).item(), ref.out[k], name=k)
            assert getattr(n, k).item() == getattr(with_out, k).item()
        else:
            _close(losses[i], ref.out[k], name=f"losses/{k}")
            assert losses[i] == getattr(with_out, k).item(), k
    if outputs == "coef_null":
        assert n.policy_loss_coef.item() == 0.0  # not the caller's: left alone
    for k, v in n.get_params("params").items():
        np.testing.assert_array_equal(v, with_out.get_params("params")[k], err_msg=k)


def test_learner_end_to_end():
    """CRRLearner over an offline dataset: a sequence table (T = 3) filled once through a
    SequenceAdder, batches of B = 4 through make_reverb_dataset; three steps, the logged keys,
    get_variables' names and TARGET values, and save -> restore -> step equal to the
    uninterrupted run bit for bit."""
    from acme_amd import dm_env, replay, specs
    from acme_amd.adders import reverb as adders
    from acme_amd.agents.crr import CRRLearner, RCRRLearner
    from acme_amd.datasets import make_reverb_dataset
    from acme_amd.networks import make_dmpo_networks
    from acme_amd.utils import loggers
    B, T, od, A = 4, 3, 24, 6
    spec = specs.EnvironmentSpec(
        observations=specs.Array((od,), np.float32),
        actions=specs.BoundedArray((A,), np.float32, -1.0, 1.0),
        rewards=specs.Array((), np.float32), discounts=specs.BoundedArray((), np.float32, 0, 1))
    table = replay.Table(adders.DEFAULT_PRIORITY_TABLE, replay.selectors.Uniform(),
                         replay.selectors.Fifo(), 256, replay.rate_limiters.MinSize(1),
                         signature=adders.SequenceAdder.signature(spec), seed=7)
    server = replay.Server([table], port=None)
    adder = adders.SequenceAdder(client=replay.Client(server), period=T - 1, sequence_length=T)
    rng = np.random.default_rng(0)
    for _ in range(4):
        adder.add_first(dm_env.restart(rng.standard_normal(od).astype(np.float32)))
        for t in range(9):
            r, o = np.float32(rng.standard_normal()), rng.standard_normal(od).astype(np.float32)
            ts = dm_env.termination(r, o) if t == 8 else dm_env.transition(r, o, np.float32(1.0))
            adder.add(rng.uniform(-1, 1, A).astype(np.float32), ts)
    table.flush()
    assert table.size() >= 2 * B and table.sequence_length == T
    nets = make_dmpo_networks(od, spec.actions, (64, 64), (128, 64), vmin=-10.0, vmax=10.0,
                              num_atoms=21)
    log = loggers.InMemoryLogger()
    assert RCRRLearner is CRRLearner

    def make(logger):
        return CRRLearner(nets["policy"], nets["critic"], nets["policy"], nets["critic"],
                          dataset=make_reverb_dataset(server, batch_size=B, sequence_length=T),
                          target_update_period=2, num_action_samples_td_learning=2,
                          logger=logger, seed=0)

    with pytest.raises(ValueError, match="batch_size is 5 but the dataset yields batches of 4"):
        CRRLearner(nets["policy"], nets["critic"], nets["policy"], nets["critic"], batch_size=5,
                   dataset=make_reverb_dataset(server, batch_size=B, sequence_length=T))
    learner = make(log)
    n = learner.native
    assert (n.sequence_length, n.max_batch, n.cfg.num_atoms) == (T, B * (T - 1), 21)
    targets = []
    for _ in range(3):
        learner.step()
        torch.cuda.synchronize()
        targets.append((n.get_params("target"), n.get_params("params")))
    assert learner.num_steps == 3
    row = log.data[-1]
    for k in ("critic_loss", "policy_loss", "policy_loss_coef", "steps"):
        assert np.isfinite(row[k]), k
    assert 0 < row["policy_loss_coef"] <= 20.0 * (T - 1) / T
    # Post-update copies with period 2: target == online after steps 0 and 2, not after step 1.
    for s, (tgt, onl) in enumerate(targets):
        same = all(np.array_equal(tgt[k], onl[k]) for k in tgt)
        assert same == (s % 2 == 0), s
    crit, pol = learner.get_variables(["critic", "policy"])
    assert all(k.startswith("critic/") for k in crit) and len(crit) == 8
    assert all(k.startswith("policy/") for k in pol) and len(pol) == 10
    assert crit["critic/discrete_valued_head/linear/w"].shape == (64, 21)
    for k, v in {**crit, **pol}.items():
        np.testing.assert_array_equal(v, targets[-1][0][k], err_msg=k)  # the TARGET networks
    mean, stddev = learner.policy_distribution(np.zeros((2, od), np.float32))
    assert mean.shape == (2, A) and stddev.shape == (2, A) and (stddev > 0).all()
    saved = learner.save()
    other = make(loggers.NoOpLogger())
    for buf in (other.native.params, other.native.target, other.native.m, other.native.v):
        buf.add_(1.0)
    other.restore(saved)
    assert other.num_steps == 3
    # The same step from the restored state gives the same bits (generated noise: same seed,
    # same step number).
    sample = next(iter(make_reverb_dataset(server, batch_size=B, sequence_length=T)))
    batch = [t.clone() for t in CRRLearner.flatten(sample)]
    assert batch[0].shape == (B * (T - 1), od)
    np.testing.assert_array_equal(batch[4][1].cpu().numpy(),
                                  sample.data.observation[0, 2].cpu().numpy())
    learner.native.step(*batch)
    other.native.step(*batch)
    torch.cuda.synchronize()
    for which in ("params", "target", "m", "v"):
        x, y = learner.native.get_params(which), other.native.get_params(which)
        for k in x:
            np.testing.assert_array_equal(x[k], y[k], err_msg=f"{which}/{k}")
    assert learner.native.policy_loss.item() == other.native.policy_loss.item()
