"""HIP DDPG learner step vs the numpy oracle (tests/ddpg_oracle.py, float64).

Reference: DDPGLearner._step (acme/agents/tf/ddpg/learning.py:143-237).
Tolerances (fp32 kernels against an fp64 restatement), those of tests/test_d4pg_gpu.py:
  losses, q values, actions, td, dqda, global norms: rtol 1e-5 (+ an atol of 2e-6 times the
      tensor's largest magnitude, the fp32 rounding floor of its scale)
  gradients: per tensor |g - g_ref| <= 1e-4 |g_ref| + 2e-5 max|g_ref|
  Adam-updated params: every element within 2 lr of the oracle's and 99% within
      1e-5 relative (Adam normalises each gradient element, so elements whose gradient
      sits at the fp32 rounding floor may take a different sign).
"""

import os

import numpy as np
import pytest
import torch

from tests import ddpg_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ddpg_step_b8.npz")


def _native(cfg, B, **kw):
    from acme_amd.native import NativeDDPG
    return NativeDDPG(obs_dim=cfg.obs_dim, act_dim=cfg.act_dim, max_batch=B,
                      policy_sizes=cfg.policy_sizes, critic_sizes=cfg.critic_sizes,
                      action_min=cfg.action_min, action_max=cfg.action_max,
                      discount=cfg.discount, target_update_period=cfg.target_update_period,
                      policy_learning_rate=cfg.policy_lr, critic_learning_rate=cfg.critic_lr,
                      clipping=cfg.clipping, **kw)


def _dev(batch):
    return [torch.as_tensor(batch[k]).cuda().contiguous()
            for k in ("o_tm1", "a_tm1", "r_t", "d_t", "o_t")]


def _close(got, ref, rtol=1e-5, floor=2e-6, name=""):
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    scale = max(float(np.abs(ref).max()), 1e-30)
    err = float(np.abs(got - ref).max())
    print(f"{name}: max |err| {err:.3e}, scale {scale:.3e}")
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=floor * scale, err_msg=name)


def _check_grads(native, g_ref):
    g = native.get_params("grads")
    for name, ref in g_ref.items():
        got = g[name].reshape(ref.shape).astype(np.float64)
        scale = np.abs(ref).max()
        err = np.abs(got - ref)
        bound = 1e-4 * np.abs(ref) + 2e-5 * scale + 1e-30
        assert (err <= bound).all(), (name, float(err.max()), float(scale))


def _check_params(got, ref, lr):
    for k, r in ref.items():
        gk = got[k].reshape(r.shape).astype(np.float64)
        err = np.abs(gk - r)
        assert err.max() <= 2 * lr + 1e-6, (k, float(err.max()))
        frac = np.mean(err <= 1e-5 * np.abs(r) + 1e-7)
        assert frac >= 0.99, (k, frac)


def _random_params(cfg, seed):
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in O.ddpg_tensor_shapes(cfg):
        if name.endswith("/scale"):
            v = 1.0 + 0.1 * rng.standard_normal(shape)
        elif name.endswith("/b") or name.endswith("/offset"):
            v = 0.1 * rng.standard_normal(shape)
        else:
            v = rng.standard_normal(shape) / np.sqrt(shape[0])
        out[name] = v.astype(np.float32)
    return out


def _batch(cfg, B, seed):
    rng = np.random.default_rng(seed)
    d = np.where(rng.random(B) < 0.05, 0.0, 0.99 ** 4).astype(np.float32)
    return dict(o_tm1=rng.standard_normal((B, cfg.obs_dim)).astype(np.float32),
                a_tm1=rng.uniform(-1, 1, (B, cfg.act_dim)).astype(np.float32),
                r_t=rng.uniform(0, 5, B).astype(np.float32), d_t=d,
                o_t=rng.standard_normal((B, cfg.obs_dim)).astype(np.float32))


def _check_buffers(n, ref, B, A, tag=""):
    """Every debug buffer of the step against the oracle's `out`."""
    _close(n.critic_loss.item(), ref["critic_loss"], name=f"critic_loss{tag}")
    _close(n.policy_loss.item(), ref["policy_loss"], name=f"policy_loss{tag}")
    _close(n.debug_buffer("p_a")[:B * A], ref["dpg_a"], name=f"p_a{tag}")
    _close(n.debug_buffer("t_a")[:B * A], ref["a_target"], name=f"t_a{tag}")
    _close(n.debug_buffer("c_q")[:2 * B], np.concatenate([ref["q_tm1"], ref["dpg_q"]]),
           name=f"c_q{tag}")
    _close(n.debug_buffer("t_q")[:B], ref["q_t"], name=f"t_q{tag}")
    _close(n.debug_buffer("td")[:B], ref["td"], name=f"td{tag}")
    dq = n.debug_buffer("dq")[:2 * B]
    _close(dq, ref["dq"], name=f"dq{tag}")
    np.testing.assert_array_equal(dq[B:], np.ones(B, np.float32))  # exactly 1
    _close(n.debug_buffer("dqda")[:B * A], ref["dqda"], name=f"dqda{tag}")
    _close(n.debug_buffer("norms"), ref["norms"], name=f"norms{tag}")


def _run_steps(cfg, max_batch, B, steps, pseed, bseed, learner=None):
    """`steps` teacher-forced steps against the oracle: after each one the oracle continues
    from the kernel's parameters and moments, so fp32 drift cannot compound.  B: the rows of
    every step, or a sequence with the rows of each (a learner created once for max_batch,
    stepped at whatever arrives).  learner: an already created learner to step instead (it
    starts over: these parameters, zero moments, step 0)."""
    n = learner if learner is not None else _native(cfg, max_batch)
    params, target = _random_params(cfg, pseed), _random_params(cfg, pseed + 1)
    n.set_params(params, target)
    if learner is not None:
        n.m.zero_()
        n.v.zero_()
        n.num_steps = 0
    sizes = [B] * steps if np.isscalar(B) else list(B)
    assert len(sizes) == steps
    z = {k: np.zeros_like(v) for k, v in params.items()}
    state = dict(params=params, target=target, m=z, v=dict(z), num_steps=0)
    for s, B in enumerate(sizes):
        batch = _batch(cfg, B, bseed + s)
        n.step(*_dev(batch))
        torch.cuda.synchronize()
        ref, raw, state = O.ddpg_step(cfg, state, batch, np.float64)
        _check_buffers(n, ref, B, cfg.act_dim, tag=f"@{s}")
        _check_grads(n, raw)
        got = n.get_params("params")
        _check_params(got, state["params"], cfg.policy_lr)
        state["params"] = {k: got[k].astype(np.float32) for k in got}
        state["m"] = n.get_params("m")
        state["v"] = n.get_params("v")
        tgt = n.get_params("target")
        for k, r in state["target"].items():
            np.testing.assert_array_equal(tgt[k], np.asarray(r, np.float32), err_msg=k)
        state["target"] = tgt
    assert n.num_steps == steps
    return n


def test_tensor_layout_matches_oracle():
    cfg = O.DDPGConfig()
    n = _native(cfg, 8)
    assert [(k, s) for k, _, s in n.tensors] == O.ddpg_tensor_shapes(cfg)
    assert n.policy_size == [o for k, o, _ in n.tensors if k.startswith("critic/")][0]
    assert n.tensors[-2][0] == "critic/layer_norm_mlp/mlp/linear_2/w"
    assert n.tensors[-2][2] == (256, 1) and n.tensors[-1][2] == (1,)


def test_golden_step():
    from tests.golden.make_ddpg_golden import golden_cfg, unpack
    z = np.load(GOLDEN)
    cfg = golden_cfg()
    params, target, batch = unpack(cfg, z)
    B = len(batch["r_t"])
    n = _native(cfg, B)
    n.set_params(params, target)
    n.num_steps = 1  # no start-of-step target copy; Adam t = 2
    n.step(*_dev(batch))
    torch.cuda.synchronize()
    ref = {k[len("out/"):]: z[k] for k in z.files if k.startswith("out/")}
    _check_buffers(n, ref, B, cfg.act_dim)
    _check_grads(n, {k[len("grad/"):]: v for k, v in ref.items() if k.startswith("grad/")})
    _check_params(n.get_params("params"),
                  {k[len("new/"):]: v for k, v in ref.items() if k.startswith("new/")},
                  cfg.policy_lr)


@pytest.mark.parametrize("B", [5, 37, 256])
def test_steps_match_oracle(B):
    """Full-size networks (policy 256x3, critic 512/512/256/1): three steps with a target
    period of 2, so steps 0 and 2 copy online -> target at the start.  B = 5: less than one
    32-row tile, a ragged last four-row block, dpg rows starting mid-block; B = 37: ragged
    against both 4 and 32."""
    _run_steps(O.DDPGConfig(target_update_period=2), 256, B, 3, 1, 10)


@pytest.mark.parametrize("B", [45, 600])
def test_odd_shapes_match_oracle(B):
    """Widths that are not multiples of the 32-wide tiles, 3 actions, 7 observations, a
    ragged batch and one past 512 rows (two k passes in the weight gradients).  The critic's
    last hidden width is first 44 (less than a wave of float4 groups in the head kernel), then
    1024 (four groups per lane, the widest); two steps each."""
    for critic in ((1024, 132, 44), (64, 1024)):
        cfg = O.DDPGConfig(obs_dim=7, act_dim=3, policy_sizes=(36, 100), critic_sizes=critic,
                           action_min=(-1.0,) * 3, action_max=(1.0,) * 3,
                           target_update_period=2)
        _run_steps(cfg, B, B, 2, 7, 20)


def test_single_action():
    """Pendulum-shaped specs (3 observations, 1 action in [-2, 2]): with the scalar head the
    policy head, the critic head and the action slice of the first layer are all 1 wide."""
    cfg = O.DDPGConfig(obs_dim=3, act_dim=1, policy_sizes=(32, 32), critic_sizes=(64, 32),
                       action_min=(-2.0,), action_max=(2.0,), target_update_period=2)
    _run_steps(cfg, 9, 9, 2, 3, 30)


def _steep_params(cfg, seed):
    """Random parameters with the action rows of the critic's first layer and its head
    scaled up, so dq/da is large (the LayerNorm undoes most of a first-layer scale alone)."""
    p = _random_params(cfg, seed)
    w1 = p["critic/layer_norm_mlp/linear/w"].copy()
    w1[cfg.obs_dim:] *= 2.0
    p["critic/layer_norm_mlp/linear/w"] = w1
    head = f"critic/layer_norm_mlp/mlp/linear_{len(cfg.critic_sizes) - 1}/w"
    p[head] = p[head] * 4.0
    return p


def test_no_clipping_path():
    """clipping=False: neither the dqda clip nor the global-norm clip; the same inputs with
    clipping=True clip the rows whose |dqda| exceeds 1."""
    base = dict(policy_sizes=(64, 64), critic_sizes=(128, 64), target_update_period=100)
    B = 32
    cfg = O.DDPGConfig(clipping=False, **base)
    params, target = _steep_params(cfg, 5), _random_params(cfg, 6)
    batch = _batch(cfg, B, 3)
    z = {k: np.zeros_like(v) for k, v in params.items()}
    refs = {}
    for clipping in (False, True):
        cfg = O.DDPGConfig(clipping=clipping, **base)
        n = _native(cfg, B)
        n.set_params(params, target)
        n.num_steps = 1
        n.step(*_dev(batch))
        torch.cuda.synchronize()
        ref, raw, st = O.ddpg_step(cfg, dict(params=params, target=target, m=z, v=dict(z),
                                             num_steps=1), batch, np.float64)
        refs[clipping] = ref
        _check_buffers(n, ref, B, cfg.act_dim, tag=f"[clipping={clipping}]")
        _check_grads(n, raw)
        _check_params(n.get_params("params"), st["params"], cfg.policy_lr)
        got = np.linalg.norm(n.debug_buffer("dqda")[:B * 6].reshape(B, 6), axis=1)
        big = np.linalg.norm(refs[False]["dqda"], axis=1) > 1.0
        if clipping:
            assert (got <= 1.0 + 1e-5).all()
            np.testing.assert_allclose(got[big], 1.0, rtol=1e-5)
        else:
            # The case shows something only if the clip would have bitten.
            assert big.mean() >= 0.25, big.mean()
            assert (got[big] > 1.0).all()
    assert refs[False]["policy_loss"] > refs[True]["policy_loss"]


def test_graph_replay_matches_eager():
    """The captured step graph (default) and the eager launch sequence (forced by the
    section profiler) produce bit-identical parameters, including across the target copy
    and with the two alternating batch buffers the dataset iterator uses."""
    from acme_amd import _lib
    cfg = O.DDPGConfig(target_update_period=2, policy_sizes=(64, 64, 64),
                       critic_sizes=(128, 128, 64))
    params, target = _random_params(cfg, 11), _random_params(cfg, 12)
    batches = [_dev(_batch(cfg, 64, 20 + i)) for i in range(2)]
    results = []
    for eager in (True, False):
        n = _native(cfg, 64)
        n.set_params(params, target)
        _lib.lib().acme_profile_enable(1 if eager else 0)
        try:
            for s in range(5):
                n.step(*batches[s % 2])
        finally:
            _lib.lib().acme_profile_enable(0)
        torch.cuda.synchronize()
        results.append((n.get_params("params"), n.get_params("target"),
                        n.critic_loss.item(), n.policy_loss.item()))
    (p0, t0, c0, l0), (p1, t1, c1, l1) = results
    for k in p0:
        np.testing.assert_array_equal(p0[k], p1[k], err_msg=k)
        np.testing.assert_array_equal(t0[k], t1[k], err_msg=k)
    assert c0 == c1 and l0 == l1


def test_d4pg_unchanged_beside_ddpg():
    """A D4PG learner stepping in turn with a DDPG learner in one process gives the bits it
    gives alone: the two share the native object and its graph cache code, not state."""
    from acme_amd.native import NativeD4PG
    from oracle import d4pg_oracle as O4
    sizes = dict(policy_sizes=(64, 64), critic_sizes=(128, 64))
    c4 = O4.D4PGConfig(target_update_period=2, **sizes)
    cd = O.DDPGConfig(target_update_period=2, **sizes)
    rng = np.random.default_rng(0)
    p4 = {}
    for name, shape in O4.d4pg_tensor_shapes(c4):
        v = 1.0 + 0.1 * rng.standard_normal(shape) if name.endswith("/scale") else \
            rng.standard_normal(shape) / np.sqrt(shape[0])
        p4[name] = v.astype(np.float32)
    pd = _random_params(cd, 1)
    batches = [_dev(_batch(cd, 32, 40 + i)) for i in range(3)]

    def d4pg():
        n = NativeD4PG(obs_dim=24, act_dim=6, max_batch=32, target_update_period=2, **sizes)
        n.set_params(p4, p4)
        return n

    alone = d4pg()
    for b in batches:
        alone.step(*b)
    torch.cuda.synchronize()
    beside, ddpg = d4pg(), _native(cd, 32)
    ddpg.set_params(pd, pd)
    for b in batches:
        ddpg.step(*b)
        beside.step(*b)
    ddpg.step(*batches[0])
    torch.cuda.synchronize()
    assert beside.num_steps == 3 and ddpg.num_steps == 4
    for which in ("params", "target", "m", "v"):
        a, b = alone.get_params(which), beside.get_params(which)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{which}/{k}")
    assert alone.critic_loss.item() == beside.critic_loss.item()
    assert alone.policy_loss.item() == beside.policy_loss.item()
    assert np.isfinite(ddpg.critic_loss.item())


def test_learner_dropin_path():
    """DDPGLearner through the uniform GPU replay Table + make_reverb_dataset, the
    reference's get_variables contract, and a save -> restore round trip."""
    from acme_amd import replay, specs
    from acme_amd.adders import reverb as adders
    from acme_amd.agents.ddpg import DDPGLearner
    from acme_amd.datasets import make_reverb_dataset
    from acme_amd.networks import make_ddpg_networks
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
    nets = make_ddpg_networks(24, env_spec.actions)

    def make(seed):
        return DDPGLearner(nets["policy"], nets["critic"], nets["policy"], nets["critic"],
                           discount=0.99, target_update_period=100,
                           dataset=make_reverb_dataset(server, batch_size=256),
                           logger=loggers.NoOpLogger(), seed=seed)

    learner = make(0)
    for _ in range(3):
        learner.step()
    torch.cuda.synchronize()
    assert learner.num_steps == 3
    assert np.isfinite(learner.native.critic_loss.item())
    assert np.isfinite(learner.native.policy_loss.item())
    crit, pol = learner.get_variables(["critic", "policy"])
    assert all(k.startswith("critic/") for k in crit) and len(crit) == 10
    assert all(k.startswith("policy/") for k in pol) and len(pol) == 10
    assert crit["critic/layer_norm_mlp/mlp/linear_2/w"].shape == (256, 1)
    assert crit["critic/layer_norm_mlp/mlp/linear_2/b"].shape == (1,)
    assert "policy/near_zero_initialized_linear/w" in pol
    tgt = learner.native.get_params("target")  # the exposed variables are the TARGET networks
    np.testing.assert_array_equal(crit["critic/layer_norm_mlp/linear/w"],
                                  tgt["critic/layer_norm_mlp/linear/w"])
    a = learner.policy(np.zeros((2, 24), np.float32))
    assert a.shape == (2, 6) and np.isfinite(a).all()
    assert (a >= -1.0).all() and (a <= 1.0).all()
    # save -> a new learner (other initial weights) -> restore; one more step on the same
    # batch gives the same bits in both.
    other = make(5)
    other.restore(learner.save())
    assert other.num_steps == 3
    rng = np.random.default_rng(1)
    batch = _dev(dict(o_tm1=rng.standard_normal((256, 24)).astype(np.float32),
                      a_tm1=rng.uniform(-1, 1, (256, 6)).astype(np.float32),
                      r_t=rng.uniform(0, 5, 256).astype(np.float32),
                      d_t=np.full(256, 0.99 ** 4, np.float32),
                      o_t=rng.standard_normal((256, 24)).astype(np.float32)))
    learner.native.step(*batch)
    other.native.step(*batch)
    torch.cuda.synchronize()
    for which in ("params", "target", "m", "v"):
        x, y = learner.native.get_params(which), other.native.get_params(which)
        for k in x:
            np.testing.assert_array_equal(x[k], y[k], err_msg=f"{which}/{k}")


def test_agent_runs_in_environment_loop():
    """The reference's agent test (acme/agents/tf/ddpg/agent_test.py:57-78), run-only: tiny
    networks on a fake continuous environment, two episodes; learner steps happen."""
    from acme_amd import specs
    from acme_amd.agents.ddpg import DDPG
    from acme_amd.environment_loop import EnvironmentLoop
    from acme_amd.networks import make_ddpg_networks
    from acme_amd.testing import fakes
    from acme_amd.utils import loggers
    env = fakes.ContinuousEnvironment(episode_length=10, bounded=True)
    spec = specs.make_environment_spec(env)
    nets = make_ddpg_networks(24, spec.actions, (12, 12), (12, 12))
    agent = DDPG(spec, nets["policy"], nets["critic"], batch_size=10, samples_per_insert=2,
                 min_replay_size=10, logger=loggers.NoOpLogger())
    loop = EnvironmentLoop(env, agent, logger=loggers.NoOpLogger())
    loop.run(num_episodes=2)
    learner = agent._learner  # noqa: SLF001
    torch.cuda.synchronize()
    assert learner.num_steps >= 1
    assert np.isfinite(learner.native.critic_loss.item())
    assert np.isfinite(learner.native.policy_loss.item())
