"""The acting paths against the float64 oracles: acme_dqn_q_values (NativeDQN.q_values,
DQNLearner.q_values, the DQN agent's epsilon-greedy policy) and acme_impala_policy_step served
from the learner's own workspace between learner steps.

q_values is not a thin wrapper.  On the plane path it runs the online parameters through the
target network's activation planes and scale records (kScT1..kScT3), uses the step's shared
slab and frame buffers, calibrates in two passes while the learner has no scales yet, ends
with its own rescale (which moves the records the next step's target forward reads) and
reports an overflow through the guard's qv word, which DQNLearner.q_values answers with a
second call.  It also runs the unfused conv kernels at batch sizes the step never gives
them: one frame (conv2_fwd's two-frame block half empty), 3 and 5 (its last block partial),
37 (a partial 128-row fc tile), always below and at max_batch.

Bars.  q against oracle.dqn_oracle.forward (float64) on the parameters the GPU holds:
tests/test_dqn_gpu.py's bar for q_tm1, rtol 1e-5 and atol 1e-6 (Q_BAR; the same kernels, K
and operands).  Learner steps beside the acting calls: tests/test_step_guard_gpu.py's
_teacher_forced (loss and TD at 1e-5, the suite's gradient bar) from the GPU's own pre-step
state.  IMPALA policy answers: tests/test_impala_gpu.py's _close defaults (rtol 1e-5 + 2e-6 of
the tensor's scale) against oracle.impala_oracle.forward, learner steps its _compare.
Engines without scale state (the MLP, Nature on the exact-f32 engine, IMPALA with
policy_planes off) must not notice the acting calls at all: twin learners, one serving and
one not, stay bit-identical.  On the DQN plane engine q_values legitimately moves the
target records' scales, so there each step of the serving twin is checked against the oracle
instead (a plane-path step is not bitwise equal after a scale move).
"""

import contextlib

import numpy as np
import pytest
import torch

from oracle import dqn_oracle as O
from oracle import impala_oracle as IO
from tests import limit_cases as C
from tests import test_dqn_gpu as dqn_t
from tests import test_impala_gpu as impala_t
from tests import test_step_guard_gpu as guard_t

pytestmark = pytest.mark.gpu

Q_BAR = dict(rtol=1e-5, atol=1e-6)  # tests/test_dqn_gpu.py, q_tm1

# dqn.hip's scale-record enum: kScX1 0, kScX2 1, kScX3 2, kScT1 3, kScT2 4, kScT3 5, kScDzh 6,
# kScDz3 7, kScDz2 8, kScDz1 9, kScTransient = kScParams 10, kScTarget 11, kScCount 12.  A
# record is (w, r, wi, rl) in scale_state().
T_RECORDS = (3, 4, 5)  # kScT1, kScT2, kScT3
SC_COUNT = 12          # kScCount


@contextlib.contextmanager
def _f32_engine():
    """The exact-f32 matmul engine for learners created and used inside."""
    from acme_amd import _lib
    _lib.lib().acme_set_matmul_engine(_lib.MATMUL_F32)
    try:
        yield
    finally:
        _lib.lib().acme_set_matmul_engine(_lib.MATMUL_X6)


def _nature(obs_dtype="uint8"):
    from acme_amd.networks import DQNAtariNetwork
    return DQNAtariNetwork(18, obs_dtype=obs_dtype)


def _frames(rng, n, net):
    if net.obs_dtype == "uint8":
        return rng.integers(0, 256, (n,) + net.obs_shape, dtype=np.uint8)
    return rng.standard_normal((n,) + net.obs_shape).astype(np.float32)


def _ask(d, obs, use_target):
    x = torch.as_tensor(obs).cuda().reshape(obs.shape[0], -1).contiguous()
    q = d.q_values(x, use_target=use_target)
    torch.cuda.synchronize()
    return q.cpu().numpy()


def _ref(net, params, obs):
    return O.forward(dqn_t._cfg(net), params, obs, np.float64)[0]


def _quiet(d):
    """The plane path's side of an answer: no overflow reported, none recorded."""
    assert d.guard_state()["q_values_overflowed"] == 0
    assert not d.plane_overflow()


def _check_q(d, net, obs, use_target, plane, ref=None, bar=Q_BAR, what=""):
    """One q_values answer against the oracle on the parameters the GPU holds now."""
    if ref is None:
        ref = _ref(net, d.get_params("target" if use_target else "params"), obs)
    q = _ask(d, obs, use_target)
    print(f"{what} n={obs.shape[0]} target={int(use_target)} max |q - ref| "
          f"{np.abs(q - ref).max():.3e} max |ref| {np.abs(ref).max():.3e}")
    np.testing.assert_allclose(q, ref, err_msg=what, **bar)
    if plane:
        _quiet(d)
    return ref


def _check_both(d, net, obs, plane, calls=1, what=""):
    """Online and target answers, interleaved `calls` times (on the plane path each call
    moves the scales the next one reads): every one must match."""
    refs = {}
    for call in range(calls):
        for use_target in (False, True):
            refs[use_target] = _check_q(d, net, obs, use_target, plane, refs.get(use_target),
                                        what=f"{what} call {call}")


def _step_batch(rng, net, B):
    return dqn_t._batch(rng, B, net.obs_shape, net.num_actions, u8=net.obs_dtype == "uint8")


def _dev(net, batch):
    dev = dqn_t._dev(batch)
    B = dev[1].shape[0]
    return [x.reshape(B, -1).contiguous() if x.dim() > 1 else x for x in dev]


def _differ(a, b):
    return any(not np.array_equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------ A. q_values = f64 forward


@pytest.mark.parametrize("n,B", [(1, 4), (3, 4), (4, 4), (37, 37)])
def test_q_values_on_fresh_plane_learner(n, B):
    """No step yet: every call calibrates in two passes (scales_ok is false until a step).
    Online and target parameters are distinct draws with non-zero biases; two rounds."""
    net = _nature()
    d = dqn_t._learner(net, B)
    d.set_params(C.dqn_params(net, 1), C.dqn_params(net, 2))
    _check_both(d, net, _frames(np.random.default_rng(n), n, net), plane=True, calls=2)


@pytest.mark.parametrize("n", [1, 5])
def test_q_values_after_steps_and_a_target_copy(n):
    """Two steps at B = 8 with target_update_period 2: the copy of step 0 has landed, step 1
    moved the online parameters on, and the planes are Adam's, not a fresh split."""
    net = _nature()
    B = 8
    t0 = C.dqn_params(net, 2)
    d = dqn_t._learner(net, B, target_update_period=2)
    d.set_params(C.dqn_params(net, 1), t0)
    rng = np.random.default_rng(40 + n)
    for _ in range(2):
        d.step(*_dev(net, _step_batch(rng, net, B)))
    torch.cuda.synchronize()
    prm, tgt = d.get_params("params"), d.get_params("target")
    assert _differ(tgt, t0) and _differ(tgt, prm)
    g = d.guard_state()
    assert g["applied"] == 2 and g["skipped"] == 0, g
    _check_both(d, net, _frames(rng, n, net), plane=True, calls=2)


@pytest.mark.parametrize("stepped", [False, True])
def test_q_values_after_new_parameters(stepped):
    """set_params with a second, different draw on a learner that has already answered a
    call (and, stepped, taken a step: scales_ok was true): stale planes, scales_ok reset."""
    net = _nature()
    B = 4
    d = dqn_t._learner(net, B)
    d.set_params(C.dqn_params(net, 1), C.dqn_params(net, 2))
    rng = np.random.default_rng(7)
    if stepped:
        d.step(*_dev(net, _step_batch(rng, net, B)))
    obs = _frames(rng, 3, net)
    _check_both(d, net, obs, plane=True, what="first draw")
    p2, t2 = C.dqn_params(net, 3), C.dqn_params(net, 4)
    d.set_params(p2, t2)
    _check_both(d, net, obs, plane=True, calls=2, what="second draw")


@pytest.mark.parametrize("stepped", [False, True])
@pytest.mark.parametrize("n", [1, 3])
def test_q_values_on_f32_engine(n, stepped):
    net = _nature()
    B = 4
    with _f32_engine():
        d = dqn_t._learner(net, B)
        d.set_params(C.dqn_params(net, 1), C.dqn_params(net, 2))
        rng = np.random.default_rng(50 + n)
        if stepped:
            d.step(*_dev(net, _step_batch(rng, net, B)))
        _check_both(d, net, _frames(rng, n, net), plane=False, calls=2)


def test_q_values_on_float32_observations():
    net = _nature("float32")
    d = dqn_t._learner(net, 4)
    d.set_params(C.dqn_params(net, 1), C.dqn_params(net, 2))
    _check_both(d, net, _frames(np.random.default_rng(3), 3, net), plane=False, calls=2)


@pytest.mark.parametrize("stepped", [False, True])
@pytest.mark.parametrize("n", [1, 32])
@pytest.mark.parametrize("netname", ["mlp_vec", "cartpole_mlp"])
def test_q_values_on_mlp(netname, n, stepped):
    """The MLP branch writes the target network's activation buffers (mlp_tact)."""
    net = dqn_t.NETS[netname]()
    B = 32
    d = dqn_t._learner(net, B)
    d.set_params(C.dqn_params(net, 1), C.dqn_params(net, 2))
    rng = np.random.default_rng(n)
    if stepped:
        d.step(*_dev(net, _step_batch(rng, net, B)))
    _check_both(d, net, _frames(rng, n, net), plane=False, calls=2)


@pytest.mark.parametrize("netname", ["nature", "mlp_vec"])
def test_q_values_rejects_batches_outside_the_learner(netname):
    net = dqn_t.NETS[netname]()
    B = 4
    d = dqn_t._learner(net, B)
    d.set_params(C.dqn_params(net, 1), C.dqn_params(net, 2))
    rng = np.random.default_rng(0)
    for n in (0, B + 1):
        x = torch.as_tensor(_frames(rng, max(n, 1), net)).cuda().reshape(max(n, 1), -1)
        with pytest.raises(ValueError):
            d.q_values(x[:n])
    _check_both(d, net, _frames(rng, B, net), plane=netname == "nature")


# ------------------------------------------------------------------ B. edge inputs


def _t_records(d):
    """(w, r, wi) of the T records (rl follows r at every rescale: not a scale of its own)."""
    s = d.scale_state()
    assert s.size == 4 * SC_COUNT
    return s.reshape(SC_COUNT, 4)[list(T_RECORDS), :3].copy()


@pytest.mark.parametrize("stepped", [False, True])
def test_black_frames_with_zero_biases(stepped):
    """Every torso activation is zero (tests/test_acting_cpu.py), so the T records see a
    maximum of 0 and must keep their scale (the initial one, or with `stepped` the one a
    step's target forward left; that step at learning rate 0, so the biases stay zero); q is
    the head's biases, here 0, so atol 1e-6 alone.  A call on random frames afterwards meets
    Q_BAR."""
    net, p, t, black = C.dqn_acting_edge("black_zero_bias")
    d = dqn_t._learner(net, 4, learning_rate=0.0, target_update_period=100)
    d.set_params(p, t)
    rng = np.random.default_rng(5)
    if stepped:
        d.step(*_dev(net, _step_batch(rng, net, 4)))
        torch.cuda.synchronize()
    before = _t_records(d)
    assert (before != 1.0).any() == stepped  # calibrated scales only after a step
    for use_target in (False, True):
        q = _ask(d, black, use_target)
        np.testing.assert_allclose(q, np.zeros_like(q), rtol=0, atol=1e-6)
        _quiet(d)
    np.testing.assert_array_equal(_t_records(d), before)
    _check_both(d, net, _frames(rng, 3, net), plane=True)


@pytest.mark.parametrize("name", ["black_biased", "saturated"])
def test_constant_frames(name):
    """Black frames under non-zero biases (activations constant per channel away from the
    padding) and one saturated frame (the largest input a uint8 actor can send)."""
    net, p, t, frames = C.dqn_acting_edge(name)
    d = dqn_t._learner(net, 4)
    d.set_params(p, t)
    _check_both(d, net, frames, plane=True, calls=2)
    _check_both(d, net, _frames(np.random.default_rng(6), 3, net), plane=True)


# ------------------------------------------------------------------ C. the overflow answer


def _force_t_overflow(d):
    """The T records' write scale 2^12 too large (and the read scales to match): the next
    forward through them overflows f16 at 2^7..2^8 x 2^12, the arithmetic overflow the guard
    is built for (tests/test_step_guard_gpu.py::test_overflow_skips_step_and_recovers)."""
    s = d.scale_state()
    assert s.size == 4 * SC_COUNT
    s = s.reshape(SC_COUNT, 4).copy()
    for i in T_RECORDS:
        s[i, 0] *= np.float32(2.0 ** 12)
        s[i, 1:] /= np.float32(2.0 ** 12)
    assert (np.frexp(s)[0] == 0.5).all()  # every entry a power of two
    d.set_scale_state(s.reshape(-1))


def _checked_step(d, net, b):
    """One step, applied, at tests/test_dqn_gpu.py's bars against the oracle teacher-forced
    from the GPU's own pre-step state."""
    B = b["a_tm1"].shape[0]
    pre = d.get_params("params"), d.get_params("target")
    before = d.guard_state()
    q = torch.empty(B, net.num_actions, device="cuda")
    d.step(*_dev(net, b), q_tm1=q)
    torch.cuda.synchronize()
    _after_step(d, net, b, pre, before, q)


def _after_step(d, net, b, pre, before, q=None):
    B = b["a_tm1"].shape[0]
    g = d.guard_state()
    assert g["skipped"] == before["skipped"] and g["applied"] == before["applied"] + 1, g
    guard_t._teacher_forced(d, pre[0], pre[1], b, B)
    if q is not None:
        np.testing.assert_allclose(q.cpu().numpy(), _ref(net, pre[0], b["o_tm1"]), **Q_BAR)


def test_native_q_values_reports_overflow_and_recovers():
    net = _nature()
    B = 8
    d = dqn_t._learner(net, B)
    d.set_params(C.dqn_params(net, 1), C.dqn_params(net, 2))
    rng = np.random.default_rng(9)
    d.step(*_dev(net, _step_batch(rng, net, B)))
    torch.cuda.synchronize()
    assert d.guard_state()["applied"] == 1
    obs = _frames(rng, 3, net)
    for use_target in (False, True):
        _force_t_overflow(d)
        _ask(d, obs, use_target)
        assert d.guard_state()["q_values_overflowed"] == 1
        assert d.plane_overflow(reset=True)
        # The identical call again, at the scales the first call's rescale chose.
        _check_q(d, net, obs, use_target, plane=True, what="second call")
    _checked_step(d, net, guard_t._batch(rng, B, 18))


def test_learner_q_values_retries_an_overflowed_call():
    """DQNLearner.q_values answers the qv word with a second call: oracle-accurate values in
    one call of the learner's, and the step that follows is applied and accurate.  Built as
    tests/test_step_guard_gpu.py::test_learner_reissues_skipped_step."""
    from acme_amd import replay, specs
    from acme_amd.adders import reverb as adders
    from acme_amd.agents.dqn import DQNLearner
    from acme_amd.utils import loggers
    B, A = 8, 18
    net = _nature()
    rng = np.random.default_rng(10)
    batches = [guard_t._batch(rng, B, A), guard_t._batch(rng, B, A)]
    spec = specs.EnvironmentSpec(
        observations=specs.Array((84, 84, 4), np.uint8), actions=specs.DiscreteArray(A, np.int32),
        rewards=specs.Array((), np.float32), discounts=specs.BoundedArray((), np.float32, 0, 1))
    table = replay.Table(adders.DEFAULT_PRIORITY_TABLE, replay.selectors.Prioritized(0.6),
                         replay.selectors.Fifo(), 1000, replay.rate_limiters.MinSize(1),
                         signature=adders.NStepTransitionAdder.signature(spec), seed=3)
    table.native.fill_synthetic(1000, layout=0, num_actions=A, seed=0)
    ds = guard_t._FixedBatches([guard_t._sample(b, B * i) for i, b in enumerate(batches)])
    lr = DQNLearner(net, net, discount=0.99, importance_sampling_exponent=0.2,
                    learning_rate=1e-3, target_update_period=2, dataset=ds,
                    replay_client=replay.Client(replay.Server([table])),
                    logger=loggers.NoOpLogger(), seed=0)
    d = lr.native
    d.set_params(C.dqn_params(net, 1), C.dqn_params(net, 2))
    lr.step()
    torch.cuda.synchronize()
    obs = _frames(rng, 3, net)
    for use_target in (False, True):
        ref = _ref(net, d.get_params("target" if use_target else "params"), obs)
        _force_t_overflow(d)
        q = lr.q_values(obs, use_target=use_target)
        assert d.plane_overflow(reset=True), "the first native call must have overflowed"
        np.testing.assert_allclose(q, ref, **Q_BAR)
        assert d.guard_state()["q_values_overflowed"] == 0
    pre = d.get_params("params"), d.get_params("target")
    before = d.guard_state()
    lr.step()
    lr.save()  # settles: a skipped step would have been re-issued
    torch.cuda.synchronize()
    assert lr._reissued == 0  # noqa: SLF001
    _after_step(d, net, batches[1], pre, before)


# ------------------------------------------------------------------ D. acting between steps


def _serve(d, net, rng, plane, what):
    """What an agent asks between steps: one frame of the online network, three of the
    target's, each against the oracle on the parameters of that moment."""
    _check_q(d, net, _frames(rng, 1, net), False, plane, what=what)
    _check_q(d, net, _frames(rng, 3, net), True, plane, what=what)


def _state(d):
    out = {buf: d.get_params(buf) for buf in ("params", "target", "m", "v")}
    out["out"] = dict(loss=d.loss.cpu().numpy(), td=d.td_error.cpu().numpy(),
                      prio=d.priorities.cpu().numpy())
    return out


def _twin_step(d, dev, schedule, between=None):
    if schedule == "fused":
        d.step(*dev)
    else:
        d.forward_backward(*dev)
        if between:
            between()
        d.apply()
    torch.cuda.synchronize()


@pytest.mark.parametrize("schedule", ["fused", "staged"])
@pytest.mark.parametrize("kind", ["mlp", "nature_f32"])
def test_acting_leaves_engines_without_scales_bit_identical(kind, schedule):
    """Twin learners, three steps with a target copy between them (period 2).  Twin A serves
    q_values before the first step, after each step and (staged) between forward_backward
    and apply; twin B serves none.  Neither engine has scale state, so loss, TD errors,
    priorities, params, target, m and v are bit-identical after every step."""
    net = dqn_t.NETS["mlp_vec"]() if kind == "mlp" else _nature()
    B = 5
    with (_f32_engine() if kind == "nature_f32" else contextlib.nullcontext()):
        p0, t0 = C.dqn_params(net, 1), C.dqn_params(net, 2)
        a = dqn_t._learner(net, B, target_update_period=2)
        b = dqn_t._learner(net, B, target_update_period=2)
        a.set_params(p0, t0)
        b.set_params(p0, t0)
        rng, arng = np.random.default_rng(12), np.random.default_rng(13)
        _serve(a, net, arng, False, "before step 0")
        for step in range(3):
            dev = _dev(net, _step_batch(rng, net, B))
            _twin_step(a, dev, schedule,
                       lambda: _serve(a, net, arng, False, f"inside step {step}"))
            _twin_step(b, dev, schedule)
            sa, sb = _state(a), _state(b)
            for buf in sa:
                for k in sa[buf]:
                    np.testing.assert_array_equal(sa[buf][k], sb[buf][k],
                                                  err_msg=f"step {step} {buf}/{k}")
            _serve(a, net, arng, False, f"after step {step}")
        assert a.num_steps == b.num_steps == 3
        assert _differ(a.get_params("target"), t0)


@pytest.mark.parametrize("schedule", ["fused", "staged"])
def test_acting_between_plane_steps(schedule):
    """As above on the plane engine, where q_values legitimately moves the T records' scales
    (so the twins need not agree bit for bit: a plane-path step is not bitwise equal after a
    scale move).  Every step of the serving twin meets tests/test_dqn_gpu.py's bars against
    the oracle, teacher-forced from its own pre-step state; neither twin skips a step.  On
    the fused schedule step 1 carries inputs_event and obs_f16 (as
    test_early_target_forward_bitwise), so the early target forward comes right after a
    q_values call."""
    from acme_amd._lib import OrderEvent
    net = _nature()
    B = 5
    p0, t0 = C.dqn_params(net, 1), C.dqn_params(net, 2)
    a = dqn_t._learner(net, B, target_update_period=2)
    b = dqn_t._learner(net, B, target_update_period=2)
    a.set_params(p0, t0)
    b.set_params(p0, t0)
    rng, arng = np.random.default_rng(14), np.random.default_rng(15)
    _serve(a, net, arng, True, "before step 0")
    for step in range(3):
        batch = guard_t._batch(rng, B, 18)
        dev = _dev(net, batch)
        pre, before = (a.get_params("params"), a.get_params("target")), a.guard_state()
        if schedule == "fused" and step == 1:
            fb = torch.cat([dev[0], dev[4]]).to(torch.float16).view(torch.int16)
            ev = OrderEvent()
            ev.record()
            a.step(*dev, obs_f16=fb, inputs_event=ev)
            torch.cuda.synchronize()
        else:
            _twin_step(a, dev, schedule,
                       lambda: _serve(a, net, arng, True, f"inside step {step}"))
        _twin_step(b, dev, schedule)
        _after_step(a, net, batch, pre, before)
        _serve(a, net, arng, True, f"after step {step}")
    for d in (a, b):
        g = d.guard_state()
        assert g["skipped"] == 0 and g["applied"] == 3, g
    assert _differ(a.get_params("target"), t0)


def test_q_values_after_a_skipped_step():
    """tests/test_step_guard_gpu.py::test_overflow_skips_step_and_recovers's recipe (head x
    1e-4; a batch with |TD| ~ 1e-4, then one with |TD| ~ 1: the head dZ overflows and the
    step is skipped).  The skipped step's Adam launch rewrote the parameter planes at the
    old write scale and changed no parameter: right after it, q_values of both parameter
    sets meets Q_BAR on the unchanged parameters."""
    net = _nature()
    B = 8
    p0, t0 = guard_t._head_scaled_params(net)
    d = dqn_t._learner(net, B)
    d.set_params(p0, t0)
    rng = np.random.default_rng(3)
    d.step(*_dev(net, guard_t._batch(rng, B, 18, r=0.0, d=0.0)))
    torch.cuda.synchronize()
    state1 = {buf: d.get_params(buf) for buf in ("params", "target")}
    d.step(*_dev(net, guard_t._batch(rng, B, 18, r=1.0, d=0.0)))
    torch.cuda.synchronize()
    g = d.guard_state()
    assert g["applied"] == 1 and g["skipped"] == 1 and g["last_skipped"] == 1, g
    d.plane_overflow(reset=True)  # the skipped step's own
    for n in (1, 3):
        obs = _frames(rng, n, net)
        for use_target in (False, True):
            ref = _ref(net, state1["target" if use_target else "params"], obs)
            _check_q(d, net, obs, use_target, plane=True, ref=ref, what="after the skip")
    for buf, want in state1.items():
        got = d.get_params(buf)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{buf}/{k}")


# ------------------------------------------------------------------ E. IMPALA policy steps


def _policy_ok(cfg, n, rows, seed, what):
    """One policy step of `rows` actors against the f64 forward on the learner's current
    parameters (tests/test_impala_gpu.py::test_policy_step_matches_unroll's bars)."""
    params = n.get_params("params")
    b = impala_t._batch(cfg, rows, 1, seed)
    logits, values, cache = IO.forward(cfg, params, b, np.float64)
    d = lambda x: torch.as_tensor(np.ascontiguousarray(x)).cuda()  # noqa: E731
    lg, v, h, c = n.policy_step(d(b["obs"][:, 0]), d(b["prev_action"][:, 0]),
                                d(b["prev_reward"][:, 0]), d(b["h0"]), d(b["c0"]))
    torch.cuda.synchronize()
    impala_t._close(lg.cpu().numpy(), logits[:, 0], name=f"{what} logits")
    impala_t._close(v.cpu().numpy(), values[:, 0], name=f"{what} values")
    impala_t._close(h.cpu().numpy(), cache["hs"][:, 0], name=f"{what} h")
    impala_t._close(c.cpu().numpy(), cache["cs"][:, 0], name=f"{what} c")


IMPALA_TWINS = {
    "flat": (IO.IMPALAConfig(num_actions=5, torso="flat", obs_dim=12, lstm_size=16, head_size=16,
                             entropy_cost=0.01, baseline_cost=0.5), 4, 6),
    # 64 frames: the learner step takes the plane path, the one-launch LSTM unroll.
    "atari": (IO.IMPALAConfig(num_actions=18, torso="atari", lstm_size=256, head_size=64,
                              entropy_cost=0.01, baseline_cost=0.5), 4, 16),
}


@pytest.mark.parametrize("torso", ["flat", "atari"])
def test_policy_steps_leave_the_impala_learner_bit_identical(torso):
    """The single-process agent serves policy steps from the learner's own workspace (pv, h,
    c, the torso activations) between learner steps.  Twin A answers rows = 1 and rows = 3
    before and between two learner steps, twin B none.  With policy_planes off (the default) a
    policy step does no rescale: metrics, params, m and v are bit-identical after each step,
    and every policy answer meets _close's bars on A's parameters of that moment."""
    cfg, B, T = IMPALA_TWINS[torso]
    params = impala_t._params(cfg, 1)
    a, b = impala_t._native(cfg, B, T), impala_t._native(cfg, B, T)
    a.set_params(params)
    b.set_params(params)
    for step in range(2):
        for rows in (1, 3):
            _policy_ok(cfg, a, rows, 100 + 10 * step + rows, f"before step {step} rows {rows}")
        batch = impala_t._batch(cfg, B, T, 2 + step)
        impala_t._run(a, batch)
        impala_t._run(b, batch)
        np.testing.assert_array_equal(a.metrics.cpu().numpy(), b.metrics.cpu().numpy())
        for buf in ("params", "m", "v"):
            ga, gb = a.get_params(buf), b.get_params(buf)
            for k in ga:
                np.testing.assert_array_equal(ga[k], gb[k], err_msg=f"step {step} {buf}/{k}")
    for n in (a, b):
        g = n.guard_state()
        assert g["applied"] == 2 and g["skipped"] == 0, g
    assert _differ(a.get_params("params"), params)
    _policy_ok(cfg, a, 3, 199, "after the steps")


def test_policy_steps_on_planes_around_a_learner_step():
    """set_policy_planes(True), 64 rows: a policy call rescales every transient record from
    a T = 1 forward, so the backward's records see a maximum of 0 and must keep their scale,
    and the learner step that follows must still find every record it needs calibrated: it
    passes _compare teacher-forced from the GPU's parameters and is not skipped; the policy
    calls on both sides of it meet _close's bars; no plane overflow."""
    cfg, B, T = IMPALA_TWINS["atari"]
    rows = 64
    n = impala_t._native(cfg, rows, T)
    n.set_policy_planes(True)
    n.set_params(impala_t._params(cfg, 7))
    _policy_ok(cfg, n, rows, 30, "before the step")
    params = n.get_params("params")
    batch = impala_t._batch(cfg, B, T, 4)
    impala_t._run(n, batch)
    g = n.guard_state()
    assert n.skipped_steps == 0 and g["skipped"] == 0 and g["applied"] == 1, g
    impala_t._compare(cfg, n, params, batch)
    _policy_ok(cfg, n, rows, 31, "after the step")
    assert not n.plane_overflow()
