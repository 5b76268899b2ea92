"""The plane-engine learner steps on degenerate frames and on scale jumps at the step guard's
window edges (DQN, IMPALA, R2D2 on uint8 Atari frames).

Every GEMM of these steps runs on two scaled f16 planes (csrc/gemm_p3.h) whose per-tensor
scale records lag one step, are calibrated in several passes on a learner's first batch
(dqn.hip calibrate_scales, recurrent_common.h calibrate_then_step), are moved by the
end-of-step rescale (rescale.h) and are watched by the step guard, which skips a step whose
planes overflowed or underflowed.  The contract, checked here on inputs the rest of the
suite never sends (it draws i.i.d. uniform bytes and N(0, 1.5) rewards):

  * an applied step is as accurate as f32;
  * a skipped step changes nothing;
  * a repeated batch gets applied.

No verdict is prescribed for a schedule's steps: _issue_until_applied takes whatever the guard
decides and holds it to the invariant.  A skipped issue: params, target, m, v (and, with a
replay table, its raw priorities) bit-identical, `applied` unchanged, `skipped` one higher;
the same batch is issued again.  An applied issue, teacher-forced from the GPU's own
pre-step state, at existing bars only:
  tests/test_step_guard_gpu.py _teacher_forced: loss and TD at 1e-5, the suite's gradient bar
      (1e-4 |g| + 2e-5 max |g|) on the kernel's own ReLU masks, the activations at 1e-5 + 2e-6
      of their scale.  Where the oracle's tensor is identically zero these bars demand exact
      zeros of the kernels.
  tests/test_dqn_gpu.py: q_tm1 at rtol 1e-5 / atol 1e-6 (Q_BAR).
  tests/test_step_guard_gpu.py test_overflow_skips_step_and_recovers: Adam on the GPU's own
      gradients at rtol 1e-6 / atol 1e-9 with t = the applied count (ADAM_BAR).
  The target: bitwise the new parameters when the copy was due, else unchanged.
At most `cap` skips per batch, a condition and not a measurement: the learner's number of
transient scale records (dqn.hip kScTransient = 10; impala.hip kScTransient = 8;
r2d2_learner.hip rescales kScCount = 9 records as transient).  Each skipped issue ends with
a rescale that leaves at least one more record of the forward and input-gradient chains at
a measured scale, so a chain of that many records is calibrated after as many issues.

Schedules (tests/limit_cases.py DQN_PLANE_SCHEDULES; the Nature network, 18 actions, B = 5:
conv2_fwd's last two-frame block half empty, every row tile partial; shown to produce their
edges on the oracle alone by tests/test_plane_inputs_cpu.py):
  black_first          the calibrating step measures 0 for every activation and every input
                       gradient below the head dZ; the second batch meets records that
                       were never calibrated.  Also with a table.
  black_between        records with a maximum of 0 keep a stale scale across a step
                       (learning rate 0, so the biases stay zero).
  black_after_update   the same batches at the default learning rate: the black batch's
                       activations are the biases the first update left, about 2^-10 of
                       the first batch's, and the third batch's 2^10 above them.
  black_biased         activations constant per channel.
  dark_then_saturated  x1's maximum moves 2^7..2^8-fold up and then down: inside the band
                       where the window's verdict depends on the mantissa.  Also with a table.
  sparse               Atari-like frames: operand units that are entirely zero next to
                       full-range ones.
Skips seen on the MI355X, per batch of the schedule (a record, asserted nowhere; the same
with and without a table):
  black_first [0, 1, 0] (the second batch underflows its never-calibrated records once);
  black_between [0, 0, 0]; black_after_update [0, 1, 1] (an underflow, then an overflow);
  black_biased [0, 0, 0]; dark_then_saturated [0, 0, 0]; sparse [0, 0, 0];
  IMPALA [0, 1, 0]; R2D2 [0, 1, 0]; the window cases' first batch 0 (asserted, see the test).

The window's edges (limit_cases.DQN_WINDOW_JUMPS).  The rescale leaves a tensor's maximum
times its write scale in [2^7, 2^8) (rescale_exp), and the guard applies the next step while
that product is in [1, 65520) (rescale_block).  A g-fold jump must therefore apply when
[2^7 g, 2^8 g) lies inside [1, 65520), i.e. 2^-7 <= g <= 2^7, and must skip when it lies
outside whatever the mantissa: g >= 2^9 (overflow) or g <= 2^-8 (underflow).  Two steps at
learning rate 0 on the same frames, actions and probabilities with constant rewards r0 and
g r0, d = 0, |TD| < 1 (Huber's quadratic zone) and q negligible, so the head dZ and the whole
input-gradient chain (records kScDzh, kScDz3, kScDz2, kScDz1) scale by g and nothing else
moves:
  g = 2^7, g = 2^-6    the second step is applied at once and meets the bars;
  g = 2^10             skipped exactly once with plane_overflow() set, then applied;
  g = 2^-9             skipped exactly once with plane_overflow() clear (the rescale's
                       underflow test alone), then applied.
The first step of each pair, the calibrating one, must be applied at once: every tensor of
its batch is non-zero, and calibrate_scales' passes calibrate every record whatever the
gradients' magnitude (|TD| down to 2^-11 here).

test_first_verdict_skip_writes_no_priority: a learner's first verdict (number 0) that is a
skip.  Found by these tests: the guard's verdict word started at 0, which the priority
write-back read as "verdict 0: applied" without waiting, so a skipped first step wrote its
priorities (plane_guard.h guard_create now starts it at "no verdict").

IMPALA (B = 4, T = 16: 64 frames, the fewest on the plane path) and R2D2 (B = 3, T = 6): the
first, calibrating step on black frames under zero biases, then two of the modules' random
batches; the same invariant with the modules' own _compare / _check_step bars.
"""

import numpy as np
import pytest
import torch

from oracle import dqn_oracle as O
from tests import limit_cases as C
from tests import test_dqn_gpu as dqn_t
from tests import test_impala_gpu as impala_t
from tests import test_r2d2_learner_gpu as r2d2_t
from tests import test_step_guard_gpu as guard_t

pytestmark = pytest.mark.gpu

Q_BAR = dict(rtol=1e-5, atol=1e-6)     # tests/test_dqn_gpu.py, q_tm1
ADAM_BAR = dict(rtol=1e-6, atol=1e-9)  # test_step_guard_gpu.test_overflow_skips_step_and_recovers

DQN_CAP = 10     # dqn.hip kScTransient
IMPALA_CAP = 8   # impala.hip kScTransient (= recurrent_common.h kScRecurrent)
R2D2_CAP = 9     # r2d2_learner.hip kScCount, the records its step's rescale treats as transient

BUFS = ("params", "target", "m", "v")


def _unchanged(n, state, what):
    for buf, ref in state.items():
        got = n.get_params(buf)
        for k in ref:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{what}: {buf}/{k}")


def _counts_after_skip(g, before):
    assert g["applied"] == before["applied"] and g["skipped"] == before["skipped"] + 1, (before, g)


def _counts_after_apply(g, before):
    assert g["applied"] == before["applied"] + 1 and g["skipped"] == before["skipped"], (before, g)


def _issue_until_applied(d, batch, cap, table=None, log=None):
    """Issues `batch` to the NativeDQN d until the guard applies it; -> the number of skipped
    issues (more than cap fails).  Every skipped issue must have changed nothing, the
    applied one must meet the module docstring's bars.  log: a list that receives one
    {"skipped", "overflow"} per issue (plane_overflow() of that issue alone)."""
    B, A = batch["a_tm1"].shape[0], d.num_actions
    dev = guard_t._dev(batch)
    update = {}
    if table is not None:
        update["priority_update"] = (table.handle, table.sample(B, 0)["keys"])
    period, lr = int(d.cfg.target_update_period), float(d.cfg.learning_rate)
    skips = 0
    while True:
        torch.cuda.synchronize()
        before = d.guard_state()
        state = {buf: d.get_params(buf) for buf in BUFS}
        raw = table.export_state()["raw_priorities"].copy() if table is not None else None
        copy_due = d.num_steps % period == 0
        d.plane_overflow(reset=True)
        q = torch.empty(B, A, device="cuda")
        d.step(*dev, q_tm1=q, **update)
        torch.cuda.synchronize()
        g = d.guard_state()
        if log is not None:
            log.append(dict(skipped=bool(g["last_skipped"]), overflow=d.plane_overflow()))
        if not g["last_skipped"]:
            break
        _counts_after_skip(g, before)
        _unchanged(d, state, f"skipped issue {skips}")
        if table is not None:
            np.testing.assert_array_equal(table.export_state()["raw_priorities"], raw)
        skips += 1
        assert skips <= cap, f"{skips} skips of one batch, cap {cap}"
    _counts_after_apply(g, before)
    guard_t._teacher_forced(d, state["params"], state["target"], batch, B)
    cfg = O.DQNConfig(num_actions=A, network="nature")
    q_ref, _ = O.forward(cfg, state["params"], batch["o_tm1"], np.float64)
    np.testing.assert_allclose(q.cpu().numpy(), q_ref, **Q_BAR)
    grads, got = d.get_params("grads"), d.get_params("params")
    for k in got:
        want, _, _ = O.adam_update(state["params"][k], grads[k], state["m"][k], state["v"][k],
                                   g["applied"], lr)
        np.testing.assert_allclose(got[k], want, err_msg=k, **ADAM_BAR)
    for k, v in d.get_params("target").items():
        np.testing.assert_array_equal(v, got[k] if copy_due else state["target"][k], err_msg=k)
    if table is not None:  # an applied step writes the batch's priorities
        assert not np.array_equal(table.export_state()["raw_priorities"], raw)
    return skips


def _table():
    from acme_amd.native import NativeReplay
    table = NativeReplay(1000, [4], prioritized=True, priority_exponent=0.6, seed=5)
    rows = np.arange(600, dtype=np.uint32).view(np.uint8).reshape(600, 4)
    table.insert([rows], np.linspace(0.5, 2.0, 600))
    return table


# ------------------------------------------------------------------ DQN schedules


@pytest.mark.parametrize("name,with_table", [
    ("black_first", False), ("black_first", True), ("black_between", False),
    ("black_after_update", False), ("black_biased", False), ("dark_then_saturated", False), ("dark_then_saturated", True),
    ("sparse", False)])
def test_dqn_schedule(name, with_table):
    net, params, target, batches, lr = C.dqn_plane_schedule(name)
    d = dqn_t._learner(net, C.DQN_PLANE_B, learning_rate=lr)
    d.set_params(params, target)
    table = _table() if with_table else None
    skips, log = [], []
    for b in batches:
        skips.append(_issue_until_applied(d, b, DQN_CAP, table, log))
    print(f"{name} table={int(with_table)}: skips per batch {skips}, issues {log}")
    g = d.guard_state()
    assert g["applied"] == len(batches) and g["skipped"] == sum(skips), g
    assert d.num_steps == len(batches) + sum(skips)


# ------------------------------------------------------------------ the window's edges


@pytest.mark.parametrize("name", sorted(C.DQN_WINDOW_JUMPS))
def test_dqn_guard_window(name):
    net, params, target, first, second, g = C.dqn_window_case(name)
    _, _, _, want_skips, want_overflow = C.DQN_WINDOW_JUMPS[name]
    d = dqn_t._learner(net, C.DQN_PLANE_B, learning_rate=0.0)
    d.set_params(params, target)
    log1, log2 = [], []
    first_skips = _issue_until_applied(d, first, DQN_CAP, log=log1)
    skips = _issue_until_applied(d, second, DQN_CAP, log=log2)
    print(f"{name}: g = {g}, first batch {log1}, second batch {log2}")
    # Every tensor of the first batch is non-zero (tests/test_plane_inputs_cpu.py) with
    # |TD| down to 2^-11: calibrate_scales' passes, one per tensor of the input-gradient
    # chain, leave every record calibrated whatever the gradients' magnitude, so the
    # calibrating step itself is applied.
    assert first_skips == 0, (name, log1)
    assert skips == want_skips, (name, log2)
    if want_skips:
        assert log2[0]["overflow"] == want_overflow, (name, log2)
    assert not log2[-1]["overflow"]


def test_first_verdict_skip_writes_no_priority():
    """A learner's first step with a priority write-back carries verdict number 0.  Its
    scale records restored at 1 (set_scale_state: no calibration, as after a checkpoint taken
    before the first step), that step underflows and is skipped, and the write-back riding
    conv1's weight-gradient launch must wait for that verdict like any later one: the
    guard's verdict word started at 0, which reads as "verdict 0: applied", and the skipped
    step's priorities were written."""
    net, params, target, batch = C.dqn_uncalibrated_case()
    d = dqn_t._learner(net, C.DQN_PLANE_B)
    d.set_params(params, target)
    d.set_scale_state(d.scale_state())
    log = []
    skips = _issue_until_applied(d, batch, DQN_CAP, _table(), log)
    print(f"first verdict: skips {skips}, issues {log}")
    assert log[0]["skipped"], log
    assert d.guard_state()["verdict_timeouts"] == 0


# ------------------------------------------------------------------ IMPALA and R2D2


def test_impala_first_step_on_black_frames():
    cfg, B, T, params, batches = C.impala_plane_black()
    n = impala_t._native(cfg, B, T)
    n.set_params(params)
    seen = []
    for b in batches:
        skips = 0
        while True:
            torch.cuda.synchronize()
            before = n.guard_state()
            state = {buf: n.get_params(buf) for buf in ("params", "m", "v")}
            impala_t._run(n, b)
            g = n.guard_state()
            if not g["last_skipped"]:
                break
            _counts_after_skip(g, before)
            _unchanged(n, state, f"skipped issue {skips}")
            skips += 1
            assert skips <= IMPALA_CAP, f"{skips} skips of one batch, cap {IMPALA_CAP}"
        _counts_after_apply(g, before)
        impala_t._compare(cfg, n, state["params"], b,
                          moments=(state["m"], state["v"], before["applied"]))
        seen.append(skips)
    print(f"impala black first: skips per batch {seen}")
    g = n.guard_state()
    assert g["applied"] == len(batches) and g["skipped"] == sum(seen) and g["lstm_timeouts"] == 0, g


def test_r2d2_first_step_on_black_frames():
    cfg, B, T, params, target, batches = C.r2d2_plane_black()
    n = r2d2_t._native(cfg, B, T)
    n.set_params(params, target)
    seen = []
    for i, b in enumerate(batches):
        skips = 0
        while True:
            torch.cuda.synchronize()
            before = n.guard_state()
            state = {buf: n.get_params(buf) for buf in BUFS}
            copy_due = n.num_steps % cfg.target_update_period == 0
            r2d2_t._run(n, b)
            g = n.guard_state()
            if not g["last_skipped"]:
                break
            _counts_after_skip(g, before)
            _unchanged(n, state, f"skipped issue {skips}")
            skips += 1
            assert skips <= R2D2_CAP, f"{skips} skips of one batch, cap {R2D2_CAP}"
        _counts_after_apply(g, before)
        r2d2_t._check_step(cfg, n, dict(state, num_steps=before["applied"]), b, copy_due, k=i)
        seen.append(skips)
    print(f"r2d2 black first: skips per batch {seen}")
    g = n.guard_state()
    assert g["applied"] == len(batches) and g["skipped"] == sum(seen), g
    assert n.debug_buffer("lstm_timeout").view(np.uint32)[0] == 0
