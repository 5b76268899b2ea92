"""Learner steps below and across the shapes the learner was created for.

Every other learner test creates its learner for the one batch it runs.  Here each learner
is created once at its maxima and stepped through a schedule of shapes
(tests/schedule_cases.py), as data-parallel shares, short last batches and a long-lived
learner see them; the workspaces then keep the rows of earlier, larger steps beyond the
current ones.

(a) test_*_schedule_matches_oracle: every step against the float64 oracle, teacher-forced
(the oracle continues from the kernel's own parameters and moments), by the helpers of the
per-learner modules at the bars their docstrings state: test_dqn_gpu.py, test_impala_gpu.py,
test_r2d2_learner_gpu.py, test_d4pg_gpu.py, test_ddpg_gpu.py, test_mpo_gpu.py and
test_dmpo_gpu.py.  No tolerance is introduced here.  Debug buffers are sized for the maxima;
only the step's rows are read, laid out with that step's B and T.  Every step must be
applied: no skip, no plane overflow, no LSTM spin timeout.

(b) test_*_small_step_is_independent_of_history: the first step smaller than its
predecessor, run on the used learner, again on the used learner restored to the state before
it, and on a fresh learner restored to that state.  All three run identical code on
identical state, so everything the step produces is equal bit for bit; a difference means a
workspace row, granule or scale record left by the larger step was read.

tests/test_batch_schedule_cpu.py shows on the oracles alone that one leaked row would exceed
the bars of (a) a hundredfold.
"""

import numpy as np
import pytest
import torch

from oracle import d4pg_oracle as D4
from oracle import dqn_oracle as DQ
from tests import schedule_cases as S
from tests import test_d4pg_gpu as d4pg_t
from tests import test_ddpg_gpu as ddpg_t
from tests import test_dmpo_gpu as dmpo_t
from tests import test_dqn_gpu as dqn_t
from tests import test_impala_gpu as impala_t
from tests import test_mpo_gpu as mpo_t
from tests import test_r2d2_learner_gpu as r2d2_t
from tests.test_mpo_gpu import _report_all_misses  # noqa: F401  (MPO / DMPO helpers' misses)

pytestmark = pytest.mark.gpu

DQN_PERIOD = 2  # target copies after the updates of steps 0 and 2


def _shaped(got, like):
    return {k: got[k].reshape(like[k].shape) for k in like}


def _word(n, name):
    return int(n.debug_buffer(name)[:1].view(np.uint32)[0])


# ------------------------------------------------------------------ DQN


def _dqn_learner(name):
    c = S.DQN[name]
    net, params, target, batches = S.dqn_schedule(name)
    d = dqn_t._learner(net, c["max_batch"], target_update_period=DQN_PERIOD)
    return net, d, params, target, batches


def _dqn_run(d, batch, mean_over=None, q=None, priority_update=None):
    """One step: acme_dqn_step, or with mean_over the staged step a data-parallel rank
    issues (stages 0 and 1, then apply), the only entry that takes the denominator."""
    dev = dqn_t._dev(batch)
    if mean_over is None:
        d.step(*dev, q_tm1=q, priority_update=priority_update)
    else:
        d.forward_backward_stage(0, *dev, q_tm1=q, mean_over=mean_over)
        d.forward_backward_stage(1, *dev, mean_over=mean_over)
        d.apply()
    torch.cuda.synchronize()


def _tables():
    from acme_amd.native import NativeReplay
    rows = np.arange(600, dtype=np.uint32).view(np.uint8).reshape(600, 4)
    tables = [NativeReplay(1000, [4], prioritized=True, priority_exponent=0.6, seed=77)
              for _ in range(2)]
    for t in tables:
        t.insert([rows], np.linspace(0.5, 2.0, 600))
    torch.cuda.synchronize()
    return tables


@pytest.mark.parametrize("name", list(S.DQN))
def test_dqn_schedule_matches_oracle(name):
    """test_dqn_gpu's comparisons on every step: q, loss, TD errors and priorities at rtol
    1e-5, the gradients by _check_grads under the kernel's own ReLU pattern, Adam on the
    kernel's own gradients at rtol 1e-6, the target copied after the updates of steps 0 and
    2 and kept otherwise.  With mean_over the loss and every gradient are the oracle's batch
    means times B / mean_over; TD errors and priorities are the batch's own.  dqn_nature
    gives each step a table and keys: the priorities written inside the step equal those of
    a twin table updated from the step's output."""
    c = S.DQN[name]
    net, d, params, target, batches = _dqn_learner(name)
    cfg = dqn_t._cfg(net, target_update_period=DQN_PERIOD)
    d.set_params(params, target)
    tables = _tables() if c.get("rider") else None
    rode = d.update_rider_launches()
    z = {k: np.zeros_like(v) for k, v in params.items()}
    m, v = z, dict(z)
    A = net.num_actions
    for k, batch in enumerate(batches):
        B = len(batch["a_tm1"])
        q = torch.empty(B, A, device="cuda")
        update = None
        if tables:
            keys = tables[0].sample(B, k)["keys"]
            assert torch.equal(keys, tables[1].sample(B, k)["keys"])
            update = (tables[0].handle, keys)
        _dqn_run(d, batch, c.get("mean_over"), q, update)
        masks = dqn_t._relu_masks(d, net, batch, params, B)
        out, grads = DQ.dqn_loss_and_grads(cfg, params, target, batch, np.float64, masks=masks)
        share = B / c["mean_over"] if c.get("mean_over") else 1.0
        np.testing.assert_allclose(q.cpu().numpy(), out["q_tm1"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(d.loss.item(), out["loss"] * share, rtol=1e-5)
        np.testing.assert_allclose(d.td_error[:B].cpu().numpy(), out["td_error"], rtol=1e-5,
                                   atol=1e-6)
        np.testing.assert_allclose(d.priorities[:B].cpu().numpy(), out["priorities"], rtol=1e-5,
                                   atol=1e-6)
        g = d.get_params("grads")
        dqn_t._check_grads(g, {n: x * share for n, x in grads.items()})
        got, tgt = _shaped(d.get_params("params"), params), _shaped(d.get_params("target"), params)
        for n in params:
            want, m[n], v[n] = DQ.adam_update(params[n], g[n].reshape(params[n].shape), m[n],
                                              v[n], k + 1, cfg.learning_rate)
            np.testing.assert_allclose(got[n], want, rtol=1e-6, atol=1e-9, err_msg=f"{n} @{k}")
            np.testing.assert_array_equal(tgt[n], got[n] if k % DQN_PERIOD == 0 else target[n],
                                          err_msg=f"target {n} @{k}")
        if tables:
            tables[1].update_priorities(keys, d.priorities[:B])
            torch.cuda.synchronize()
            sa, sb = tables[0].debug_state(), tables[1].debug_state()
            for field in ("leaves", "raw", "keys"):
                np.testing.assert_array_equal(sa[field], sb[field], err_msg=f"{field} @{k}")
        assert d.num_steps == k + 1
        # Teacher forcing: the next step starts from the kernel's own state.
        params, target = got, tgt
        m, v = _shaped(d.get_params("m"), params), _shaped(d.get_params("v"), params)
    g = d.guard_state()
    assert g["applied"] == len(batches) and g["skipped"] == 0, g
    assert not d.plane_overflow()
    if tables:
        assert d.update_rider_launches() == rode + len(batches), "a write-back did not ride"


# ------------------------------------------------------------------ IMPALA


def _impala_learner(name):
    c = S.IMPALA[name]
    cfg, params, batches = S.impala_schedule(name)
    n = impala_t._native(cfg, *c["max"])
    if c.get("per_step"):
        n.set_lstm_unroll(True)
    return cfg, n, params, batches


def _impala_clean(name, n, steps):
    g = n.guard_state()
    assert g["applied"] == steps and g["skipped"] == 0 and g["lstm_timeouts"] == 0, g
    assert not n.plane_overflow()
    if S.IMPALA[name].get("one_launch"):
        assert _word(n, "lstm_timeout") == 0


@pytest.mark.parametrize("name", list(S.IMPALA))
def test_impala_schedule_matches_oracle(name):
    """test_impala_gpu._compare on every step, from the learner's own parameters and
    moments."""
    cfg, n, params, batches = _impala_learner(name)
    n.set_params(params)
    z = {k: np.zeros_like(v) for k, v in params.items()}
    m, v = z, dict(z)
    for k, b in enumerate(batches):
        impala_t._run(n, b)
        impala_t._compare(cfg, n, params, b, moments=(m, v, k))
        assert n.num_steps == k + 1
        params = _shaped(n.get_params("params"), params)
        m, v = _shaped(n.get_params("m"), params), _shaped(n.get_params("v"), params)
    _impala_clean(name, n, len(batches))


# ------------------------------------------------------------------ R2D2


@pytest.mark.parametrize("name", list(S.R2D2))
def test_r2d2_schedule_matches_oracle(name):
    """test_r2d2_learner_gpu._compare over the schedule: _check_step on every step, every
    step applied, and the sticky timeout word clear where the learner has the one-launch
    kernels."""
    c = S.R2D2[name]
    n = r2d2_t._compare(S.r2d2_cfg(name), *c["max"], seed=c["seed"], steps=len(c["steps"]),
                        maxima=c["max"], shapes=c["steps"])
    if name == "r2d2_rg":  # the used learner, started over on the two smallest shapes
        r2d2_t._compare(S.r2d2_cfg(name), *c["max"], seed=c["seed"] + 1, steps=2, learner=n,
                        shapes=c["steps"][2:4])
    if S.r2d2_one_launch(name):
        assert _word(n, "lstm_timeout") == 0


# ------------------------------------------------------------------ D4PG / DDPG / MPO / DMPO


def test_d4pg_schedule_matches_oracle():
    """test_d4pg_gpu's comparisons (test_full_size_steps_match_oracle's, with the logits and
    dqda of test_limits_gpu._d4pg_step at the bars of the golden step) on every step."""
    c = S.AC["d4pg"]
    cfg = c["cfg"]
    n = d4pg_t._native(cfg, S.AC_MAX)
    params, target = S.ac_params("d4pg")
    n.set_params(params, target)
    z = {k: np.zeros_like(v) for k, v in params.items()}
    state = dict(params=params, target=target, m=z, v=dict(z), num_steps=0)
    K, A = cfg.num_atoms, cfg.act_dim
    for s, B in enumerate(S.AC_STEPS):
        batch, _ = S.ac_batch("d4pg", s)
        n.step(*d4pg_t._dev(batch))
        torch.cuda.synchronize()
        ref, raw, state = D4.d4pg_step(cfg, state, batch, np.float64)
        d4pg_t._close(n.critic_loss.item(), ref["critic_loss"], name=f"critic_loss@{s}")
        d4pg_t._close(n.policy_loss.item(), ref["policy_loss"], rtol=1e-4, name=f"policy_loss@{s}")
        d4pg_t._close(n.debug_buffer("c_logits")[:B * K], ref["q_tm1"], name=f"q_tm1@{s}")
        d4pg_t._close(n.debug_buffer("t_logits")[:B * K], ref["q_t"], name=f"q_t@{s}")
        d4pg_t._close(n.debug_buffer("dqda")[:B * A], ref["dqda"], rtol=1e-4, name=f"dqda@{s}")
        d4pg_t._close(n.debug_buffer("norms"), ref["norms"], rtol=1e-4, name=f"norms@{s}")
        d4pg_t._check_grads(n, raw)
        got = n.get_params("params")
        d4pg_t._check_params(got, state["params"], cfg.policy_lr)
        state["params"] = {k: got[k].astype(np.float32) for k in got}
        state["m"] = n.get_params("m")
        state["v"] = n.get_params("v")
        tgt = n.get_params("target")
        for k, r in state["target"].items():
            np.testing.assert_array_equal(tgt[k], np.asarray(r, np.float32), err_msg=f"{k}@{s}")
        state["target"] = tgt
    assert n.num_steps == len(S.AC_STEPS)


def test_ddpg_schedule_matches_oracle():
    c = S.AC["ddpg"]
    n = ddpg_t._run_steps(c["cfg"], S.AC_MAX, S.AC_STEPS, len(S.AC_STEPS), c["pseed"],
                          c["bseed"])
    # The used learner, started over on the two smallest batches.
    ddpg_t._run_steps(c["cfg"], S.AC_MAX, (4, 1), 2, c["pseed"] + 2, c["bseed"] + 5, learner=n)


def test_mpo_schedule_matches_oracle():
    c = S.AC["mpo"]
    n = mpo_t._native(c["cfg"], S.AC_MAX)
    mpo_t._run_steps(c["cfg"], S.AC_STEPS, len(S.AC_STEPS), c["pseed"], c["bseed"],
                     mean_scale=c["mean_scale"], learner=n)


def test_dmpo_schedule_matches_oracle():
    """check_branches off: a one-row batch cannot take every branch of the projection;
    schedule_cases.dmpo_batch asserts them on every batch of two rows or more."""
    c = S.AC["dmpo"]
    dmpo_t._run_steps(c["cfg"], S.AC_STEPS, len(S.AC_STEPS), c["pseed"], c["bseed"],
                      critic_scale=c["critic_scale"], batch_fn=S.dmpo_batch,
                      check_branches=False, max_batch=S.AC_MAX)


# ------------------------------------------------------------------ independence from history

_FLAT = ("params", "target", "m", "v")


def _save(n):
    """The full learner state: the flat buffers, the step counts and, on the plane learners,
    the scale state."""
    st = {buf: getattr(n, buf).clone() for buf in _FLAT if hasattr(n, buf)}
    st["num_steps"] = n.num_steps
    if hasattr(n, "scale_state"):
        st["applied"] = n.guard_state()["applied"]
        st["scales"] = n.scale_state()
    return st


def _restore(n, st):
    """params_changed, then the counts, then set_scale_state (test_plane_state_gpu)."""
    for buf in _FLAT:
        if buf in st:
            getattr(n, buf).copy_(st[buf])
    n.params_changed()
    n.num_steps = st["num_steps"]
    if "scales" in st:
        n.applied_steps = st["applied"]
        n.set_scale_state(st["scales"])
        np.testing.assert_array_equal(n.scale_state(), st["scales"])


def _state_out(n):
    """What every step leaves in the learner's state."""
    out = {f"{buf}/{k}": x for buf in _FLAT + ("grads",) if hasattr(n, buf)
           for k, x in n.get_params(buf).items()}
    out["num_steps"] = np.asarray(n.num_steps)
    if hasattr(n, "scale_state"):
        out["scales"] = n.scale_state()
        for k, x in n.guard_state().items():
            out[f"guard/{k}"] = np.asarray(x)
    return out


def _independent(make, run, outputs, batches, k):
    """Steps 0..k-1 on one learner, then step k three times: on it, on it again restored to
    the state before the step, and on a fresh learner restored to that state."""
    used = make()
    for b in batches[:k]:
        run(used, b)
    saved = _save(used)
    assert saved["num_steps"] == k
    run(used, batches[k])
    first = dict(outputs(used, batches[k]), **_state_out(used))
    fresh = make()
    for who, n in (("used", used), ("fresh", fresh)):
        _restore(n, saved)
        run(n, batches[k])
        again = dict(outputs(n, batches[k]), **_state_out(n))
        assert again.keys() == first.keys()
        for key in first:
            np.testing.assert_array_equal(again[key], first[key],
                                          err_msg=f"{who} learner: {key}")
    if "guard/skipped" in first:
        assert first["guard/skipped"] == 0 and first["guard/applied"] == k + 1


@pytest.mark.parametrize("name", list(S.DQN))
def test_dqn_small_step_is_independent_of_history(name):
    c = S.DQN[name]
    net, _, params, target, batches = _dqn_learner(name)
    A = net.num_actions
    qs = {}

    def make():
        d = _dqn_learner(name)[1]
        d.set_params(params, target)
        return d

    def run(d, batch):
        qs[id(d)] = torch.empty(len(batch["a_tm1"]), A, device="cuda")
        _dqn_run(d, batch, c.get("mean_over"), qs[id(d)])

    def outputs(d, batch):
        B = len(batch["a_tm1"])
        return dict(loss=d.loss.cpu().numpy(), td=d.td_error[:B].cpu().numpy(),
                    priorities=d.priorities[:B].cpu().numpy(), q=qs[id(d)].cpu().numpy(),
                    overflow=np.asarray(d.plane_overflow()))

    _independent(make, run, outputs, batches, S.small_step(c["steps"]))


@pytest.mark.parametrize("name", list(S.IMPALA))
def test_impala_small_step_is_independent_of_history(name):
    c = S.IMPALA[name]
    cfg, _, params, batches = _impala_learner(name)
    A, H = cfg.num_actions, cfg.lstm_size

    def make():
        n = _impala_learner(name)[1]
        n.set_params(params)
        return n

    def outputs(n, b):
        B, T = b["action"].shape
        buf = n.debug_buffer
        out = dict(metrics=n.metrics.cpu().numpy(), pv=buf("pv")[:B * T * (A + 1)],
                   vs=buf("vs")[:(T - 1) * B], pg_adv=buf("pg_adv")[:(T - 1) * B],
                   h=buf("h")[:B * T * H], c=buf("c")[:B * T * H],
                   dgates=buf("dgates")[:B * T * 4 * H],
                   overflow=np.asarray(n.plane_overflow()))
        if c.get("one_launch"):
            out["lstm_timeout"] = np.asarray(_word(n, "lstm_timeout"))
        return out

    _independent(make, impala_t._run, outputs, batches, S.small_step(c["steps"]))


@pytest.mark.parametrize("name", list(S.R2D2))
def test_r2d2_small_step_is_independent_of_history(name):
    c = S.R2D2[name]
    cfg, params, target, batches = S.r2d2_schedule(name)
    A, H = cfg.num_actions, cfg.lstm_size

    def make():
        n = r2d2_t._native(cfg, *c["max"])
        n.set_params(params, target)
        return n

    def outputs(n, b):
        B, T = b["action"].shape
        L = T - cfg.burn_in_length
        buf = n.debug_buffer
        out = dict(loss=n.loss.cpu().numpy(), errors=n.errors.cpu().numpy(),
                   priorities=n.priorities[:B].cpu().numpy(), q=buf("q")[:L * B * A],
                   target_q=buf("target_q")[:L * B * A], g=buf("g")[:L * B],
                   h=buf("h")[:B * T * H])
        if S.r2d2_one_launch(name):
            out["lstm_timeout"] = np.asarray(_word(n, "lstm_timeout"))
        return out

    _independent(make, r2d2_t._run, outputs, batches, S.small_step(c["steps"]))


@pytest.mark.parametrize("name", list(S.AC))
def test_actor_critic_small_step_is_independent_of_history(name):
    c = S.AC[name]
    mod = S.AC_MODULES[name]
    params, target = S.ac_params(name)
    batches = [S.ac_batch(name, s) for s in range(len(S.AC_STEPS))]

    def make():
        n = mod._native(c["cfg"], S.AC_MAX)
        n.set_params(params, target)
        return n

    def run(n, b):
        batch, eps = b
        kw = dict(noise=torch.as_tensor(eps).cuda()) if eps is not None else {}
        n.step(*mod._dev(batch), **kw)
        torch.cuda.synchronize()

    def outputs(n, b):
        out = dict(critic_loss=n.critic_loss.cpu().numpy(), policy_loss=n.policy_loss.cpu().numpy(),
                   norms=n.debug_buffer("norms"))
        if name in ("mpo", "dmpo"):
            out.update(stats=n.stats.cpu().numpy(), kl_mean_rel=n.kl_mean_rel.cpu().numpy(),
                       kl_stddev_rel=n.kl_stddev_rel.cpu().numpy())
        return out

    _independent(make, run, outputs, batches, S.small_step(S.AC_STEPS))
