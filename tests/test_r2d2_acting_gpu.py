"""The R2D2 acting step (acme_r2d2_q_step, csrc/r2d2_learner.hip) and the epsilon-greedy
selection (acme_epsilon_greedy, csrc/kernels.hip) on the GPU.

q, h_out and c_out against oracle.r2d2_oracle.forward in float64 on the parameters the GPU
holds, at tests/test_r2d2_learner_gpu.py's bars for the network forwards (_close: rtol 1e-5
plus 2e-6 of the tensor's scale; the same f32 kernels as one time step of the learner's
unroll).  The selection is integer arithmetic on one Philox call per row: bit-exact against
tests/r2d2_act_oracle.py on the q the call returned.  Acting must leave a learner's steps
bit-identical to those of a twin that never acted.
"""

import types

import numpy as np
import pytest
import torch

from oracle import r2d2_oracle as O
from tests import r2d2_act_oracle as S
from tests.test_r2d2_learner_gpu import _batch, _cfg, _close, _native, _params, _run

pytestmark = pytest.mark.gpu

FLAT = dict(num_actions=5, lstm_size=16, head_size=8, obs_dim=6)
ATARI = dict(torso="atari", num_actions=18, lstm_size=256, head_size=64, obs_dim=0)
MAX_BATCH, SEQ = 4, 4  # the learners' max_batch; burn-in 2 + 2 steps


class _Net:
    """A learner with distinct online / target draws, and its numpy parameters."""

    def __init__(self, cfg, B=MAX_BATCH, T=SEQ, seed=0):
        self.cfg = cfg
        self.n = _native(cfg, B, T)
        self.params, self.target = _params(cfg, 50 + seed), _params(cfg, 60 + seed)
        self.n.set_params(self.params, self.target)


@pytest.fixture(scope="module")
def nets():
    return {"flat": _Net(_cfg(**FLAT)), "atari": _Net(_cfg(**ATARI), seed=1)}


def _inputs(cfg, rows, T, seed):
    """[rows, T] actor inputs and an initial state, in _batch's layout."""
    return _batch(cfg, rows, T, seed)


def _dev(x):
    return torch.as_tensor(x).cuda().contiguous()


def _step_inputs(b, t, rows=None):
    r = slice(0, rows)
    return _dev(b["obs"][r, t]), _dev(b["prev_action"][r, t]), _dev(b["prev_reward"][r, t])


def _strided_state(b, rows=None):
    """h / c as [rows, H] views of one [rows, 2, H] tensor: row stride 2 H."""
    st = _dev(np.stack([b["h0"], b["c0"]], axis=1)[:rows])
    return st[:, 0], st[:, 1]


def _reference(cfg, params, b, rows=None):
    """(q [rows, T, A], h [rows, T, H], c [rows, T, H]) of the f64 unroll."""
    bb = {k: v[:rows] for k, v in b.items() if k != "probabilities"}
    q, cache = O.forward(cfg, params, bb, np.float64)
    return q, cache["hs"], cache["cs"]


def _check_one_step(net, b, rows, use_target, ref=None, tag=""):
    cfg, n = net.cfg, net.n
    params = n.get_params("target" if use_target else "params")
    q_ref, h_ref, c_ref = ref if ref is not None else _reference(cfg, params, b, rows)
    h, c = _strided_state(b, rows)
    q, a, h1, c1 = n.q_step(*_step_inputs(b, 0, rows), h, c, epsilon=0.0, seed=1, step=0,
                            use_target=use_target)
    torch.cuda.synchronize()
    name = f"{tag} rows {rows} target {use_target}"
    _close(q.cpu().numpy(), q_ref[:rows, 0], name="q " + name)
    _close(h1.cpu().numpy(), h_ref[:rows, 0], name="h " + name)
    _close(c1.cpu().numpy(), c_ref[:rows, 0], name="c " + name)
    np.testing.assert_array_equal(a.cpu().numpy(), S.select(q.cpu().numpy(), 0.0, 1, 0))
    return q


# ------------------------------------------------------------------ A. one step
@pytest.mark.parametrize("torso,rows", [("flat", 1), ("flat", 3), ("flat", 4), ("atari", 1),
                                        ("atari", 3)])
def test_one_step_matches_oracle(nets, torso, rows):
    net = nets[torso]
    b = _inputs(net.cfg, rows, 1, 7 + rows)
    q_on = _check_one_step(net, b, rows, False, tag=torso)
    q_tg = _check_one_step(net, b, rows, True, tag=torso)
    assert not np.array_equal(q_on.cpu().numpy(), q_tg.cpu().numpy())


# ------------------------------------------------------------------ B. chained steps
@pytest.mark.parametrize("torso", ["flat", "atari"])
def test_chained_steps_equal_an_unroll(nets, torso):
    net, rows, T = nets[torso], 3, 5
    cfg, n = net.cfg, net.n
    b = _inputs(cfg, rows, T, 21)
    q_ref, h_ref, c_ref = _reference(cfg, n.get_params("params"), b)
    h, c = _dev(b["h0"]), _dev(b["c0"])
    q = torch.empty(rows, cfg.num_actions, dtype=torch.float32, device="cuda")
    for t in range(T):  # the state fed back in place
        n.q_step(*_step_inputs(b, t), h, c, epsilon=0.0, seed=0, step=t, out=[q, None, h, c])
        torch.cuda.synchronize()
        _close(q.cpu().numpy(), q_ref[:, t], name=f"{torso} q at t = {t}")
    _close(h.cpu().numpy(), h_ref[:, T - 1], name=f"{torso} final h")
    _close(c.cpu().numpy(), c_ref[:, T - 1], name=f"{torso} final c")


# ------------------------------------------------------------------ C. selection
@pytest.mark.parametrize("epsilon", [0.0, 0.3, 1.0])
def test_q_step_actions_are_the_oracles(nets, epsilon):
    net, rows = nets["flat"], 4
    b = _inputs(net.cfg, rows, 1, 33)
    h, c = _strided_state(b)
    draws = {}
    for step in (5, 6, 5, 2 ** 40 + 1):
        q, a, _, _ = net.n.q_step(*_step_inputs(b, 0), h, c, epsilon=epsilon, seed=99, step=step)
        torch.cuda.synchronize()
        a = a.cpu().numpy()
        assert a.dtype == np.int32
        np.testing.assert_array_equal(a, S.select(q.cpu().numpy(), epsilon, 99, step),
                                      err_msg=f"step {step}")
        if step in draws:  # the same (seed, step) repeats
            np.testing.assert_array_equal(a, draws[step])
        draws[step] = a
    if epsilon == 1.0:  # the oracle's draws of steps 5 and 6 differ (checked on the CPU)
        assert (draws[5] != draws[6]).any()
    # Without a q output the actions are the same.
    a_only = torch.empty(rows, dtype=torch.int32, device="cuda")
    net.n.q_step(*_step_inputs(b, 0), h, c, epsilon=epsilon, seed=99, step=5,
                 out=[None, a_only, None, None])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(a_only.cpu().numpy(), draws[5])


@pytest.mark.parametrize("num_actions", [5, 70])
def test_one_launch_ending_equals_the_two_launches(num_actions):
    """ACME_V_R2ACT=1 at creation (the head finish and the selection in one launch, the form
    tools/r2d2_act_time.py compares): the same q bits and the same actions."""
    from acme_amd._lib import lib
    cfg, rows = _cfg(**dict(FLAT, num_actions=num_actions)), 4
    lib().acme_tune_set(b"R2ACT", 1)  # read at the learner's creation
    try:
        fused = _native(cfg, MAX_BATCH, SEQ)
    finally:
        lib().acme_tune_set(b"R2ACT", 0)
    plain = _native(cfg, MAX_BATCH, SEQ)
    p, t = _params(cfg, 80), _params(cfg, 81)
    p[f"{O.PREFIX}/duelling_q_network/mlp_1/linear_1/w"][:, 1] = \
        p[f"{O.PREFIX}/duelling_q_network/mlp_1/linear_1/w"][:, 3]  # actions 1 and 3 tie
    p[f"{O.PREFIX}/duelling_q_network/mlp_1/linear_1/b"][1] = \
        p[f"{O.PREFIX}/duelling_q_network/mlp_1/linear_1/b"][3]
    b = _inputs(cfg, rows, 1, 90)
    outs = []
    for n in (fused, plain):
        n.set_params(p, t)
        h, c = _strided_state(b)
        q, a, _, _ = n.q_step(*_step_inputs(b, 0), h, c, epsilon=0.3, seed=4, step=8)
        a_only = torch.empty(rows, dtype=torch.int32, device="cuda")
        n.q_step(*_step_inputs(b, 0), h, c, epsilon=0.3, seed=4, step=8,
                 out=[None, a_only, None, None])
        torch.cuda.synchronize()
        outs.append((q.cpu().numpy(), a.cpu().numpy(), a_only.cpu().numpy()))
    (q1, a1, o1), (q2, a2, o2) = outs
    np.testing.assert_array_equal(q1, q2)
    np.testing.assert_array_equal(q1[:, 1], q1[:, 3])
    want = S.select(q1, 0.3, 4, 8)
    for got in (a1, o1, a2, o2):
        np.testing.assert_array_equal(got, want)


def _hand_made_rows():
    rng = np.random.default_rng(3)
    f = np.float32
    cases = {}
    cases["all equal"] = np.full((257, 5), 1.25, f)
    two = rng.standard_normal((257, 6)).astype(f)
    two[:, 1] = two[:, 4] = two.max(axis=1) + 1
    cases["two ties"] = two
    cases["A = 1"] = rng.standard_normal((257, 1)).astype(f)
    wide = rng.standard_normal((257, 70)).astype(f)  # more than one wave
    wide[::2, [3, 64, 69]] = 9.0
    cases["A = 70"] = wide
    big = rng.standard_normal((257, 1024)).astype(f)
    big[::2, [0, 63, 64, 500, 1023]] = 9.0
    big[1::4, 1023] = 11.0
    cases["A = 1024"] = big
    nan = rng.standard_normal((257, 7)).astype(f)
    nan[:, 2] = np.nan
    nan[::3, 5] = np.nan
    nan[::5, 0] = np.inf
    nan[::7, :] = -np.inf
    cases["NaN beside finite"] = nan
    allnan = rng.standard_normal((257, 4)).astype(f)
    allnan[::2] = np.nan
    cases["all-NaN rows"] = allnan
    cases["signed zeros"] = np.tile(np.array([-0.0, 0.0, -1.0, 0.0], f), (257, 1))
    return cases


@pytest.mark.parametrize("name", list(_hand_made_rows()))
def test_epsilon_greedy_on_hand_made_rows(name):
    from acme_amd.native import epsilon_greedy
    q = _hand_made_rows()[name]
    for rows in (1, 257):
        for epsilon in (0.0, 0.3, 1.0):
            got = epsilon_greedy(_dev(q[:rows]), epsilon, seed=7, step=11).cpu().numpy()
            np.testing.assert_array_equal(got, S.select(q[:rows], epsilon, 7, 11),
                                          err_msg=f"{name} rows {rows} epsilon {epsilon}")
    assert got.dtype == np.int32 and got.min() >= 0 and got.max() < q.shape[1]


def test_epsilon_greedy_argument_checks():
    from acme_amd.native import epsilon_greedy
    q = _dev(np.zeros((2, 3), np.float32))
    for eps in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            epsilon_greedy(q, eps, 0, 0)
    with pytest.raises(ValueError):
        epsilon_greedy(_dev(np.zeros((2, 1025), np.float32)), 0.1, 0, 0)
    with pytest.raises(ValueError):
        epsilon_greedy(q.double(), 0.1, 0, 0)


# ------------------------------------------------------------------ D. the learner is left alone
def _learner_state(n):
    s = {f"{w}/{k}": v for w in ("params", "target", "m", "v")
         for k, v in n.get_params(w).items()}
    s["loss"] = n.loss.cpu().numpy().copy()
    s["errors"] = n.errors.cpu().numpy().copy()
    s["priorities"] = n.priorities.cpu().numpy().copy()
    s["scales"] = n.scale_state()
    g = n.guard_state()
    s["guard"] = np.array([g["applied"], g["skipped"], g["last_skipped"]])
    s["num_steps"] = np.array([n.num_steps])
    return s


@pytest.mark.parametrize("torso", ["flat", "atari"])
def test_acting_leaves_the_learner_alone(torso):
    """Twin learners take the same three steps (target_update_period 2); one answers q_steps
    (rows 1 and 3, online and target) before and between them, the other none."""
    if torso == "flat":
        cfg, B, T = _cfg(), 3, 9
    else:  # test_r2d2_atari_step_matches_oracle's shapes: the plane path
        cfg, B, T = _cfg(torso="atari", num_actions=18, lstm_size=512, head_size=512, obs_dim=0,
                         burn_in_length=2, n_step=2), 3, 6
    assert cfg.target_update_period == 2
    twins = [_native(cfg, B, T), _native(cfg, B, T)]
    p0, t0 = _params(cfg, 70), _params(cfg, 71)
    for n in twins:
        n.set_params(p0, t0)
    actor = twins[0]
    for k in range(3):
        b = _inputs(cfg, 3, 1, 40 + k)
        for use_target in (False, True):
            params = actor.get_params("target" if use_target else "params")
            ref = _reference(cfg, params, b)  # rows are independent: rows 1 is its first row
            for rows in (1, 3):
                net = types.SimpleNamespace(cfg=cfg, n=actor)
                _check_one_step(net, b, rows, use_target, ref=ref, tag=f"{torso} before step {k}")
        batch = _batch(cfg, B, T, 300 + k)
        states = []
        for n in twins:
            _run(n, batch)
            states.append(_learner_state(n))
        assert states[0].keys() == states[1].keys()
        for key in states[0]:
            np.testing.assert_array_equal(states[0][key], states[1][key],
                                          err_msg=f"{torso} step {k}: {key}")
        assert np.isfinite(states[0]["loss"]).all()
        assert states[0]["guard"][1] == 0 and states[0]["num_steps"][0] == k + 1


# ------------------------------------------------------------------ E. argument checks
def test_q_step_argument_checks(nets):
    net = nets["flat"]
    cfg, n, H = net.cfg, net.n, net.cfg.lstm_size
    b = _inputs(cfg, MAX_BATCH + 1, 1, 55)

    def call(rows, epsilon=0.1, state=None):
        h, c = state if state is not None else _strided_state(b, rows)
        return n.q_step(*_step_inputs(b, 0, rows), h, c, epsilon=epsilon, seed=0, step=0)

    for rows in (0, MAX_BATCH + 1):
        with pytest.raises(ValueError):
            call(rows)
    for eps in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            call(2, epsilon=eps)
    # State rows that start 4 bytes off a 16-byte boundary (row stride H + 4 floats).
    wide = torch.zeros(2, 2, H + 4, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        call(2, state=(wide[:, 0, 1:H + 1], wide[:, 1, 1:H + 1]))
    # A row stride that is no multiple of 4 floats.
    odd = torch.zeros(2, 2, H + 2, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        call(2, state=(odd[:, 0, :H], odd[:, 1, :H]))
    torch.cuda.synchronize()
    _check_one_step(net, b, 3, False, tag="after the refused calls")
