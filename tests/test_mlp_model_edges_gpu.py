"""The native learned model (acme_mlp_model_*) where tests/test_mlp_model_gpu.py does not reach:
row groups of several 16-row tiles, one handle stepped at many batch sizes, what the gather may
read, ordering on a stream, resume, the smallest accepted shape and exact zeros.

The oracle, the helpers and the tolerances are those of tests/test_mlp_model_gpu.py (its header
states them); nothing here adds or widens one."""

import numpy as np
import pytest
import torch

from tests import mlp_model_oracle as O
from tests.test_az_gpu import _state_of
from tests.test_mlp_model_gpu import (RING, _check_pred, _check_step, _idx, _native, _params,
                                      _ring)

pytestmark = pytest.mark.gpu

CFG = O.Config(7, (36, 68), 5)  # every width off the MFMA tile, 68 past the 64-column stride


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _load(n, saved, num_steps):
    """params, m, v (flat device tensors) and the step count into the handle."""
    for dst, src in zip((n.params, n.m, n.v), saved):
        dst.copy_(src)
    n.num_steps = num_steps


def _min_preact(cfg, params, obs, actions):
    """The smallest |z| among the hidden pre-activations of all towers."""
    acts = O.forward(cfg, params, obs, actions)[3]
    return min(np.abs(acts[t][i] @ np.asarray(params[f"{t}/linear_{i}/w"], np.float64)
                      + np.asarray(params[f"{t}/linear_{i}/b"], np.float64)).min()
               for t in O.TOWERS for i in range(len(cfg.hidden)))


# ----------------------------------------------------------------- several tiles per group
# Eight row groups: a group takes a second tile from B = 129 on.  129: group 0's second tile has
# one row; 137: nine rows; 145: two groups with two tiles, six with one; 272: 17 full tiles,
# group 0 has three.
@pytest.mark.parametrize("B", [129, 137, 145, 272])
def test_several_tiles_per_group(B):
    n = _native(CFG, B)
    n.set_params(_params(CFG, 1))
    ring = _ring(CFG, 2)  # 40 rows: every index repeats
    for s in range(3):  # teacher-forced
        _check_step(n, CFG, _state_of(n), ring, _idx(B, 10 + s), tag=f" B={B} t={s + 1}")


def test_several_tiles_per_group_k4_padding():
    cfg = O.Config(50, (50,), 3)  # D + A = 53: layer 0's k loop is padded to 56
    n = _native(cfg, 137)
    n.set_params(_params(cfg, 3))
    _check_step(n, cfg, _state_of(n), _ring(cfg, 4), _idx(137, 5), tag=" B=137 D=50")


# ----------------------------------------------------------------- one handle, many batch sizes
def test_one_handle_many_batch_sizes():
    D = CFG.obs_dim
    n = _native(CFG, 145)
    n.set_params(_params(CFG, 6))
    ring = _ring(CFG, 7)
    saved = [x.clone() for x in (n.params, n.m, n.v)]
    for i, B in enumerate((145, 5, 33, 1, 145)):  # 8 slots, then 1, 3, 1, 8
        _check_step(n, CFG, _state_of(n), ring, _idx(B, 30 + i), tag=f" B={B} (step {i + 1})")
        if B == 5:
            assert n.debug_buffer("pred").size == 5 * (D + 2)
            assert n.debug_buffer("dout").size == 5 * (D + 2)
    dring = torch.as_tensor(ring).cuda()
    for B in (146, 0):
        with pytest.raises(ValueError, match="batch must be in"):
            n.step(dring, torch.zeros(B, dtype=torch.int32, device="cuda"))
    assert n.num_steps == 5
    # Nothing of those steps is left in the handle: from the first state, a step at B = 33 is
    # bit for bit a fresh handle's.
    idx = torch.as_tensor(_idx(33, 40)).cuda()
    fresh = _native(CFG, 145)
    got = []
    for h in (n, fresh):
        _load(h, saved, 0)
        h.step(dring, idx)
        torch.cuda.synchronize()
        assert h.num_steps == 1
        got.append([_bits(x) for x in (h.params, h.grads, h._losses)])  # noqa: SLF001
    for x, y, name in zip(*got, ("params", "grads", "losses")):
        np.testing.assert_array_equal(x, y, err_msg=name)


# ----------------------------------------------------------------- the gather reads what it should
def test_indices_outside_the_ring_are_clamped():
    """The ring is rows 8 .. 8 + R of a larger tensor whose other rows hold 1e6, and no index is
    further than 8 rows outside: a gather without the clamp reads 1e6, never unowned memory."""
    R, B = RING, 33
    ring = _ring(CFG, 41)
    big = np.full((8 + R + 8, ring.shape[1]), 1e6, np.float32)
    big[8:8 + R] = ring
    dev = torch.as_tensor(big).cuda()[8:8 + R]
    idx = _idx(B, 42)
    idx[[1, 5, 9, 17]] = [-1, -8, R, R + 7]  # 17: the first row of the second tile
    assert idx.min() == -8 and idx.max() == R + 7
    n = _native(CFG, B)
    n.set_params(_params(CFG, 43))
    _check_step(n, CFG, _state_of(n), ring, idx, tag=" clamp", dev=dev, clamp=True)


def test_step_reads_only_its_rows_and_columns():
    """NaN in every ring row the batch does not name and in the columns past 2 D + 3."""
    B, D = 33, CFG.obs_dim
    ring = _ring(CFG, 44)
    used = np.arange(1, RING, 3)
    idx = used[np.random.default_rng(45).integers(0, len(used), B)].astype(np.int32)
    unused = np.ones(RING, bool)
    unused[used] = False
    ring[unused] = np.nan
    ring[:, 2 * D + 3:] = np.nan
    assert np.isnan(ring).sum() == unused.sum() * ring.shape[1] + 2 * len(used)
    n = _native(CFG, B)
    n.set_params(_params(CFG, 46))
    _check_step(n, CFG, _state_of(n), ring, idx, tag=" poison")  # asserts finite losses


def test_actions_outside_the_range_set_no_column():
    B, D, A = 33, CFG.obs_dim, CFG.num_actions
    n = _native(CFG, B)
    n.set_params(_params(CFG, 47))
    ring = _ring(CFG, 48, actions=[-1, A, A + 100, 0, 1, 2, 3, 4])
    idx = _idx(B, 49)
    a = ring[idx, D]
    assert {-1, A, A + 100} <= set(a.tolist()) and ((a >= 0) & (a < A)).sum() >= 8
    _check_step(n, CFG, _state_of(n), ring, idx, tag=" mixed actions")
    ring = _ring(CFG, 50, actions=[-1, A, A + 100])
    _check_step(n, CFG, _state_of(n), ring, _idx(B, 51), tag=" no action in range")
    g = n.get_params("grads")
    for tower in O.TOWERS:
        w = g[f"{tower}/linear_0/w"]
        assert (w[D:] == 0.0).all() and np.abs(w[:D]).max() > 0.0, tower


def test_predict_reads_and_writes_only_its_rows():
    D, A = CFG.obs_dim, CFG.num_actions
    n = _native(CFG, 4, rows=8)
    p = _params(CFG, 52)
    n.set_params(p)
    state = np.random.default_rng(53).standard_normal((5, D + 3)).astype(np.float32)
    state[:, D:] = np.nan
    actions = np.array([-1, 0, A, 3, A - 1], np.int32)
    dstate = torch.as_tensor(state).cuda()
    buf = torch.full((8, D + 2), -7.5, device="cuda")
    n.predict_packed(dstate, torch.as_tensor(actions).cuda(), out=buf[:5])
    torch.cuda.synchronize()
    s, r, x, acts = O.forward(CFG, p, state[:, :D], actions)
    _check_pred(CFG, p, buf[:5].cpu().numpy(), np.column_stack([s, r, x]), acts, " 5 of 8 rows")
    np.testing.assert_array_equal(_bits(buf[5:]), np.full((3, D + 2), -7.5, np.float32).view(np.uint32))
    out = n.predict_packed(dstate[:1], A)  # by value, outside the range
    s, r, x, acts = O.forward(CFG, p, state[:1, :D], [A])
    _check_pred(CFG, p, out.cpu().numpy(), np.column_stack([s, r, x]), acts, " action0 = A")


# ----------------------------------------------------------------- ordering and resume
@pytest.mark.parametrize("stream", ["default", "side"])
def test_predict_sees_the_update(stream):
    B, D = 8, CFG.obs_dim
    n = _native(CFG, B, rows=2)
    n.set_params(_params(CFG, 54))
    ring, idx = _ring(CFG, 55), _idx(B, 56)
    state = _state_of(n)
    dring, didx = torch.as_tensor(ring).cuda(), torch.as_tensor(idx).cuda()
    actions = ring[:2, D].astype(np.int32)
    dact = torch.as_tensor(actions).cuda()
    st = None
    if stream == "side":
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())  # the uploads above
    n.step(dring, didx, stream=st)
    out = n.predict_packed(dring[:2], dact, stream=st)  # no synchronisation in between
    torch.cuda.synchronize()
    _, _, new = O.step(CFG, state, O.batch_of(CFG, ring, idx))
    s, r, x, acts = O.forward(CFG, new["params"], ring[:2, :D], actions)
    ref = np.column_stack([s, r, x])
    s0, r0, x0, _ = O.forward(CFG, state["params"], ring[:2, :D], actions)
    old = np.column_stack([s0, r0, x0])
    assert np.abs(ref - old).max() > 1e-4  # the step moved them far past the tolerance
    _check_pred(CFG, new["params"], out.cpu().numpy(), ref, acts, f" after step ({stream})")


def test_resume_continues_bit_for_bit():
    B = 33
    dring = torch.as_tensor(_ring(CFG, 57)).cuda()
    idx = [torch.as_tensor(_idx(B, 60 + s)).cuda() for s in range(4)]
    a = _native(CFG, B)
    a.set_params(_params(CFG, 58))
    for s in range(4):
        a.step(dring, idx[s])
        if s == 1:
            torch.cuda.synchronize()
            saved = [x.clone() for x in (a.params, a.m, a.v)]
    torch.cuda.synchronize()
    assert a.num_steps == 4

    def resumed(num_steps):
        h = _native(CFG, B)
        _load(h, saved, num_steps)
        h.step(dring, idx[2])
        h.step(dring, idx[3])
        torch.cuda.synchronize()
        return h

    b = resumed(2)
    assert b.num_steps == 4
    for x, y, name in zip((a.params, a.m, a.v), (b.params, b.m, b.v), ("params", "m", "v")):
        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=name)
    c = resumed(0)  # Adam's bias correction comes from the handle's step count
    assert c.num_steps == 2
    assert (_bits(a.params) != _bits(c.params)).mean() > 0.5


# ----------------------------------------------------------------- smallest shape, exact zeros
# Seeds (params, ring) at which every hidden pre-activation of the oracle is at least 1e-3 from
# zero, so that no ReLU can fall on different sides in f32 and f64; no gradient there is both
# nonzero and below 1e-3 (Adam's first step divides by |g| + eps), and at (1, 1, 1) two towers
# are alive through every layer and the third is dead.
@pytest.mark.parametrize("hidden,B,seeds", [((1,), 1, (1, 5)), ((1, 1, 1), 2, (19, 117))])
def test_smallest_shape(hidden, B, seeds):
    cfg = O.Config(1, hidden, 1)
    p, ring = _params(cfg, seeds[0]), _ring(cfg, seeds[1])
    idx = _idx(B, 5)
    assert _min_preact(cfg, p, ring[idx, :1], ring[idx, 1]) >= 1e-3
    n = _native(cfg, B, rows=1)
    n.set_params(p)
    _check_step(n, cfg, _state_of(n), ring, idx, tag=f" smallest {hidden}")
    p = n.get_params("params")
    assert _min_preact(cfg, p, ring[:1, :1], [0]) >= 1e-3
    out = n.predict_packed(torch.as_tensor(ring[:1]).cuda(), 0)  # NP = 1: 256 partials a column
    s, r, x, acts = O.forward(cfg, p, ring[:1, :1], [0])
    _check_pred(cfg, p, out.cpu().numpy(), np.column_stack([s, r, x]), acts, f" smallest {hidden}")


def test_dead_layer_gives_exact_zeros():
    B, D = 33, CFG.obs_dim
    p = _params(CFG, 70)
    for tower in O.TOWERS:
        p[f"{tower}/linear_1/b"][:] = -100.0
    ring, idx = _ring(CFG, 71), _idx(B, 72)
    acts = O.forward(CFG, p, ring[idx, :D], ring[idx, D])[3]
    for tower in O.TOWERS:
        assert acts[tower][1].max() > 0.0 and (acts[tower][2] == 0.0).all(), tower
    n = _native(CFG, B)
    n.set_params(p)
    _check_step(n, CFG, _state_of(n), ring, idx, tag=" dead layer")
    g = n.get_params("grads")
    for tower in O.TOWERS:
        for k in ("linear_0/w", "linear_0/b", "linear_1/w", "linear_1/b", "linear_2/w"):
            assert (g[f"{tower}/{k}"] == 0.0).all(), (tower, k)
        assert (g[f"{tower}/linear_2/b"] != 0.0).any(), tower


def test_zero_gradient_leaves_parameters_alone():
    B, D = 33, CFG.obs_dim
    p = _params(CFG, 73)
    ring = _ring(CFG, 74, actions=[0, 1, 3, 4])  # action 2 never occurs
    dring = torch.as_tensor(ring).cuda()
    n = _native(CFG, B)
    n.set_params(p)
    for s in range(4):
        n.step(dring, torch.as_tensor(_idx(B, 80 + s)).cuda())
    torch.cuda.synchronize()
    assert n.num_steps == 4
    now, m, v = n.get_params("params"), n.get_params("m"), n.get_params("v")
    for tower in O.TOWERS:
        k = f"{tower}/linear_0/w"
        np.testing.assert_array_equal(now[k][D + 2].view(np.uint32), p[k][D + 2].view(np.uint32))
        assert (m[k][D + 2] == 0.0).all() and (v[k][D + 2] == 0.0).all(), tower
        assert (now[k][D + 1] != p[k][D + 1]).any(), tower  # a used action's row moved
