"""The DQN step's priority write-back as the leading workgroups of conv1's weight-gradient
launch (csrc/prio_update.h UpdateRider, gemm_p3.h gemm_p3r_kernel) against the separate
launch after it (a learner created with ACME_V_UPDATE_RIDER=0): the same update body, so
every result is compared bit for bit.

  * test_rider_equals_separate_launch: B = 1, 37, 512 on tables of 64, 65 and 4097 slots (1, 2
    and 3 tree levels), three steps of which one copies the target, each batch with a
    repeated key (the last update wins) and a key evicted since the draw.
  * test_batch_above_rider_capacity_falls_back: a learner with max_batch = 513 rides at
    B = 512 and takes the separate launch for a 513-row batch.
  * test_skipped_step_writes_no_priority_under_rider: a step skipped by the end-of-step
    rescale (as test_step_guard_gpu.py forces it) writes no priority from the rider's
    workgroups, and the same batch issued again ends identical.
  * test_update_body_workgroup_counts: the moved body through its own kernel
    (prio_update_fused_kernel) at 64, 128 and 256 update workgroups against the C oracle.

Compared in every learner case: parameters, target, Adam moments, loss, the step's
priorities, the table's raw priorities, every stored tree level and the next draw.
"""

import numpy as np
import pytest
import torch

from tests._oracle import OracleTable

pytestmark = pytest.mark.gpu

A = 18
HEAD = ("duelling_q_network/mlp/linear_1/w", "duelling_q_network/mlp_1/linear_1/w")
_pairs = {}


def _make(max_batch, rider, **kw):
    from acme_amd._lib import lib
    from acme_amd.native import NativeDQN
    lib().acme_tune_set(b"UPDATE_RIDER", 1 if rider else 0)  # read once, at creation
    try:
        return NativeDQN(network="nature", num_actions=A, max_batch=max_batch, obs_dtype="uint8",
                         **kw)
    finally:
        lib().acme_tune_set(b"UPDATE_RIDER", 1)  # the shipped default


def _pair(max_batch):
    """(rider learner, separate-launch learner), shared by the cases of one max_batch: both
    always take the same calls, so they stay comparable from case to case."""
    if max_batch not in _pairs:
        _pairs[max_batch] = (_make(max_batch, True, target_update_period=3),
                             _make(max_batch, False, target_update_period=3))
    return _pairs[max_batch]


def _batch(rng, B, r=None, d=None):
    o1 = rng.integers(0, 256, (B, 84, 84, 4), dtype=np.uint8)
    o2 = rng.integers(0, 256, (B, 84, 84, 4), dtype=np.uint8)
    rr = (rng.standard_normal(B) * 1.5).astype(np.float32) if r is None else np.full(B, r, np.float32)
    dd = (np.where(rng.random(B) < 0.2, 0.0, 0.99 ** 4).astype(np.float32) if d is None
          else np.full(B, d, np.float32))
    vals = (o1, rng.integers(0, A, B).astype(np.int32), rr, dd, o2, rng.uniform(1e-6, 1e-3, B))
    return [torch.as_tensor(v).cuda().contiguous() for v in vals]


def _tables(capacity, extra=10):
    """Two identical prioritized tables that have wrapped: keys [0, extra) are evicted."""
    from acme_amd.native import NativeReplay
    n = capacity + extra
    rows = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)
    tables = [NativeReplay(capacity, [4], prioritized=True, priority_exponent=0.6, seed=77)
              for _ in range(2)]
    for t in tables:
        t.insert([rows], np.linspace(0.5, 2.0, n))
    torch.cuda.synchronize()
    return tables


def _keys(tables, B, step):
    keys = tables[0].sample(B, step)["keys"]
    assert torch.equal(keys, tables[1].sample(B, step)["keys"])
    k = keys.cpu().numpy().view(np.uint64).copy()
    if B >= 8:
        k[:3] = k[3]  # a repeated key: the update with the largest index wins
        k[5] = 2      # evicted since the draw: ignored
    return torch.as_tensor(k.view(np.int64)).cuda().view(torch.uint64)


def _assert_same(a, b, ta, tb, B, tag):
    torch.cuda.synchronize()
    assert a.loss.item() == b.loss.item(), tag
    assert torch.equal(a.priorities[:B], b.priorities[:B]), tag
    for buf in ("params", "target", "m", "v"):
        ga, gb = a.get_params(buf), b.get_params(buf)
        for k in ga:
            np.testing.assert_array_equal(ga[k], gb[k], err_msg=f"{tag} {buf}/{k}")
    np.testing.assert_array_equal(ta.debug_state()["raw"], tb.debug_state()["raw"], err_msg=str(tag))
    la, lb = ta.debug_levels(), tb.debug_levels()
    assert len(la) == len(lb)
    for i, (x, y) in enumerate(zip(la, lb)):
        np.testing.assert_array_equal(x, y, err_msg=f"{tag} level {i}")


def _assert_same_draw(ta, tb, B, step):
    da, db = ta.sample(B, step), tb.sample(B, step)
    for k in da:
        assert torch.equal(da[k], db[k]), k


@pytest.mark.parametrize("capacity,levels", [(64, 1), (65, 2), (4097, 3)])
@pytest.mark.parametrize("B", [1, 37, 512])
def test_rider_equals_separate_launch(B, capacity, levels):
    from acme_amd.networks import DQNAtariNetwork
    a, b = _pair(512)
    net = DQNAtariNetwork(A)
    p0, t0 = net.init(3), net.init(4)
    a.set_params(p0, t0)
    b.set_params(p0, t0)
    ta, tb = _tables(capacity)
    assert len(ta.debug_levels()) == levels
    rng = np.random.default_rng(1000 * B + capacity)
    rode, sep = a.update_rider_launches(), b.update_rider_launches()
    raw0 = ta.debug_state()["raw"].copy()
    for step in range(3):  # the learners' step counts differ from case to case: a target
        keys = _keys((ta, tb), B, step)  # copy falls on one of any three consecutive steps
        dev = _batch(rng, B)
        a.step(*dev, priority_update=(ta.handle, keys))
        b.step(*dev, priority_update=(tb.handle, keys))
        _assert_same(a, b, ta, tb, B, (B, capacity, step))
    assert a.update_rider_launches() == rode + 3, "the write-back did not ride conv1_wgrad"
    assert b.update_rider_launches() == sep == 0
    assert not np.array_equal(ta.debug_state()["raw"], raw0), "no priority was written"
    _assert_same_draw(ta, tb, max(B, 64), 99)


def test_batch_above_rider_capacity_falls_back():
    from acme_amd.networks import DQNAtariNetwork
    a, b = _pair(513)
    net = DQNAtariNetwork(A)
    p0, t0 = net.init(5), net.init(6)
    a.set_params(p0, t0)
    b.set_params(p0, t0)
    ta, tb = _tables(4097)
    rng = np.random.default_rng(513)
    for step, (B, rides) in enumerate([(512, 1), (513, 0), (512, 1)]):
        before = a.update_rider_launches()
        keys = _keys((ta, tb), B, step)
        dev = _batch(rng, B)
        a.step(*dev, priority_update=(ta.handle, keys))
        b.step(*dev, priority_update=(tb.handle, keys))
        _assert_same(a, b, ta, tb, B, (B, step))
        assert a.update_rider_launches() == before + rides, (B, step)
    assert b.update_rider_launches() == 0
    _assert_same_draw(ta, tb, 512, 99)


def test_skipped_step_writes_no_priority_under_rider():
    """|TD| ~ 1 then |TD| ~ 1e-4 (a head scaled down by 1e-4, r = d = 0): the second step's
    head dZ shrinks ~2^13-fold, the rescale workgroup (the rider's first) decides the skip
    and the rider's update workgroups write nothing.  The same batch again is applied."""
    from acme_amd.networks import DQNAtariNetwork
    B = 64
    net = DQNAtariNetwork(A)
    p0, t0 = net.init(1), net.init(2)
    for k in HEAD:
        p0[k] = p0[k] * 1e-4
        t0[k] = t0[k] * 1e-4
    a = _make(B, True, learning_rate=1e-7)
    b = _make(B, False, learning_rate=1e-7)
    a.set_params(p0, t0)
    b.set_params(p0, t0)
    ta, tb = _tables(4097)
    rng = np.random.default_rng(4)
    large, small = _batch(rng, B, r=1.0, d=0.0), _batch(rng, B, r=0.0, d=0.0)
    keys = [_keys((ta, tb), B, s) for s in range(3)]
    a.step(*large, priority_update=(ta.handle, keys[0]))
    b.step(*large, priority_update=(tb.handle, keys[0]))
    _assert_same(a, b, ta, tb, B, "applied")
    assert a.guard_state()["applied"] == 1
    raw1 = ta.debug_state()["raw"].copy()
    state1 = {buf: a.get_params(buf) for buf in ("params", "m", "v")}
    a.step(*small, priority_update=(ta.handle, keys[1]))
    b.step(*small, priority_update=(tb.handle, keys[1]))
    for d in (a, b):
        g = d.guard_state()
        assert g["skipped"] == 1 and g["last_skipped"] == 1 and g["verdict_timeouts"] == 0, g
    np.testing.assert_array_equal(ta.debug_state()["raw"], raw1)
    for buf, ref in state1.items():
        got = a.get_params(buf)
        for k in ref:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{buf}/{k}")
    _assert_same(a, b, ta, tb, B, "skipped")
    a.step(*small, priority_update=(ta.handle, keys[1]))  # issued again: applied
    b.step(*small, priority_update=(tb.handle, keys[1]))
    for d in (a, b):
        g = d.guard_state()
        assert g["applied"] == 2 and g["skipped"] == 1 and g["last_skipped"] == 0, g
    assert not np.array_equal(ta.debug_state()["raw"], raw1)
    _assert_same(a, b, ta, tb, B, "issued again")
    assert a.update_rider_launches() == 3 and b.update_rider_launches() == 0
    _assert_same_draw(ta, tb, B, 99)


@pytest.mark.parametrize("n_upd", [512, 4096])
@pytest.mark.parametrize("groups", [64, 128, 256])
def test_update_body_workgroup_counts(groups, n_upd):
    """Four-level tree: the partition over the update workgroups decides who computes a node,
    never its value.  At 64 workgroups and 4096 updates every workgroup has more (level, node)
    pairs than it prefetches: the read-back path."""
    from acme_amd._lib import lib
    from acme_amd.native import NativeReplay
    rng = np.random.default_rng(n_upd + groups)
    cap = 300_000
    r = NativeReplay(cap, [4], prioritized=True, priority_exponent=0.6, seed=1234)
    o = OracleTable(cap, True, 0.6, 1234)
    pr = rng.uniform(0.1, 2.0, cap + 1000)
    r.insert([np.zeros((cap + 1000, 1), np.int32)], pr)
    o.insert(pr)
    lib().acme_tune_set(b"UPD_GROUPS", groups)
    try:
        for it in range(2):
            keys = rng.integers(1000, cap + 1000, n_upd).astype(np.uint64)
            keys[:16] = keys[16]  # duplicates: the last one wins
            keys[17] = 3          # evicted key: ignored
            newp = rng.uniform(0.0, 3.0, n_upd)
            r.update_priorities(torch.as_tensor(keys.view(np.int64)).cuda().view(torch.uint64),
                                torch.as_tensor(newp).cuda())
            o.update(keys, newp)
            np.testing.assert_array_equal(r.debug_state()["leaves"], o.leaves()[:cap])
            g = {k: v.cpu().numpy() for k, v in r.sample(512, 200 + it).items()}
            ref = o.sample(512, 200 + it)
            np.testing.assert_array_equal(g["slots"], ref["slots"])
            np.testing.assert_array_equal(g["keys"].view(np.uint64), ref["keys"])
            np.testing.assert_array_equal(g["probabilities"], ref["probabilities"])
            np.testing.assert_array_equal(g["priorities"], ref["priorities"])
    finally:
        lib().acme_tune_set(b"UPD_GROUPS", 0)
