"""The prioritized replay table at the edges of its sampling mass, against the C oracle and
against references that do not share the oracle's arithmetic (tests/_oracle.py: the numpy tree
levels_from_leaves, numpy p**alpha for the distribution).  tests/test_replay_edges_cpu.py runs
the same inputs through the oracle alone.

  1. Degenerate masses (every priority zero: the uniform fallback; one live leaf at 1e-300 /
     1e300 in the last slot of the last partly filled node: the clamp to the last non-zero
     child; back to a mixed table; leaves 400 decades apart; NaN / negative updates; alpha 0
     and 1; a uniform table updated to 0), reached by inserts, by the one-launch update and by
     the multi-launch update, on every tree shape, wrapped and partly filled, and through
     every draw entry point.
  2. Leaf weights of the p grid of the CPU test: bit-equal to the oracle's.
  3. Stale-heavy updates (three keys in four evicted) at 64 and 256 update workgroups, and
     through the DQN step's rider.
  4. The distribution of 1M draws against numpy p**alpha.
  5. A pending pipe batch against every other writer of rows.

After every mutation check_tree compares the leaves, every stored level the readers read and
the sampling mass, bit for bit.
"""

import ctypes

import numpy as np
import pytest
import torch

from tests import _oracle as O
from tests._oracle import OracleTable, check_tree

pytestmark = pytest.mark.gpu

INFO = ("slots", "keys", "probabilities", "table_size", "priorities")


def _native(capacity, fields, prioritized=True, alpha=0.6, seed=1234):
    from acme_amd.native import NativeReplay
    return NativeReplay(capacity, fields, prioritized=prioritized, priority_exponent=alpha,
                        seed=seed)


def _dev_keys(keys):
    return torch.as_tensor(np.ascontiguousarray(keys, np.uint64).view(np.int64)).cuda() \
        .view(torch.uint64)


def _insert(r, o, prios):
    r.insert([np.zeros((len(prios), 1), np.int32)], prios)
    o.insert(prios)


def _update(r, o, keys, prios):
    r.update_priorities(_dev_keys(keys), torch.as_tensor(np.asarray(prios, np.float64)).cuda())
    o.update(keys, prios)


def _np(info, B=None):
    out = {k: info[k][:B].cpu().numpy() for k in INFO}
    out["keys"] = out["keys"].view(np.uint64)
    return out


def _assert_info(got, ref, scale=1.0, tag=""):
    """A GPU sample record against the oracle's, bit for bit (scale: a power of two)."""
    for k in INFO:
        want = ref[k] * scale if k == "probabilities" else ref[k]
        if got[k].dtype == np.float64:
            np.testing.assert_array_equal(got[k].view(np.uint64), want.view(np.uint64),
                                          err_msg=f"{tag} {k}")
        else:
            np.testing.assert_array_equal(got[k], want, err_msg=f"{tag} {k}")


def _draw(r, o, batch, step, tag=""):
    g = _np(r.sample(batch, step))
    _assert_info(g, o.sample(batch, step), tag=tag)
    return g


def _check_state(r, o, state, steps, tag):
    leaves = r.debug_state()["leaves"]
    total = O.native_total(r)
    for step in steps:
        O.assert_draw_state(_draw(r, o, 512, step, tag), leaves, total, r.size(), state)


# ------------------------------------------------------------------ 1. degenerate masses
def _walk_params():
    out = []
    for cap, wrapped in O.edge_shapes():
        for form in ("one", "multi"):
            for alpha in ((0.0, 0.6, 1.0) if cap < 100000 else (0.6,)):
                out.append((cap, wrapped, form, alpha))
    return out


@pytest.mark.parametrize("capacity,wrapped,form,alpha", _walk_params())
def test_update_walk(capacity, wrapped, form, alpha):
    """Mixed (leaves 10**±200) -> every priority zero -> one live leaf at 1e-300, then 1e300
    -> zero -> mixed (10**±12), each change by update calls of 512 / 4096 entries (form "one")
    or 5000 (form "multi"), most of whose entries are stale or never-issued keys."""
    r = _native(capacity, [4], alpha=alpha)
    o = OracleTable(capacity, True, alpha, 1234)
    for i, (op, args, state) in enumerate(O.edge_update_walk(capacity, wrapped, form)):
        if op == "insert":
            _insert(r, o, *args)
        else:
            _update(r, o, *args)
        tag = f"op {i} {op} -> {state}"
        check_tree(r, o, tag)
        if state is not None:
            _check_state(r, o, state, (i, 1000 + i), tag)


@pytest.mark.parametrize("alpha", [0.0, 0.6, 1.0])
@pytest.mark.parametrize("capacity,wrapped", O.edge_shapes())
def test_insert_walk(capacity, wrapped, alpha):
    """Every priority zero -> one live leaf in the last slot -> mixed, by host inserts."""
    r = _native(capacity, [4], alpha=alpha)
    o = OracleTable(capacity, True, alpha, 1234)
    for i, (prios, state) in enumerate(O.edge_insert_walk(capacity, wrapped)):
        _insert(r, o, prios)
        tag = f"insert {i} -> {state}"
        check_tree(r, o, tag)
        _check_state(r, o, state, (i,), tag)


def test_clamp_to_the_last_non_zero_child():
    """The constructed draw of _oracle.clamp_trap (test_replay_edges_cpu.py checks the
    construction): its residual target equals the selected node's whole mass, so the count of
    prefixes <= target is 64 and the clamp to the last non-zero child decides the slot.
    Random priorities reach this only when a target falls within an ulp of a prefix sum."""
    p, j, slot = O.clamp_trap()
    r = _native(256, [4], alpha=1.0, seed=O.CLAMP_TRAP_SEED)
    o = OracleTable(256, True, 1.0, O.CLAMP_TRAP_SEED)
    _insert(r, o, p)
    check_tree(r, o, "trap")
    g = _draw(r, o, 512, 0, "trap")
    assert g["slots"][j] == slot
    O.assert_draw_state(g, r.debug_state()["leaves"], O.native_total(r), 256, "mixed")
    keys = np.arange(256, dtype=np.uint64)  # the same leaves written by the update kernel
    _update(r, o, keys, p)
    check_tree(r, o, "trap, updated")
    assert _draw(r, o, 512, 0, "trap, updated")["slots"][j] == slot


@pytest.mark.parametrize("n_call", [O.ONE_LAUNCH_SMALL, O.MULTI_LAUNCH])
@pytest.mark.parametrize("capacity", [65, 4097])
def test_invalid_priorities_in_updates(capacity, n_call):
    """NaN, -1.0, -0.0 and -inf in an update: the weight is 0 and the raw priority is stored
    as given; with every live priority invalid the draw is the uniform fallback.  The host
    insert refuses NaN and negative priorities (-0.0 compares equal to zero: accepted, weight
    0) and leaves the table as it was."""
    rng = np.random.default_rng([capacity, n_call, 5])
    n = capacity + 10
    r = _native(capacity, [4])
    o = OracleTable(capacity, True, 0.6, 1234)
    _insert(r, o, rng.uniform(0.1, 2.0, n))
    bad = np.array([np.nan, -1.0, -0.0, -np.inf] * 2)
    keys = (n - capacity + rng.choice(capacity, len(bad), replace=False)).astype(np.uint64)
    _update(r, o, *O.update_call(rng, n_call, keys, bad, n, capacity))
    check_tree(r, o, "invalid")
    st = r.debug_state()
    slots = (keys % np.uint64(capacity)).astype(np.int64)
    np.testing.assert_array_equal(st["raw"][slots].view(np.uint64), bad.view(np.uint64))
    assert (st["leaves"][slots] == 0.0).all()
    g = _draw(r, o, 512, 1)
    assert not np.isin(g["slots"], slots).any()
    O.assert_draw_state(g, st["leaves"], O.native_total(r), capacity, "mixed")
    for p in (np.nan, -1.0, -np.inf):
        with pytest.raises(ValueError, match="must be >= 0"):
            r.insert([np.zeros((2, 1), np.int32)], np.array([1.0, p]))
    assert r.size() == capacity
    check_tree(r, o, "refused inserts")
    _draw(r, o, 512, 2)
    live = np.arange(n - capacity, n, dtype=np.uint64)
    for b in range(0, capacity, n_call):
        sel = live[b:b + n_call]
        _update(r, o, *O.update_call(rng, n_call, sel, np.resize(bad, len(sel)), n, capacity))
        check_tree(r, o, f"all invalid {b}")
    _check_state(r, o, "zero", (3, 4), "all invalid")
    _insert(r, o, np.array([-0.0, 2.0]))
    check_tree(r, o, "-0.0 inserted")
    _draw(r, o, 512, 5)


@pytest.mark.parametrize("n_call", [O.ONE_LAUNCH_SMALL, O.MULTI_LAUNCH])
def test_uniform_table_ignores_priorities(n_call):
    """Uniform(): priorities updated to 0 change neither the draws nor the probabilities."""
    rng = np.random.default_rng(n_call)
    cap, n = 1088, 1500
    r = _native(cap, [4], prioritized=False)
    o = OracleTable(cap, False, 0.0, 1234)
    _insert(r, o, np.ones(n))
    check_tree(r, o, "filled")
    before = _draw(r, o, 512, 7)
    keys = rng.integers(n - cap, n, 400).astype(np.uint64)
    _update(r, o, *O.update_call(rng, n_call, keys, np.zeros(400), n, cap))
    check_tree(r, o, "updated to 0")
    after = _draw(r, o, 512, 7)
    for k in ("slots", "keys", "probabilities", "table_size"):
        np.testing.assert_array_equal(before[k], after[k])
    assert (after["probabilities"] == 1.0 / cap).all()
    assert (after["priorities"] == 0.0).any()


# The transition layout of the entry-point test: o_tm1, a, r, d, o_t.
TRANSITION = [2048, 4, 4, 4, 2048]


def _buffers(r, B, fields):
    info = r.alloc_sample_info(B)
    for v in info.values():
        v.zero_()
    outs = [torch.zeros(B, b, dtype=torch.uint8, device="cuda") for b in fields]
    ptrs = (ctypes.c_void_p * len(outs))(*[x.data_ptr() for x in outs])
    raw = [info[k].data_ptr() for k in INFO]
    return info, outs, ptrs, raw


def _assert_rows(outs, data, index, tag=""):
    for f, x in enumerate(outs):
        np.testing.assert_array_equal(x[:len(index)].cpu().numpy(), data[f][index],
                                      err_msg=f"{tag} field {f}")


def test_every_draw_entry_point_at_degenerate_masses():
    """States (d) mixed 10**±200, (a) all zero and (b) one live leaf on a 4097-slot transition
    table.  In each state acme_replay_sample goes first (its slots asserted in [0, size)
    before any row is copied), then sample_gather, sample_gather_frames, sample_gather_pipe
    and sample_share (prob_scale 0.25: the scaled probability, in the fallback too): slots
    bit-equal to the oracle's, rows the rows of the reported keys."""
    from acme_amd._lib import lib
    L = lib()
    cap, B = 4097, 257
    n = O.edge_inserted(cap, True)
    rng = np.random.default_rng(11)
    data = [rng.integers(0, 256, (n, b), dtype=np.uint8) for b in TRANSITION]
    r = _native(cap, TRANSITION)
    o = OracleTable(cap, True, 0.6, 1234)
    pid = ctypes.c_int32()
    assert L.acme_replay_pipe_open(r.handle, ctypes.byref(pid)) == 0
    st = torch.cuda.Stream()
    step = 0
    for i, (op, args, state) in enumerate(O.edge_update_walk(cap, True, "one")):
        if op == "insert":
            r.insert(data, *args)
            o.insert(*args)
        else:
            _update(r, o, *args)
        check_tree(r, o, f"op {i}")
        if state is None:
            continue
        tag = f"op {i} {state}"
        step += 10
        g = _draw(r, o, B, step, tag)
        O.assert_draw_state(g, r.debug_state()["leaves"], O.native_total(r), cap, state)

        info, outs, ptrs, raw = _buffers(r, B, TRANSITION)
        assert L.acme_replay_sample_gather(r.handle, B, step + 1, *raw, ptrs, None) == 0
        torch.cuda.synchronize()
        g = _np(info)
        _assert_info(g, o.sample(B, step + 1), tag=tag + " sample_gather")
        _assert_rows(outs, data, g["keys"].astype(np.int64), tag + " sample_gather")

        info, outs, ptrs, raw = _buffers(r, B, TRANSITION)
        f16 = torch.zeros(2 * B, TRANSITION[0], dtype=torch.float16, device="cuda")
        assert L.acme_replay_sample_gather_frames(r.handle, B, step + 2, *raw, ptrs,
                                                  ctypes.c_void_p(f16.data_ptr()), None) == 0
        torch.cuda.synchronize()
        g = _np(info)
        k = g["keys"].astype(np.int64)
        _assert_info(g, o.sample(B, step + 2), tag=tag + " frames")
        _assert_rows(outs, data, k, tag + " frames")
        np.testing.assert_array_equal(f16[:B].cpu().numpy(), data[0][k].astype(np.float16))
        np.testing.assert_array_equal(f16[B:].cpu().numpy(), data[4][k].astype(np.float16))

        info, outs, ptrs, raw = _buffers(r, B, TRANSITION)
        with torch.cuda.stream(st):
            assert L.acme_replay_sample_gather_pipe(r.handle, pid.value, B, step + 3, *raw, ptrs,
                                                    ctypes.c_void_p(st.cuda_stream)) == 0
            assert L.acme_replay_pipe_flush(r.handle, pid.value) == 0
        torch.cuda.synchronize()
        g = _np(info)
        _assert_info(g, o.sample(B, step + 3), tag=tag + " pipe")
        _assert_rows(outs, data, g["keys"].astype(np.int64), tag + " pipe")

        info, outs, ptrs, raw = _buffers(r, B, TRANSITION)
        assert L.acme_replay_sample_share(r.handle, B, step + 4, 0.25, *raw, ptrs, None) == 0
        torch.cuda.synchronize()
        g = _np(info)
        _assert_info(g, o.sample(B, step + 4), scale=0.25, tag=tag + " share")
        _assert_rows(outs, data, g["keys"].astype(np.int64), tag + " share")
    assert L.acme_replay_pipe_close(r.handle, pid.value) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 2. leaf weights
@pytest.mark.parametrize("alpha", [0.3, 0.6, 0.9])
def test_leaf_weights_bit_equal_to_the_oracle(alpha):
    """The p grid of test_replay_edges_cpu.py::test_leaf_weight_against_longdouble, inserted
    (leaves computed on the host) and then written again by an update (on the device): both
    bit-equal to the oracle's, so the CPU test's bound holds for the kernel."""
    p = O.weight_grid()
    r = _native(len(p), [4], alpha=alpha)
    o = OracleTable(len(p), True, alpha, 1234)
    _insert(r, o, p)
    check_tree(r, o, "inserted")
    L = O.load()
    want = np.array([L.oracle_priority_weight(float(x), alpha) for x in p])
    np.testing.assert_array_equal(r.debug_state()["leaves"].view(np.uint64), want.view(np.uint64))
    keys = np.arange(len(p), dtype=np.uint64)
    _update(r, o, keys, p[::-1].copy())
    check_tree(r, o, "updated")
    np.testing.assert_array_equal(r.debug_state()["leaves"].view(np.uint64),
                                  want[::-1].view(np.uint64))
    _draw(r, o, 512, 0)


# ------------------------------------------------------------------ 3. stale-heavy updates
_stale_tables = {}


def _stale_table(capacity):
    """(table, oracle) of 4 * capacity inserted items, shared by the cases of one capacity:
    both always take the same calls."""
    if capacity not in _stale_tables:
        rng = np.random.default_rng(capacity)
        r = _native(capacity, [4])
        o = OracleTable(capacity, True, 0.6, 1234)
        _insert(r, o, rng.uniform(0.1, 2.0, 4 * capacity))
        check_tree(r, o, "filled")
        _stale_tables[capacity] = (r, o)
    return _stale_tables[capacity]


@pytest.mark.parametrize("n_upd,groups", O.STALE_CASES)
@pytest.mark.parametrize("capacity", [4097, 262145])
def test_stale_heavy_updates(capacity, n_upd, groups):
    """Three update keys in four were evicted.  They still join their workgroup's update and
    node lists: at 64 workgroups and 4096 updates on the four-level table every workgroup
    overflows its 32 prefetched (level, node) pairs and takes the read-back path; at 256
    workgroups and 512 updates none does.  A call of stale keys only leaves every level as it
    was; every other call has at least one live update in ten (asserted from the table's own
    keys), so the test cannot pass by updating nothing."""
    from acme_amd._lib import lib
    r, o = _stale_table(capacity)
    inserted = 4 * capacity
    lib().acme_tune_set(b"UPD_GROUPS", groups)
    try:
        for it, (kind, keys, prios) in enumerate(O.stale_heavy_calls(capacity, n_upd, groups)):
            stored = r.debug_state()["keys"]
            live = float((stored[(keys % np.uint64(capacity)).astype(np.int64)] == keys).mean())
            assert live == O.live_fraction(capacity, inserted, keys)
            before = r.debug_levels()
            _update(r, o, keys, prios)
            after = r.debug_levels()
            tag = f"{kind} {it}"
            if kind == "all_stale":
                assert live == 0.0
                for l, (x, y) in enumerate(zip(before, after)):
                    np.testing.assert_array_equal(x.view(np.uint64), y.view(np.uint64),
                                                  err_msg=f"{tag} level {l}")
            else:
                assert live >= 0.1, live
                assert not np.array_equal(before[0], after[0]), "no priority was written"
            check_tree(r, o, tag)
            _draw(r, o, 512, 100 * n_upd + 10 * groups + it, tag)
    finally:
        lib().acme_tune_set(b"UPD_GROUPS", 0)


def test_stale_heavy_rider():
    """The DQN step's write-back riding conv1's weight-gradient launch with three keys in four
    evicted and a repeated live key (B = 512, 4097 slots): equal to the separate launch, and
    the table equal to an oracle fed the step's own priorities."""
    from acme_amd.native import NativeReplay
    from acme_amd.networks import DQNAtariNetwork
    from tests import test_update_rider_gpu as R
    cap, B = 4097, 512
    inserted = 4 * cap
    a, b = R._pair(512)
    net = DQNAtariNetwork(R.A)
    p0, t0 = net.init(7), net.init(8)
    a.set_params(p0, t0)
    b.set_params(p0, t0)
    rng = np.random.default_rng(512)
    pr = rng.uniform(0.1, 2.0, inserted)
    rows = np.zeros((inserted, 1), np.int32)
    ta, tb = (NativeReplay(cap, [4], prioritized=True, priority_exponent=0.6, seed=77)
              for _ in range(2))
    o = OracleTable(cap, True, 0.6, 77)
    for t in (ta, tb):
        t.insert([rows], pr)
    o.insert(pr)
    rode = a.update_rider_launches()
    for step in range(2):
        k = rng.integers(0, inserted, B).astype(np.uint64)
        k[:9] = k[9] = inserted - 1 - step  # a repeated live key: the last entry wins
        assert 0.1 <= O.live_fraction(cap, inserted, k) <= 0.5
        keys = _dev_keys(k)
        dev = R._batch(rng, B)
        a.step(*dev, priority_update=(ta.handle, keys))
        b.step(*dev, priority_update=(tb.handle, keys))
        R._assert_same(a, b, ta, tb, B, ("stale", step))
        o.update(k, a.priorities[:B].cpu().numpy())
        check_tree(ta, o, f"rider step {step}")
        check_tree(tb, o, f"separate step {step}")
        _draw(ta, o, 512, 50 + step)
    assert a.update_rider_launches() == rode + 2, "the write-back did not ride conv1_wgrad"


# ------------------------------------------------------------------ 4. distribution
@pytest.mark.parametrize("capacity", O.CHI2_CAPACITIES)
def test_distribution_independent_of_the_tree(capacity):
    """256 draws of 4096 after an insert and one 4096-key update, priorities 10**uniform(-3, 3)
    with 30 % zeros: chi-square against numpy p**alpha (not the tree) below the p = 1e-4
    threshold, binned by level-1 node (bins expecting under 5 merged) and over the 64 heaviest
    slots plus the rest; no zero-weight slot is drawn.  The seeds are fixed, so the outcome is
    deterministic; the oracle's own draws of these inputs give (test_replay_edges_cpu.py):

      capacity   binned chi-square / dof (threshold)   heaviest chi-square / dof (threshold)
      69632      1034.9 / 1087 (1269.0)                87.0 / 64 (114.8)
      4097       41.4 / 63 (113.5)                     57.9 / 64 (114.8)
      65         0.28 / 1 (15.1)                       31.4 / 40 (82.1)
    """
    r = _native(capacity, [4], seed=O.CHI2_SEED)
    o = OracleTable(capacity, True, 0.6, O.CHI2_SEED)
    pr, keys, newp = O.chi2_inputs(capacity)
    _insert(r, o, pr)
    _update(r, o, keys, newp)
    check_tree(r, o, "updated")
    final = pr.copy()
    final[keys.astype(np.int64)] = newp
    counts = torch.zeros(capacity, dtype=torch.int64, device="cuda")
    info = r.alloc_sample_info(O.CHI2_BATCH)
    for step in range(O.CHI2_STEPS):
        counts += torch.bincount(r.sample(O.CHI2_BATCH, step, out=info)["slots"],
                                 minlength=capacity)
    stats = O.chi2_statistics(counts.cpu().numpy().astype(np.float64), final, 0.6)
    print(capacity, stats)
    assert "heaviest" in stats and (capacity < 100 or "binned" in stats)
    for name, (chi2, dof, threshold) in stats.items():
        assert chi2 < threshold, (name, chi2, dof, threshold)


# ------------------------------------------------------------------ 5. the pending pipe batch
PIPE_FIELDS = [2048, 4, 2048]


def _pipe_case(writer):
    # the n-step writer and the synthetic fill take transition tables only
    return TRANSITION if writer in ("nstep", "fill_synthetic") else PIPE_FIELDS


@pytest.mark.parametrize("writer", ["device_insert", "stage_commit", "nstep", "fill_synthetic",
                                    "export_import", "restore"])
def test_pending_pipe_batch_against_row_writers(writer):
    """A batch drawn on the pipe's stream whose rows are not copied yet, then every slot of
    the 3000-slot table overwritten through one of the other writers of rows (on another
    stream where it takes one): the pending batch holds the rows of its drawn keys (the data
    from before), its record equals the oracle's, the pipe's flush is then a no-op, and a
    fresh draw sees the new rows."""
    from acme_amd._lib import lib
    L = lib()
    fields = _pipe_case(writer)
    cap, B = 3000, 257
    rng = np.random.default_rng(len(writer))
    data = [rng.integers(0, 256, (cap, b), dtype=np.uint8) for b in fields]
    new = [rng.integers(0, 256, (cap, b), dtype=np.uint8) for b in fields]
    pr, newp = rng.uniform(0.0, 2.0, cap), rng.uniform(0.1, 1.0, cap)
    r = _native(cap, fields)
    o = OracleTable(cap, True, 0.6, 1234)
    r.insert(data, pr)
    o.insert(pr)
    check_tree(r, o, "filled")
    pid = ctypes.c_int32()
    assert L.acme_replay_pipe_open(r.handle, ctypes.byref(pid)) == 0
    st, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    sets = [_buffers(r, B, fields) for _ in range(2)]
    for k, step in enumerate((10, 11)):  # batch 10's rows ride batch 11's launch; 11 pends
        _, _, ptrs, raw = sets[k]
        assert L.acme_replay_sample_gather_pipe(r.handle, pid.value, B, step, *raw, ptrs,
                                                ctypes.c_void_p(st.cuda_stream)) == 0
    refs = [o.sample(B, 10), o.sample(B, 11)]

    key_base = cap  # a fresh draw's keys index `new` from here (None: rows not known here)
    if writer == "device_insert":
        with torch.cuda.stream(s2):
            dev = [torch.as_tensor(x).cuda() for x in new]
        s2.synchronize()
        r.insert(dev, newp, stream=s2)
        o.insert(newp)
    elif writer == "stage_commit":
        assert r.stage_capacity() >= cap
        for dst, src in zip(r.stage(cap), new):
            dst[:] = src
        r.commit(cap, newp, stream=s2)
        o.insert(newp)
    elif writer == "nstep":
        # n = 1: item k is (obs[k], act[k], rew[k], disc[k], obs[k + 1]); 3000 adds wrap the ring
        obs = rng.integers(0, 256, (cap + 1, fields[0]), dtype=np.uint8)
        act = rng.integers(0, 18, cap).astype(np.int32)
        rew = rng.standard_normal(cap).astype(np.float32)
        disc = rng.uniform(0.5, 1.0, cap).astype(np.float32)
        w = r.nstep_writer(1, 0.99, fields[0], 4, rows_per_chunk=64)
        w.start(obs[0].ctypes.data)
        for k in range(cap):
            w.add_raw(act[k:].ctypes.data, float(rew[k]), float(disc[k]), obs[k + 1].ctypes.data,
                      False, float(newp[k]))
        w.flush()
        assert w.pending() == 0
        o.insert(newp)
        new = [obs[:-1], act.view(np.uint8).reshape(cap, 4), rew.view(np.uint8).reshape(cap, 4),
               disc.view(np.uint8).reshape(cap, 4), obs[1:]]
    elif writer == "fill_synthetic":
        r.fill_synthetic(cap, 0, num_actions=18, seed=5, stream=s2)
        o.insert(np.ones(cap))
        key_base = None
    elif writer == "restore":
        # acme_replay_restore on its own (new raw priorities, the rows as they are): it issues
        # the pending copy itself, not through acme_replay_storage
        from acme_amd.native import _memcpy_htod
        rp = ctypes.c_void_p()
        assert L.acme_replay_debug_leaves(r.handle, None, ctypes.byref(rp), None) == 0
        _memcpy_htod(rp.value, newp)
        assert L.acme_replay_restore(r.handle, cap, None) == 0
        o = OracleTable(cap, True, 0.6, 1234)
        o.insert(newp)
        new, key_base = data, 0
    else:
        state = r.export_state()  # acme_replay_storage: issues the pending copy and waits
        for f in range(len(fields)):
            np.testing.assert_array_equal(state[f"field_{f}"], data[f])
        for f in range(len(fields)):
            state[f"field_{f}"] = new[f]
        state["raw_priorities"] = newp
        r.import_state(state)  # acme_replay_restore
        o = OracleTable(cap, True, 0.6, 1234)
        o.insert(newp)
        key_base = 0
    torch.cuda.synchronize()
    r.sync_inserts()

    for k in range(2):  # the batches drawn before the overwrite: the old rows
        info, outs = sets[k][0], sets[k][1]
        g = _np(info)
        _assert_info(g, refs[k], tag=f"{writer} batch {k}")
        _assert_rows(outs, data, g["keys"].astype(np.int64), f"{writer} batch {k}")
    held = [x.clone() for x in sets[1][1]]
    assert L.acme_replay_pipe_flush(r.handle, pid.value) == 0  # nothing pending: no-op
    torch.cuda.synchronize()
    for x, y in zip(held, sets[1][1]):
        assert torch.equal(x, y)
    check_tree(r, o, writer)

    info, outs, ptrs, raw = _buffers(r, B, fields)  # a fresh draw: the new rows
    assert L.acme_replay_sample_gather(r.handle, B, 12, *raw, ptrs, None) == 0
    torch.cuda.synchronize()
    g = _np(info)
    _assert_info(g, o.sample(B, 12), tag=f"{writer} fresh")
    if key_base is None:  # the synthetic rows, as the table's storage holds them
        new = [r.export_state()[f"field_{f}"] for f in range(len(fields))]
        index = g["slots"]
        assert not np.array_equal(new[0], data[0])
    else:
        index = g["keys"].astype(np.int64) - key_base
    _assert_rows(outs, new, index, f"{writer} fresh")
    assert L.acme_replay_pipe_close(r.handle, pid.value) == 0
    torch.cuda.synchronize()
