"""Builds and binds the C replay oracle (oracle/replay_oracle.c) — test infrastructure."""

import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "oracle", "replay_oracle.c")
OUT = os.path.join(ROOT, "oracle", "build", "libreplay_oracle.so")

_L = None


def build() -> str:
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < os.path.getmtime(SRC):
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall",
                               "-o", OUT, SRC, "-lm"])
    return OUT


def load():
    global _L
    if _L is None:
        if not os.path.exists(OUT):
            build()
        L = ctypes.CDLL(OUT)
        vp, i64, u64, f64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
        L.oracle_philox4x32_10.argtypes = [vp, vp, vp]
        L.oracle_uniform.restype = f64
        L.oracle_uniform.argtypes = [u64, u64, ctypes.c_uint32]
        L.oracle_log.restype = f64
        L.oracle_log.argtypes = [f64]
        L.oracle_exp.restype = f64
        L.oracle_exp.argtypes = [f64]
        L.oracle_priority_weight.restype = f64
        L.oracle_priority_weight.argtypes = [f64, f64]
        L.oracle_table_new.restype = vp
        L.oracle_table_new.argtypes = [i64, ctypes.c_int, f64, u64]
        L.oracle_table_free.argtypes = [vp]
        L.oracle_table_insert.restype = i64
        L.oracle_table_insert.argtypes = [vp, i64, vp]
        L.oracle_table_update.argtypes = [vp, i64, vp, vp]
        L.oracle_table_sample.restype = ctypes.c_int
        L.oracle_table_sample.argtypes = [vp, i64, u64, vp, vp, vp, vp, vp]
        L.oracle_table_size.restype = i64
        L.oracle_table_size.argtypes = [vp]
        L.oracle_table_leaves.restype = ctypes.POINTER(ctypes.c_double)
        L.oracle_table_leaves.argtypes = [vp]
        L.oracle_table_total.restype = f64
        L.oracle_table_total.argtypes = [vp]
        _L = L
    return _L


def philox(ctr, key):
    L = load()
    c = np.asarray(ctr, np.uint32)
    k = np.asarray(key, np.uint32)
    o = np.zeros(4, np.uint32)
    L.oracle_philox4x32_10(c.ctypes.data, k.ctypes.data, o.ctypes.data)
    return o


class OracleTable:
    def __init__(self, capacity, prioritized, alpha, seed):
        self.L = load()
        self.capacity = capacity
        self.h = self.L.oracle_table_new(capacity, 1 if prioritized else 0, alpha, seed)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.oracle_table_free(self.h)
            self.h = None

    def insert(self, priorities):
        p = np.ascontiguousarray(priorities, np.float64)
        return self.L.oracle_table_insert(self.h, len(p), p.ctypes.data)

    def update(self, keys, priorities):
        k = np.ascontiguousarray(keys, np.uint64)
        p = np.ascontiguousarray(priorities, np.float64)
        self.L.oracle_table_update(self.h, len(k), k.ctypes.data, p.ctypes.data)

    def sample(self, batch, step):
        out = dict(slots=np.empty(batch, np.int64), keys=np.empty(batch, np.uint64),
                   probabilities=np.empty(batch, np.float64),
                   table_size=np.empty(batch, np.int64), priorities=np.empty(batch, np.float64))
        rc = self.L.oracle_table_sample(self.h, batch, step, out["slots"].ctypes.data,
                                        out["keys"].ctypes.data, out["probabilities"].ctypes.data,
                                        out["table_size"].ctypes.data,
                                        out["priorities"].ctypes.data)
        if rc != 0:
            raise RuntimeError("oracle: empty table")
        return out

    def leaves(self):
        p = self.L.oracle_table_leaves(self.h)
        n = ((self.capacity + 63) // 64) * 64
        return np.ctypeslib.as_array(p, shape=(n,)).copy()

    def total(self):
        return self.L.oracle_table_total(self.h)


# ------------------------------------------------------------------ the stored tree, in numpy
def scan64(rows):
    """The inclusive Hillis-Steele scan of each row of a [n, 64] array, the additions in the
    scan's fixed order (round d = 1, 2, ..., 32: x[i] = x[i - d] + x[i] for i >= d, from the
    values before the round)."""
    x = np.array(rows, np.float64)
    d = 1
    while d < 64:
        y = x.copy()
        y[:, d:] = x[:, :-d] + x[:, d:]
        x = y
        d *= 2
    return x


def _scan_totals(rows):
    return scan64(rows)[:, 63].copy()


def _pad64(v):
    v = np.asarray(v, np.float64).ravel()
    out = np.zeros(-(-max(len(v), 1) // 64) * 64)
    out[:len(v)] = v
    return out


def levels_from_leaves(leaves):
    """(levels, total) of the 64-ary sum tree over `leaves`, restated in numpy without the C
    oracle: level 0 is the leaves padded with zeros to a multiple of 64; level l + 1 holds the
    scan total of each 64 entries of level l, padded likewise; the last level has exactly 64
    entries, and the total is that row's scan total."""
    with np.errstate(over="ignore", invalid="ignore"):
        levels = [_pad64(leaves)]
        while len(levels[-1]) > 64:
            levels.append(_pad64(_scan_totals(levels[-1].reshape(-1, 64))))
        return levels, float(_scan_totals(levels[-1].reshape(1, 64))[0])


def computed_top(level_sizes):
    """True when the table's readers compute the top level from the level below (at most 16
    of its nodes have children) and the one-launch update leaves the stored top alone."""
    return len(level_sizes) >= 2 and level_sizes[-2] // 64 <= 16


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_oracle_tree(oracle):
    """The C oracle's total against the numpy restatement of the tree over its leaves."""
    levels, total = levels_from_leaves(oracle.leaves())
    assert _bits(total) == _bits(oracle.total()), (total, oracle.total())
    return levels, total


def native_total(native):
    """acme_replay_total of a NativeReplay: the sampling mass as its readers compute it."""
    import ctypes

    import torch
    from acme_amd._lib import lib
    out = torch.zeros(1, dtype=torch.float64, device=native.device)
    assert lib().acme_replay_total(native.handle, ctypes.c_void_p(out.data_ptr()), None) == 0
    torch.cuda.synchronize(native.device)
    return out.item()


def check_tree(native, oracle, tag=""):
    """After a mutation: the GPU table's leaves, every stored level its readers read and its
    sampling mass equal, bit for bit, the oracle's leaves, their numpy tree and the oracle's
    total; and the numpy tree ends in the oracle's total (no GPU involved)."""
    cap = native.capacity
    ref_leaves = oracle.leaves()
    np.testing.assert_array_equal(_bits(native.debug_state()["leaves"]), _bits(ref_leaves[:cap]),
                                  err_msg=f"{tag} leaves")
    ref_levels, _ = check_oracle_tree(oracle)
    got = native.debug_levels()
    assert [len(x) for x in got] == [len(x) for x in ref_levels], tag
    skip_top = computed_top([len(x) for x in got])
    for l, (g, ref) in enumerate(zip(got, ref_levels)):
        if skip_top and l == len(got) - 1:
            continue  # not maintained by the one-launch update: only the total is asserted
        np.testing.assert_array_equal(_bits(g), _bits(ref), err_msg=f"{tag} level {l}")
    total = native_total(native)
    if native.prioritized:
        assert _bits(total) == _bits(oracle.total()), (tag, total, oracle.total())
    else:  # Uniform(): the mass is the item count
        assert total == float(native.size()), (tag, total, native.size())


# ------------------------------------------------------------------ degenerate-mass inputs
# Shared by tests/test_replay_edges_cpu.py (the oracle alone) and tests/test_replay_edges_gpu.py
# (the GPU table against it): every input below is a pure function of its arguments.
#
# The smallest capacities that reach each tree shape (stored levels of 64-entry rows):
#   1        a single slot                      64       one full level
#   65       two levels, 2 nodes, computed top  1088     two levels, 17 nodes: the stored top
#   4097     three levels, computed top         262145   four levels
EDGE_CAPACITIES = (1, 64, 65, 1088, 4097, 262145)
ONE_LAUNCH_SMALL, ONE_LAUNCH_MAX, MULTI_LAUNCH = 512, 4096, 5000


def edge_inserted(capacity, wrapped):
    """Items inserted first: more than the capacity (the ring wrapped) or fewer (partly
    filled, the last live node partly filled too).  A single slot has no partly filled state."""
    if wrapped:
        return capacity + max(1, min(capacity // 2, 1000))
    return capacity - capacity // 3 - 1


def edge_shapes():
    return [(c, w) for c in EDGE_CAPACITIES for w in (True, False) if edge_inserted(c, w) > 0]


def wide_priorities(rng, n, decades):
    """10**uniform(-decades, decades) with 30-50 % exact zeros; the last one (live in every
    table, a single slot included) stays positive."""
    p = 10.0 ** rng.uniform(-decades, decades, n)
    p[:-1][rng.random(n - 1) < rng.uniform(0.3, 0.5)] = 0.0
    return p


def last_slot_key(capacity, inserted):
    """(slot, key) of the last slot of the last partly filled node: the last live slot."""
    size = min(inserted, capacity)
    slot = size - 1
    key = inserted - 1 - (inserted - 1 - slot) % capacity
    assert key % capacity == slot and inserted - size <= key < inserted
    return slot, key


def update_call(rng, n_call, keys, prios, inserted, capacity):
    """One update call of exactly n_call entries that applies (keys, prios) in order: the
    entries are spread over the call in order, and the rest are keys that update nothing
    (never issued, and evicted ones where the ring wrapped) with positive priorities."""
    keys = np.asarray(keys, np.uint64)
    assert 0 < len(keys) <= n_call
    k = (inserted + rng.integers(0, 4 * capacity + 64, n_call)).astype(np.uint64)
    if inserted > capacity:
        ev = rng.random(n_call) < 0.5
        k[ev] = rng.integers(0, inserted - capacity, int(ev.sum())).astype(np.uint64)
    p = 10.0 ** rng.uniform(-3, 3, n_call)
    at = np.sort(rng.choice(n_call, len(keys), replace=False))
    k[at] = keys
    p[at] = prios
    return k, p


def edge_update_walk(capacity, wrapped, form):
    """The states of issue section 1 reached by priority updates.  Yields (op, args, state):
    op "insert" (priorities) or "update" (keys, priorities); state, where the table is in one
    after the op, "zero" (every priority zero), ("single", slot) (one positive leaf, in the
    last slot of the last partly filled node) or "mixed"; None mid-way through a bulk change.
    form "one": calls of 512 (single-key changes) and up to 4096 entries (bulk), the one-launch
    update; form "multi": calls of 5000 entries, the multi-launch path."""
    rng = np.random.default_rng([capacity, int(wrapped), 0 if form == "one" else 1])
    n = edge_inserted(capacity, wrapped)
    size = min(n, capacity)
    live = np.arange(n - size, n, dtype=np.uint64)
    n_single = ONE_LAUNCH_SMALL if form == "one" else MULTI_LAUNCH
    n_bulk = ONE_LAUNCH_MAX if form == "one" else MULTI_LAUNCH

    def bulk(prios, end_state):
        order = rng.permutation(size)
        for b in range(0, size, n_bulk):
            sel = order[b:b + n_bulk]
            yield ("update", update_call(rng, n_bulk, live[sel], prios[sel], n, capacity),
                   end_state if b + n_bulk >= size else None)

    yield "insert", (wide_priorities(rng, n, 200),), "mixed"
    yield from bulk(np.zeros(size), "zero")
    slot, key = last_slot_key(capacity, n)
    for p in (1e-300, 1e300):
        # the same key three times in one call: the last entry wins
        yield ("update", update_call(rng, n_single, [key] * 3, [7.0, 0.0, p], n, capacity),
               ("single", slot))
    yield "update", update_call(rng, n_single, [key], [0.0], n, capacity), "zero"
    yield from bulk(wide_priorities(rng, size, 12), "mixed")


def edge_insert_walk(capacity, wrapped):
    """The same states reached by inserts alone: (priorities, state) per insert."""
    rng = np.random.default_rng([capacity, int(wrapped), 2])
    n = edge_inserted(capacity, wrapped)
    yield np.zeros(n), "zero"
    # up to the last slot: of the ring where it wrapped, else three more items
    m = capacity - n % capacity if wrapped else min(3, capacity - n - 1)
    p = np.zeros(m)
    p[-1] = 1e300 if wrapped else 1e-300
    n += m
    yield p, ("single", last_slot_key(capacity, n)[0])
    m = capacity // 2 + 1 if wrapped else capacity - n - 1
    if m > 0:
        yield wide_priorities(rng, m, 200), "mixed"


CLAMP_TRAP_SEED = 1234


def clamp_trap(batch=512, step=0):
    """(priorities of a 256-slot alpha = 1 table, draw index j, slot): draw j of that step
    reaches a child with a residual target equal to the child's whole mass, where only the
    clamp to the last non-zero child keeps the descent on a live leaf.

    Node totals 1, 2**-53, 2**-52 (one leaf, in place 5 of node 2) and R.  In the top row the
    scan gives s[1] = fl(1 + 2**-53) = 1 (the tie rounds to even) but s[2] =
    fl(1 + fl(2**-53 + 2**-52)) = 1 + 2**-51 (the tie rounds up), so t = 1 + 2**-52 selects
    node 2 with the residual t - s[1] = 2**-52: every prefix of node 2's row is <= it, and the
    count of such prefixes is 64.  R is chosen for draw j's known uniform u so that
    fl(u * total) is exactly that t."""
    L = load()
    ulp = 2.0 ** -52
    for j in range(batch):
        u = L.oracle_uniform(CLAMP_TRAP_SEED, step, j)
        if not 0.5 < u < 1.0:
            continue
        k0 = int(((1.0 + ulp) / u - 1.0) / ulp)
        for k in range(max(k0 - 4, 2), k0 + 5):
            if u * (1.0 + k * ulp) == 1.0 + ulp:
                p = np.zeros(256)
                p[0], p[64], p[128 + 5], p[192] = 1.0, ulp / 2, ulp, (k - 1) * ulp
                return p, j, 128 + 5
    raise AssertionError("no draw of this step has a usable uniform")


def assert_draw_state(sample, leaves, total, size, state):
    """What a draw (the dict of OracleTable.sample, or a GPU draw in numpy) must satisfy in a
    given state of the table, from the leaves and the total alone."""
    slots, probs = sample["slots"], sample["probabilities"]
    assert ((slots >= 0) & (slots < size)).all(), (slots.min(), slots.max(), size)
    assert (sample["table_size"] == size).all()
    if state == "zero":  # the uniform fallback over the live items, not the capacity
        assert total == 0.0
        assert (probs == 1.0 / size).all()
        if size > 1 and len(slots) >= 64:
            assert len(np.unique(slots)) > 1
    elif state == "mixed":
        assert np.isfinite(total) and total > 0.0
        assert (leaves[slots] > 0.0).all(), "a zero-weight slot was drawn"
        np.testing.assert_array_equal(probs, leaves[slots] / total)
    else:
        _, slot = state
        assert leaves[slot] > 0.0 and total == leaves[slot]
        assert (slots == slot).all(), np.unique(slots)
        assert (probs == 1.0).all()


def weight_grid():
    """p = 10**k over k in [-300, 300], the smallest normal, the largest finite, a subnormal."""
    p = [10.0 ** k for k in range(-300, 301)]
    return np.array(p + [np.finfo(np.float64).tiny, np.finfo(np.float64).max, 5e-321])


# ------------------------------------------------------------------ stale-heavy update calls
def live_fraction(capacity, inserted, keys):
    """Fraction of update keys the FIFO ring still holds: those in [inserted - capacity, inserted)."""
    k = np.asarray(keys, np.uint64).astype(np.float64)
    return float(((k >= inserted - capacity) & (k < inserted)).mean())


# (updates per call, update workgroups; 0: the multi-launch path, which has none)
STALE_CASES = ((512, 64), (512, 256), (4096, 64), (4096, 256), (5000, 0))


def stale_heavy_calls(capacity, n_upd, groups):
    """Update calls of n_upd entries against a table of 4 * capacity inserted items, so a key
    drawn uniformly from [0, inserted) is stale three times in four.  Yields (kind, keys,
    priorities).  Every "mixed" call also holds a live key followed by the evicted key of the
    same slot (key - capacity: it must not win), 16 repeats of one live key (the last wins)
    and a key that was never issued; the "all_stale" call holds no live key at all."""
    rng = np.random.default_rng([capacity, n_upd, groups, 3])
    inserted = 4 * capacity
    for kind in ("mixed", "mixed", "all_stale", "mixed"):
        prios = rng.uniform(0.0, 3.0, n_upd)
        if kind == "all_stale":
            keys = rng.integers(0, inserted - capacity, n_upd).astype(np.uint64)
            keys[::7] = (inserted + rng.integers(0, capacity, len(keys[::7]))).astype(np.uint64)
        else:
            keys = rng.integers(0, inserted, n_upd).astype(np.uint64)
            live = rng.integers(inserted - capacity, inserted, 3).astype(np.uint64)
            keys[40], keys[41] = live[0], live[0] - np.uint64(capacity)
            keys[300], keys[100] = live[1], live[1] - np.uint64(2 * capacity)
            keys[200:216] = live[2]
            keys[-1] = inserted + 5
        yield kind, keys, prios


# ------------------------------------------------------------------ distribution statistics
CHI2_CAPACITIES = (65, 4097, 69632)
CHI2_SEED, CHI2_STEPS, CHI2_BATCH = 99, 256, 4096


def chi2_inputs(capacity):
    """(insert priorities, update keys, update priorities): 10**uniform(-3, 3) with 30 %
    zeros, inserted once (no wrap), then one update of min(4096, capacity) distinct keys."""
    rng = np.random.default_rng([capacity, 4])

    def draw(n):
        p = 10.0 ** rng.uniform(-3, 3, n)
        p[rng.random(n) < 0.3] = 0.0
        return p
    pr = draw(capacity)
    keys = rng.choice(capacity, min(4096, capacity), replace=False).astype(np.uint64)
    return pr, keys, draw(len(keys))


def _chi2(counts, expect):
    """(chi-square, dof, threshold at p = 1e-4) of counts against expected counts; bins that
    expect nothing must be empty, and bins that expect under 5 are merged into one."""
    from scipy.stats import chi2 as chi2_dist
    counts, expect = np.asarray(counts, np.float64), np.asarray(expect, np.float64)
    assert counts[expect == 0].sum() == 0, "a zero-weight slot was drawn"
    small = (expect > 0) & (expect < 5)
    keep = expect >= 5
    c, e = list(counts[keep]), list(expect[keep])
    if small.any():
        cs, es = counts[small].sum(), expect[small].sum()
        if es >= 5 or not e:
            c.append(cs)
            e.append(es)
        else:
            c[-1] += cs
            e[-1] += es
    c, e = np.array(c), np.array(e)
    dof = len(e) - 1
    if dof < 1:
        return None
    return float(((c - e) ** 2 / e).sum()), dof, float(chi2_dist.isf(1e-4, dof))


def chi2_statistics(counts, priorities, alpha):
    """Chi-square of per-slot draw counts against numpy's p**alpha (not the tree): binned by
    level-1 node (64 slots), and over the 64 heaviest slots plus the rest."""
    w = np.asarray(priorities, np.float64) ** alpha
    w[np.asarray(priorities) <= 0] = 0.0
    expect = w / w.sum() * counts.sum()
    assert counts[w == 0].sum() == 0, "a zero-weight slot was drawn"
    pad = -len(w) % 64
    out = {}
    binned = _chi2(np.pad(counts, (0, pad)).reshape(-1, 64).sum(1),
                   np.pad(expect, (0, pad)).reshape(-1, 64).sum(1))
    if binned:
        out["binned"] = binned
    top = np.argsort(-w, kind="stable")[:64]
    rest = np.ones(len(w), bool)
    rest[top] = False
    heavy = _chi2(np.append(counts[top], counts[rest].sum()),
                  np.append(expect[top], expect[rest].sum()))
    if heavy:
        out["heaviest"] = heavy
    return out
