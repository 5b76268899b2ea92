"""The inputs of tests/test_replay_edges_gpu.py through the C oracle alone (no GPU): the oracle
meets every condition the GPU test asserts of the table, so a GPU failure there is the table's.

  * the numpy restatement of the stored tree (tests/_oracle.py levels_from_leaves) ends in the
    oracle's total after every mutation of every walk;
  * degenerate sampling masses (all zero, one live leaf at 1e-300 / 1e300, back to mixed,
    leaves 400 decades apart): the uniform fallback over the live items, probability exactly
    1.0, no zero-weight draw, probability == leaf / total;
  * leaf weights p**alpha against numpy.longdouble;
  * the sampling mass stays finite for finite priorities up to 1e300 with alpha <= 0.9
    (a non-finite mass is outside the contract);
  * the stale-heavy update calls keep at least one live update in ten;
  * the chi-square statistics of the distribution check, on the oracle's own draws.
"""

import numpy as np
import pytest

from tests import _oracle as O
from tests._oracle import OracleTable

ALPHAS = (0.0, 0.6, 1.0)


def _walk_params():
    out = []
    for cap, wrapped in O.edge_shapes():
        for form in ("one", "multi"):
            for alpha in (ALPHAS if cap < 100000 else (0.6,)):
                out.append((cap, wrapped, form, alpha))
    return out


def test_levels_from_leaves_matches_the_oracle_total():
    rng = np.random.default_rng(0)
    for cap in (1, 63, 64, 65, 1088, 4096, 4097, 69632, 70000):
        o = OracleTable(cap, True, 0.6, 1)
        o.insert(O.wide_priorities(rng, cap + 5, 12))
        levels, total = O.check_oracle_tree(o)
        assert len(levels[-1]) == 64 and all(len(x) % 64 == 0 for x in levels)
        assert total > 0.0
    # the scan's order, not a left-to-right sum: they differ in the last bits
    leaves = o.leaves()
    assert np.sum(leaves) != total or np.cumsum(leaves)[-1] != total


@pytest.mark.parametrize("capacity,wrapped,form,alpha", _walk_params())
def test_update_walk_oracle(capacity, wrapped, form, alpha):
    o = OracleTable(capacity, True, alpha, 1234)
    n = O.edge_inserted(capacity, wrapped)
    size = min(n, capacity)
    seen = set()
    for i, (op, args, state) in enumerate(O.edge_update_walk(capacity, wrapped, form)):
        if op == "insert":
            o.insert(*args)
        else:
            assert len(args[0]) in (O.ONE_LAUNCH_SMALL, O.ONE_LAUNCH_MAX, O.MULTI_LAUNCH)
            o.update(*args)
        _, total = O.check_oracle_tree(o)
        if state is None:
            continue
        seen.add(state if isinstance(state, str) else state[0])
        for step in (i, 1000 + i):
            O.assert_draw_state(o.sample(512, step), o.leaves(), total, size, state)
    assert seen == {"zero", "single", "mixed"}


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("capacity,wrapped", O.edge_shapes())
def test_insert_walk_oracle(capacity, wrapped, alpha):
    o = OracleTable(capacity, True, alpha, 1234)
    n = 0
    for i, (prios, state) in enumerate(O.edge_insert_walk(capacity, wrapped)):
        o.insert(prios)
        n += len(prios)
        _, total = O.check_oracle_tree(o)
        O.assert_draw_state(o.sample(512, i), o.leaves(), total, min(n, capacity), state)
    assert (n > capacity) == wrapped


def test_clamp_trap_inputs():
    """The constructed draw of _oracle.clamp_trap: the residual target at node 2 equals the
    node's whole mass (so the count of prefixes <= target is 64 and only the clamp to the last
    non-zero child decides the slot), and the oracle lands it on the node's one live leaf."""
    p, j, slot = O.clamp_trap()
    o = OracleTable(256, True, 1.0, O.CLAMP_TRAP_SEED)
    o.insert(p)
    levels, total = O.check_oracle_tree(o)
    np.testing.assert_array_equal(o.leaves(), p)
    top = O.scan64(levels[1].reshape(1, 64))[0]
    t = O.load().oracle_uniform(O.CLAMP_TRAP_SEED, 0, j) * total
    assert top[1] <= t < top[2] and t < total and (top[3:] > t).all()
    residual = t - top[1]
    row = O.scan64(p[128:192].reshape(1, 64))[0]
    assert residual == levels[1][2] == row[63] and (row <= residual).all()
    s = o.sample(512, 0)
    assert s["slots"][j] == slot and p[slot] > 0
    assert s["probabilities"][j] == p[slot] / total
    O.assert_draw_state(s, p, total, 256, "mixed")


@pytest.mark.parametrize("alpha", [0.3, 0.6, 0.9])
def test_leaf_weight_against_longdouble(alpha):
    """oracle_priority_weight(p, alpha) against numpy.longdouble p**alpha.  The bound
    (|alpha ln p| + 2) * 2**-51 is exp's error on an argument that carries log's relative
    rounding; results below the smallest normal flush to 0 by design.  Measured worst case:
    9.6e-14 (alpha = 0.9, p near 1e300) against a bound of 2.8e-13."""
    L = O.load()
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "needs an extended-precision long double"
    tiny = np.finfo(np.float64).tiny
    worst = 0.0
    for p in O.weight_grid():
        got = L.oracle_priority_weight(float(p), alpha)
        ref = np.longdouble(p) ** np.longdouble(alpha)
        if ref < tiny * (1 + 2.0 ** -40):
            assert got == 0.0 or abs(got - float(ref)) <= 2.0 ** -51 * float(ref), (p, got)
            continue
        bound = (abs(alpha * float(np.log(np.longdouble(p)))) + 2.0) * 2.0 ** -51
        err = float(abs(np.longdouble(got) - ref) / ref)
        worst = max(worst, err)
        assert err <= bound, (p, alpha, got, float(ref), err, bound)
    print(f"alpha {alpha}: worst relative error {worst:.3g}")
    assert L.oracle_priority_weight(0.0, alpha) == 0.0
    assert L.oracle_priority_weight(1.0, alpha) == 1.0


@pytest.mark.parametrize("alpha", [0.3, 0.6, 0.9])
def test_finite_priorities_keep_the_mass_finite(alpha):
    """The contract of DESIGN.md section 3: with finite priorities up to 1e300 and
    alpha <= 0.9 the sampling mass is finite (a leaf is at most 1e270, and no table has
    1e38 slots), so every probability is a finite positive number."""
    cap = 4097
    o = OracleTable(cap, True, alpha, 1234)
    o.insert(np.full(cap + 10, 1e300))
    _, total = O.check_oracle_tree(o)
    assert np.isfinite(total) and total > 0.0
    assert o.leaves().max() <= 1e270 * (1 + 1e-9)
    s = o.sample(512, 0)
    assert np.isfinite(s["probabilities"]).all() and (s["probabilities"] > 0).all()
    O.assert_draw_state(s, o.leaves(), total, cap, "mixed")


def test_non_finite_mass_is_outside_the_contract():
    """Why the contract asks for a finite mass: two leaves near 1.7e308 (alpha = 1) sum to
    +inf, the descent's inf - inf is NaN, and the draw degenerates."""
    o = OracleTable(65, True, 1.0, 1234)
    p = np.ones(65)
    p[3] = p[40] = 1.7e308
    o.insert(p)
    assert np.isinf(o.total())
    s = o.sample(512, 0)
    assert not (s["probabilities"] > 0).all()


@pytest.mark.parametrize("capacity", [4097, 262145])
def test_stale_heavy_inputs(capacity):
    o = OracleTable(capacity, True, 0.6, 1234)
    rng = np.random.default_rng(capacity)
    o.insert(rng.uniform(0.1, 2.0, 4 * capacity))
    for n_upd, groups in O.STALE_CASES:
        for kind, keys, prios in O.stale_heavy_calls(capacity, n_upd, groups):
            before = o.leaves()
            live = O.live_fraction(capacity, 4 * capacity, keys)
            o.update(keys, prios)
            O.check_oracle_tree(o)
            if kind == "all_stale":
                assert live == 0.0
                np.testing.assert_array_equal(o.leaves(), before)
            else:
                assert 0.1 <= live <= 0.5, (kind, live)
                assert not np.array_equal(o.leaves(), before)


@pytest.mark.parametrize("capacity", O.CHI2_CAPACITIES)
def test_distribution_statistics_of_the_oracle(capacity):
    """The statistics of test_replay_edges_gpu.py::test_distribution_independent_of_the_tree
    on the oracle's own draws of the same inputs: the reference alone passes the thresholds.
    Values (binned chi-square / dof / threshold, heaviest-64 chi-square / threshold) are
    recorded in that test's docstring."""
    o = OracleTable(capacity, True, 0.6, O.CHI2_SEED)
    pr, keys, newp = O.chi2_inputs(capacity)
    o.insert(pr)
    o.update(keys, newp)
    final = pr.copy()
    final[keys] = newp  # keys are distinct slots of a table that has not wrapped
    counts = np.zeros(capacity)
    for step in range(O.CHI2_STEPS):
        counts += np.bincount(o.sample(O.CHI2_BATCH, step)["slots"], minlength=capacity)
    stats = O.chi2_statistics(counts, final, 0.6)
    print(capacity, stats)
    for name, (chi2, dof, threshold) in stats.items():
        assert chi2 < threshold, (name, chi2, dof, threshold)
