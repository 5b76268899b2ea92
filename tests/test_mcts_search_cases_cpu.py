"""The cases of the device search's GPU tests (tests/mcts_search_cases.py and the CASES of
tests/test_mcts_native_search_gpu.py), checked on the float64 reference alone: every case keeps
clear of score ties, of the terminal tolerance and of a cancelled root value (so that a float32
search must make the same choices), and has the property it exists for.  No GPU, no kernel: a
seed that passes here was not tuned against the code under test."""

import numpy as np
import pytest

from acme_amd import _lib
from tests import mcts_search_cases as C
from tests.mcts_search_oracle import _reference
from tests.test_mcts_native_search_gpu import CASES, TOL


@pytest.mark.parametrize("name", sorted(C.COMPARED))
def test_case_is_comparable(name):
    c = C.COMPARED[name]
    ref = C.reference(c)
    print({k: ref[k] for k in ("gap", "scale", "tol_gap", "nodes", "deepest", "terminal_edges",
                               "revisits", "widest_tie", "root_value", "root_value_terms")})
    C.assert_comparable(c, ref)
    assert ref["simulations"] == c.S == ref["visits"].sum() and ref["nodes"] <= c.S + 1


@pytest.mark.parametrize("D,mh,zh,A,S,activation,discount,stream,seed", CASES)
def test_existing_cases_keep_clear_of_the_tolerance(D, mh, zh, A, S, activation, discount,
                                                    stream, seed):
    ref = _reference(D, mh, zh, A, S, activation, discount, seed, terminal_tol=TOL)
    assert ref["gap"] >= 1e-3 * ref["scale"]
    assert (ref["tol_gap"] >= 1e-3) if activation == "sigmoid" else np.isinf(ref["tol_gap"])


def test_reuse_runs_fewer_simulations_than_the_handle_holds():
    refs = [C.reference(c) for c in C.REUSE]
    assert [c.S for c in C.REUSE] == [24, 1, 7, 24] and all(c.cap == 24 for c in C.REUSE)
    assert [r["nodes"] for r in refs] == [25, 2, 8, 25]
    for c in C.REUSE_SIGMOID:  # rows of the visits table past `nodes`
        ref = C.reference(c)
        assert ref["nodes"] < c.S + 1 and ref["terminal_edges"] >= 1 and ref["revisits"] >= 1


def test_ties_reach_both_halves_of_the_mask_and_every_seed_word():
    refs = [C.reference(c) for c in C.TIES]
    for c, ref in zip(C.TIES, refs):
        assert (c.A, c.S) == (64, 100)
        assert (20 * c.A + 8) * (c.cap + 1) == 130088 <= _lib.MCTS_SEARCH_TREE_BYTES
        assert (20 * c.A + 8) * (c.cap + 2) > _lib.MCTS_SEARCH_TREE_BYTES
        assert ref["widest_tie"] > 32 and ref["high_pick"]
    a, b, c = C.TIES
    assert a.philox_seed < 1 << 32 <= b.philox_seed and a.call_counter == b.call_counter
    assert (a.philox_seed ^ b.philox_seed) & 0xFFFFFFFF == 0  # the high word alone
    assert b.philox_seed == c.philox_seed and c.call_counter >> 32 and b.call_counter == 0
    for i, j in ((0, 1), (1, 2), (0, 2)):
        assert (refs[i]["tree"] != refs[j]["tree"]).any()


def test_chain_is_as_deep_as_the_path_array():
    ref = C.reference(C.CHAIN)
    assert (C.CHAIN.A, C.CHAIN.S, ref["deepest"], ref["nodes"]) == (1, 128, 128, 129)
    # Node i was passed by every later simulation: the staircase.
    np.testing.assert_array_equal(ref["tree"][:, 0], np.arange(128, -1, -1))
    assert abs(ref["values"][0]) > 0.1 and C.CHAIN.discount == 0.99


def test_terminal_cases():
    ref = C.reference(C.ALL_TERMINAL)
    assert (ref["nodes"], ref["deepest"], ref["terminal_edges"]) == (1, 1, C.ALL_TERMINAL.A)
    assert ref["revisits"] == C.ALL_TERMINAL.S - C.ALL_TERMINAL.A
    np.testing.assert_allclose(ref["values"], ref["root_rewards"], rtol=1e-12)
    none, soft = C.reference(C.NONE_TERMINAL), C.reference(C.NONE_TERMINAL.but(
        activation="softmax"))
    assert none["terminal_edges"] == 0 and none["nodes"] == C.NONE_TERMINAL.S + 1
    np.testing.assert_array_equal(none["tree"], soft["tree"])
    ref = C.reference(C.MIXED)
    assert len(C.MIXED.mh) == 2 and C.MIXED.tol not in (0.5, TOL)
    assert ref["terminal_edges"] >= 1 and ref["revisits"] >= 1 and 1 < ref["nodes"] < C.MIXED.S + 1
    ref = C.reference(C.DISCOUNT0)
    assert C.DISCOUNT0.discount == 0.0 and (ref["visits"] > 0).sum() >= 2 and ref["deepest"] >= 2
    # An edge never taken keeps value 0 and reward 0.
    np.testing.assert_allclose(ref["values"], ref["root_rewards"], rtol=1e-12)


def test_widths_at_the_limits():
    w, d = C.WIDE, C.DEEP
    assert (w.D, w.A, w.mh) == (256, 64, (256, 1, 256)) and w.D + w.A == 256 + 64
    assert {256, 1, 129} <= set(w.zh) and max(w.zh) <= _lib.MCTS_SEARCH_MAX_WIDTH
    assert not C.resident(w) and C.resident(d)
    assert (d.D, d.mh, d.A) == (6, (5, 9, 3), 4)


def test_residency_boundary():
    assert C.lds_bytes(C.FITS) == _lib.MCTS_SEARCH_LDS_BYTES  # an exact fit
    assert C.lds_bytes(C.SPILLS) == _lib.MCTS_SEARCH_LDS_BYTES + 256  # one tensor padding over
    assert C.resident(C.FITS) and not C.resident(C.SPILLS)
    assert sum(x != y for x, y in zip(C.FITS.zh + C.FITS.mh, C.SPILLS.zh + C.SPILLS.mh)) == 1
    assert C.resident(C.SIGMOID) and C.resident(C.SMALL)
    s = C.SIGMOID
    assert (s.D, s.mh, s.zh, s.A, s.S, s.activation, s.discount, False, s.seed) in CASES
    assert s.tol == TOL


def test_bad_scores_stop_the_reference_where_the_kernel_must_stop():
    first, second = dict(bad_at=0, nodes=1, simulations=0), dict(bad_at=1, nodes=2, simulations=1)
    assert C.reference(C.NAN_ROOT) == first and C.reference(C.INF_REWARD) == second
    # NaN ahead of a ReLU: a trunk of two layers, a tower's hidden layer.
    assert len(C.NAN_UNDER_RELU.zh) == 2 and C.reference(C.NAN_UNDER_RELU) == first
    assert C.reference(C.NAN_IN_TOWER) == second
    for c in C.BAD.values():  # the clean run that follows on the same handle
        C.assert_comparable(c.but(override=()), C.reference(c.but(override=())))
