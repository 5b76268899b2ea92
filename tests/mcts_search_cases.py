"""The cases of the device tree search's edge tests, shared by
tests/test_mcts_native_search_edges_gpu.py (which runs acme_mcts_search_run on them) and
tests/test_mcts_search_cases_cpu.py (which checks, from the float64 reference alone and without
a GPU, the conditions the GPU comparison rests on and the property each case exists for).  Test
infrastructure only.

Every seed was chosen by a search on the CPU, over the range noted beside the case, for the
first one that meets the conditions of assert_comparable; none was tuned against the kernel.
"""

from __future__ import annotations

import dataclasses
from typing import Tuple

import numpy as np

from acme_amd import _lib
from tests import az_oracle as AO, mlp_model_oracle as MO
from tests.mcts_search_oracle import _reference


@dataclasses.dataclass(frozen=True)
class Case:
    D: int
    mh: Tuple[int, ...]           # the model's hidden widths
    zh: Tuple[int, ...]           # the policy-value trunk's
    A: int
    S: int                        # num_simulations of the run
    seed: int                     # parameters, root state and (without tie_seed) Philox
    activation: str = "softmax"
    discount: float = 0.99
    tol: float = 0.5              # terminal_tol, read only with activation == "sigmoid"
    max_sim: int = 0              # the handle's max_simulations; 0: S
    stream: bool = False
    call_counter: int = 0
    tie_seed: int = -1            # the Philox seed; -1: seed
    zero: object = False          # mcts_search_oracle._setup's
    override: tuple = ()          # mcts_search_oracle._setup's

    @property
    def cap(self):
        return self.max_sim or self.S

    @property
    def philox_seed(self):
        return self.seed if self.tie_seed < 0 else self.tie_seed

    def but(self, **kw):
        return dataclasses.replace(self, **kw)


def reference(c: Case):
    return _reference(c.D, c.mh, c.zh, c.A, c.S, c.activation, c.discount, c.seed,
                      call_counter=c.call_counter, zero=c.zero, terminal_tol=c.tol,
                      tie_seed=None if c.tie_seed < 0 else c.tie_seed, override=c.override)


def assert_comparable(c: Case, ref):
    """What lets float32 counts be compared with float64's for equality and the root value
    with _close: no selection within rounding of a tie, no sigmoid within rounding of the
    tolerance, and a root value that is not the remainder of a cancellation.  The root value is
    one dot product h . wv + bv of n <= 256 terms; its float32 error is of the order
    sqrt(n) u sum_k |h_k wv_k| ~ 1e-6 of the terms' sum, and _close allows 1.2e-5 |value|, so
    the value must be at least a tenth of that sum."""
    assert ref["bad_at"] is None
    assert ref["gap"] >= 1e-3 * ref["scale"], (ref["gap"], ref["scale"])
    if c.activation == "sigmoid" and 0 < c.tol < 1:
        assert ref["tol_gap"] >= 1e-3, ref["tol_gap"]
    assert abs(ref["root_value"]) >= 0.1 * ref["root_value_terms"] or c.zero is True


# a. One handle of 24 simulations run at S = 24, 1, 7, 24, with and without terminals (the
# sigmoid runs leave rows of the visits table past `nodes`).  Seeds searched: 0..199.
SMALL = Case(5, (7,), (7,), 3, 24, seed=1, max_sim=24)
REUSE_S = (24, 1, 7, 24)
REUSE = [SMALL.but(S=s) for s in REUSE_S]
REUSE_SIGMOID = [SMALL.but(S=s, activation="sigmoid", tol=0.5) for s in (24, 7)]

# b. Zero parameters, A = 64, the tree at 130088 of its 131072 bytes: every selection is a tie,
# the first among all 64 lanes.  The first two differ in the seed's high word alone, the last
# two in the call counter alone.
TIES = [Case(5, (7,), (7,), 64, 100, seed=0, discount=1.0, zero=True, tie_seed=ts,
             call_counter=cc)
        for ts, cc in ((7, 0), (7 + (3 << 32), 0), (7 + (3 << 32), (1 << 32) + 5))]

# c. One action: the tree is a chain and simulation s descends s + 1 levels.
# Seeds searched: 0..199; no scores to tie, the first seed whose root value is not cancelled.
CHAIN = Case(5, (7,), (7,), 1, 128, seed=2)

# d. Terminals.  tol = 2 makes every edge terminal, tol = 0 none; MIXED has some, on a model of
# two hidden layers.  Seeds searched: 0..199 each.
ALL_TERMINAL = SMALL.but(activation="sigmoid", tol=2.0, seed=4)
NONE_TERMINAL = SMALL.but(activation="sigmoid", tol=0.0)
MIXED = Case(6, (5, 9), (8,), 4, 24, seed=100, activation="sigmoid", tol=0.3)
DISCOUNT0 = SMALL.but(discount=0.0, seed=0)

# e. The widths at their limits: e = [D + A] fills its 320 floats, the towers run all four
# layers with a width-1 layer between two full ones, the trunk has ACME_MAX_MLP_LAYERS layers.
# Necessarily streamed (1.6 MB of weights).  DEEP is the same depth at small widths, resident.
# Seeds searched: 0..199 each.
WIDE = Case(256, (256, 1, 256), (256, 129, 1, 256, 129, 200, 256, 129), 64, 8, seed=1)
DEEP = Case(6, (5, 9, 3), (5, 3, 6, 4, 7, 2, 8, 5), 4, 8, seed=0)
assert len(WIDE.zh) == len(DEEP.zh) == _lib.MAX_MLP_LAYERS
assert len(WIDE.mh) == len(DEEP.mh) == _lib.MLP_MODEL_MAX_HIDDEN

# f. The residency boundary: FITS fills ACME_MCTS_SEARCH_LDS_BYTES to the byte, SPILLS is the
# same network with one more hidden unit in the trunk.  With A = 6 the tree is 128 (S + 1)
# bytes, so S = 7 leaves 146432 bytes = 572 tensor paddings of 64 floats for the weights.
# SIGMOID is the existing (20, (33, 17), (36, 68), 18) case of
# tests/test_mcts_native_search_gpu.py, which compares it with float64; here its resident and
# its streamed run are compared with each other.
FITS = Case(23, (245,), (250,), 6, 7, seed=25)
SPILLS = FITS.but(zh=(251,))
SIGMOID = Case(20, (33, 17), (36, 68), 18, 40, seed=67, activation="sigmoid", tol=0.5)

# g. Bad scores.  NaN in the root state: the first selection fails.  +inf as the reward
# tower's last bias: the first simulation completes, the second selection fails.
NAN_ROOT = SMALL.but(override=(("root", 2, float("nan")),))
INF_REWARD = SMALL.but(override=(("model:reward_network/linear_1/b", 0, float("inf")),))
# NaN ahead of a ReLU, which must let it through as np.maximum does: in the root state under a
# trunk of two layers (the first selection fails), and in the reward tower's hidden layer (the
# second does).  Seeds searched for DEEP_TRUNK: 0..199.
DEEP_TRUNK = Case(5, (7,), (7, 6), 3, 24, seed=2)
NAN_UNDER_RELU = DEEP_TRUNK.but(override=(("root", 2, float("nan")),))
NAN_IN_TOWER = SMALL.but(override=(("model:reward_network/linear_0/w", 3, float("nan")),))
BAD = dict(nan_root=NAN_ROOT, inf_reward=INF_REWARD, nan_under_relu=NAN_UNDER_RELU,
           nan_in_tower=NAN_IN_TOWER)

COMPARED = dict(
    **{f"reuse_S{c.S}": c for c in REUSE}, **{f"reuse_sigmoid_S{c.S}": c for c in REUSE_SIGMOID},
    **{f"ties_{i}": c for i, c in enumerate(TIES)}, chain=CHAIN, all_terminal=ALL_TERMINAL,
    none_terminal=NONE_TERMINAL, mixed=MIXED, discount0=DISCOUNT0, wide=WIDE, deep=DEEP,
    fits=FITS, spills=SPILLS, deep_trunk=DEEP_TRUNK)


def flat_size(shapes) -> int:
    """The flat parameter buffer of a native learner: every tensor padded to 64 floats."""
    return sum(-(-int(np.prod(s)) // 64) * 64 for _, s in shapes)


def lds_bytes(c: Case, model_flat=None, az_flat=None) -> int:
    """4 w_off + 4 (model flat + az flat): what acme_mcts_search_run compares with
    ACME_MCTS_SEARCH_LDS_BYTES.  The flats come from the handles where given, otherwise from
    the tensor shapes."""
    if model_flat is None:
        model_flat = flat_size(MO.tensor_shapes(MO.Config(c.D, c.mh, c.A)))
        az_flat = flat_size(AO.az_tensor_shapes(AO.AZConfig(c.D, c.zh, c.A)))
    tree = (20 * c.A + 8) * (c.cap + 1)
    w_off = -(-(_lib.MCTS_SEARCH_FIXED_BYTES + tree) // 16) * 4
    return 4 * w_off + 4 * (model_flat + az_flat)


def resident(c: Case, model_flat=None, az_flat=None) -> bool:
    return not c.stream and lds_bytes(c, model_flat, az_flat) <= _lib.MCTS_SEARCH_LDS_BYTES
