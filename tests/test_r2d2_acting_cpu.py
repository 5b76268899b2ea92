"""The R2D2 acting surface without a GPU: the two ABI entries are declared, exported and
bound; the selection oracle (tests/r2d2_act_oracle.py) has trfl's epsilon-greedy
distribution and its edge cases; RecurrentActor's state handling
(acme/agents/tf/actors.py:95-172) with a numpy policy; R2D2AtariNetwork.initial_state."""

import ctypes
import os
import re

import numpy as np

from acme_amd import dm_env
from acme_amd.agents.actors import RecurrentActor
from acme_amd.networks import LSTMState, R2D2AtariNetwork
from tests import r2d2_act_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_acting_entries_declared_exported_and_bound():
    from acme_amd import _lib
    text = open(os.path.join(ROOT, "include", "acme_hip.h")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("acme_r2d2_q_step", "acme_epsilon_greedy"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), f"{name} not declared"
        assert hasattr(L, name), f"{name} not exported"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} has no ctypes signature"
    assert len(_lib._SIGS["acme_r2d2_q_step"][1]) == 17
    assert len(_lib._SIGS["acme_epsilon_greedy"][1]) == 8


def test_oracle_distribution_with_tied_maxima():
    """20,000 rows of one q (A = 5, maxima tied at actions 1 and 3), epsilon 0.25: every
    action's frequency within 5 binomial standard deviations of eps / A + (1 - eps) *
    [greedy] / 2."""
    q = np.array([0.5, 2.0, -1.0, 2.0, 1.5], np.float32)
    n, eps, A = 20000, 0.25, 5
    acts = S.select(np.tile(q, (n, 1)), eps, seed=2024, step=7)
    assert acts.min() >= 0 and acts.max() < A
    for a in range(A):
        p = eps / A + (1 - eps) * (0.5 if a in (1, 3) else 0.0)
        sd = np.sqrt(p * (1 - p) / n)
        f = float(np.mean(acts == a))
        assert abs(f - p) <= 5 * sd, (a, f, p, sd)


def test_oracle_edges():
    rng = np.random.default_rng(0)
    q = rng.standard_normal((500, 7)).astype(np.float32)
    q[::3, 2] = q[::3].max(axis=1)  # some ties
    # epsilon 0: never outside the greedy set.
    a0 = S.select(q, 0.0, 1, 2)
    for i in range(len(q)):
        assert a0[i] in S.greedy_set(q[i])
    # epsilon 1: q is ignored.
    np.testing.assert_array_equal(S.select(q, 1.0, 1, 2), S.select(-q, 1.0, 1, 2))
    assert len(np.unique(S.select(q, 1.0, 1, 2))) == 7
    # A = 1.
    for eps in (0.0, 0.4, 1.0):
        assert not S.select(rng.standard_normal((50, 1)), eps, 3, 4).any()
    # An all-NaN row gives 0, whatever the draw, unless it explores.
    nan = np.full((200, 6), np.nan, np.float32)
    assert not S.select(nan, 0.0, 5, 6).any()
    # A NaN beside finite values is never chosen greedily.
    mixed = rng.standard_normal((300, 4)).astype(np.float32)
    mixed[:, 1] = np.nan
    mixed[::2, 3] = np.nan
    am = S.select(mixed, 0.0, 7, 8)
    assert not np.isnan(mixed[np.arange(300), am]).any()
    for i in range(300):
        assert mixed[i, am[i]] == np.nanmax(mixed[i])
    # Draws depend on the step and on the row, and repeat.
    np.testing.assert_array_equal(S.select(q, 0.5, 9, 1), S.select(q, 0.5, 9, 1))
    assert (S.select(q, 0.5, 9, 1) != S.select(q, 0.5, 9, 2)).any()
    assert S.select(q[:1], 1.0, 9, 1, first_row=3)[0] == \
        S.select(np.tile(q[:1], (4, 1)), 1.0, 9, 1)[3]


class _NumpyPolicy:
    """A recurrent policy on the host: h <- h + obs, c <- c - 1; action = the call count."""

    def __init__(self, H):
        self.H, self.h, self.c, self.calls, self.stores = H, None, None, 0, []

    def __call__(self, observation, state, store_state):
        if state is not None:
            self.h, self.c = np.array(state.hidden), np.array(state.cell)
        before = LSTMState(self.h.copy(), self.c.copy()) if store_state else None
        self.h = self.h + np.float32(observation)
        self.c = self.c - np.float32(1)
        self.calls += 1
        self.stores.append(store_state)
        return np.int32(self.calls), before


class _Adder:
    def __init__(self):
        self.first, self.added = [], []

    def add_first(self, timestep):
        self.first.append(timestep)

    def add(self, action, next_timestep, extras=None):
        self.added.append((action, next_timestep, extras))


class _Client:
    updates = 0

    def update(self):
        self.updates += 1


def _episode(actor, obs, length):
    actor.observe_first(dm_env.restart(np.float32(obs)))
    for t in range(length):
        a = actor.select_action(np.float32(obs))
        ts = (dm_env.termination(np.float32(0), np.float32(obs)) if t == length - 1 else
              dm_env.transition(np.float32(0), np.float32(obs), np.float32(1)))
        actor.observe(a, ts)


def test_recurrent_actor_state_handling():
    H = 3
    net = R2D2AtariNetwork(4, lstm_size=H, head_size=8, torso="flat", obs_dim=1)
    policy, adder, client = _NumpyPolicy(H), _Adder(), _Client()
    actor = RecurrentActor(policy, net.initial_state, adder, variable_client=client)
    _episode(actor, 2.0, 4)
    _episode(actor, 5.0, 3)
    assert len(adder.first) == 2 and len(adder.added) == 7
    # The extras of step t hold the state that went into step t: zeros at an episode's
    # first step (the state reset at observe_first), then t steps of the policy's update.
    want = [(0, 0), (2, -1), (4, -2), (6, -3), (0, 0), (5, -1), (10, -2)]
    for k, ((action, _, extras), (h, c)) in enumerate(zip(adder.added, want)):
        assert action == k + 1
        assert set(extras) == {"core_state"}
        cs = extras["core_state"]
        assert isinstance(cs, LSTMState)
        assert cs.hidden.shape == (H,) and cs.hidden.dtype == np.float32
        np.testing.assert_array_equal(cs.hidden, np.full(H, h, np.float32))
        np.testing.assert_array_equal(cs.cell, np.full(H, c, np.float32))
    assert all(policy.stores)
    actor.update()
    actor.update()
    assert client.updates == 2
    # Without an adder observe is a no-op; without a client update is.
    bare = RecurrentActor(_NumpyPolicy(H), net.initial_state)
    _episode(bare, 1.0, 2)
    bare.update()


def test_recurrent_actor_without_stored_state():
    H = 2
    net = R2D2AtariNetwork(4, lstm_size=H, head_size=8, torso="flat", obs_dim=1)
    policy, adder = _NumpyPolicy(H), _Adder()
    actor = RecurrentActor(policy, net.initial_state, adder, store_recurrent_state=False)
    _episode(actor, 1.0, 3)
    assert len(adder.added) == 3
    assert all(extras is None for _, _, extras in adder.added)
    assert not any(policy.stores)
    # The state is still carried over the episode and reset at the next one.
    np.testing.assert_array_equal(policy.h, np.full((1, H), 3, np.float32))
    _episode(actor, 1.0, 1)
    np.testing.assert_array_equal(policy.h, np.full((1, H), 1, np.float32))


def test_r2d2_network_initial_state():
    net = R2D2AtariNetwork(18)
    s = net.initial_state(3)
    assert isinstance(s, LSTMState)
    for part in s:
        assert part.shape == (3, 512) and part.dtype == np.float32 and not part.any()
    assert s.hidden is not s.cell
    small = R2D2AtariNetwork(5, lstm_size=16, head_size=8, torso="flat", obs_dim=6)
    assert small.initial_state(1).hidden.shape == (1, 16)
