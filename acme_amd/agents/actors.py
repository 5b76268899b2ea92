"""Actors (acme/agents/tf/actors.py:35-94 FeedForwardActor, :95-172 RecurrentActor) and the
epsilon-greedy DQN policy (trfl.epsilon_greedy used at acme/agents/tf/dqn/agent.py:118-124)."""

from __future__ import annotations

from typing import Callable, Optional

import numpy as np

from acme_amd import core


class FeedForwardActor(core.Actor):
    """Runs `policy` on a batch of one observation; forwards experience to an adder."""

    def __init__(self, policy: Callable, adder=None, variable_client=None):
        self._policy = policy
        self._adder = adder
        self._variable_client = variable_client

    def select_action(self, observation):
        batched = np.asarray(observation)[None]
        return np.asarray(self._policy(batched))[0]

    def observe_first(self, timestep):
        if self._adder is not None:
            self._adder.add_first(timestep)

    def observe(self, action, next_timestep):
        if self._adder is not None:
            self._adder.add(action, next_timestep)

    def update(self):
        if self._variable_client is not None:
            self._variable_client.update()


class RecurrentActor(core.Actor):
    """A recurrent actor (acme/agents/tf/actors.py:95-172): unbatched observations in,
    unbatched actions out, the recurrent state reset at episode starts and the state that
    went into each step handed to the adder as extras={"core_state": LSTMState(h, c)} (the
    layout of agents/r2d2/make_replay's signature).

    `policy(observation, state, store_state)` runs one step and returns (action,
    state_before_the_step): `state` is the LSTMState [1, H] to start from on an episode's
    first call (`initial_state(1)`), None afterwards (the policy carries its own state, which
    may live on the device); the returned state is an LSTMState [1, H], or None when
    store_state is False.  R2D2Learner.make_policy builds one."""

    def __init__(self, policy: Callable, initial_state: Callable, adder=None,
                 variable_client=None, store_recurrent_state: bool = True):
        self._policy = policy
        self._initial_state = initial_state  # batch_size -> LSTMState
        self._adder = adder
        self._variable_client = variable_client
        self._store = bool(store_recurrent_state)
        self._fresh = True        # the next call starts from initial_state(1)
        self._prev_state = None   # the state that went into the last step

    def select_action(self, observation):
        state = self._initial_state(1) if self._fresh else None
        self._fresh = False
        action, self._prev_state = self._policy(observation, state, self._store)
        return action

    def observe_first(self, timestep):
        if self._adder is not None:
            self._adder.add_first(timestep)
        self._fresh = True  # re-initialised at the next policy call

    def observe(self, action, next_timestep):
        if self._adder is None:
            return
        if not self._store:
            self._adder.add(action, next_timestep)
            return
        from acme_amd.networks import LSTMState
        h, c = self._prev_state
        core_state = LSTMState(np.asarray(h, np.float32)[0], np.asarray(c, np.float32)[0])
        self._adder.add(action, next_timestep, extras={"core_state": core_state})

    def update(self):
        if self._variable_client is not None:
            self._variable_client.update()


class EpsilonGreedyPolicy:
    """a ~ (1 - eps) * uniform over argmax q + eps * uniform over actions (trfl semantics:
    greedy ties share the greedy mass)."""

    def __init__(self, q_fn: Callable, num_actions: int, epsilon: float = 0.05, seed: int = 0,
                 action_dtype=np.int32):
        self._q_fn = q_fn
        self._A = int(num_actions)
        self.epsilon = float(epsilon)
        self._rng = np.random.default_rng(seed)
        self._dtype = action_dtype

    def __call__(self, batched_obs):
        q = np.asarray(self._q_fn(batched_obs))
        out = np.empty(q.shape[0], self._dtype)
        for i, row in enumerate(q):
            greedy = np.flatnonzero(row == row.max())
            probs = np.full(self._A, self.epsilon / self._A)
            probs[greedy] += (1.0 - self.epsilon) / len(greedy)
            out[i] = self._rng.choice(self._A, p=probs / probs.sum())
        return out
