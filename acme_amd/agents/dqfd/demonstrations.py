"""DemonstrationRecorder — drop-in for acme/agents/tf/dqfd/bsuite_demonstrations.py:35-71.

A demonstration is an (observations, actions, rewards, discounts) tuple of numpy arrays that
each cover one full episode.  Where the reference wraps the recorded episodes in a repeating,
shuffled tf.data generator, `make_dataset()` returns the episode list itself: DQfD and
DemonstrationStore take it as it is and draw episodes uniformly on the device."""

from __future__ import annotations

from typing import List, Tuple

import numpy as np

from acme_amd.utils import tree


def _nested_stack(sequence):
    """Stacks the nested elements of a sequence along a new leading axis."""
    return tree.map_structure(lambda *x: np.stack(x), *sequence)


class DemonstrationRecorder:
    """Records demonstrations step by step, episode by episode."""

    def __init__(self):
        self._demos: List[Tuple[np.ndarray, ...]] = []
        self._reset_episode()

    def step(self, timestep, action: np.ndarray) -> None:
        # As the reference: a missing reward or discount (the first step's) counts as 0.
        reward = np.array(timestep.reward or 0, np.float32)
        self._episode_reward += reward
        self._episode.append((timestep.observation, action, reward,
                              np.array(timestep.discount or 0, np.float32)))

    def record_episode(self) -> None:
        self._demos.append(_nested_stack(self._episode))
        self._reset_episode()

    def discard_episode(self) -> None:
        self._reset_episode()

    def _reset_episode(self) -> None:
        self._episode = []
        self._episode_reward = 0

    @property
    def episode_reward(self):
        return self._episode_reward

    def make_dataset(self) -> List[Tuple[np.ndarray, ...]]:
        """The recorded episodes (the reference's make_tf_dataset fails on none, too)."""
        if not self._demos:
            raise ValueError("no episode has been recorded")
        return list(self._demos)

    make_tf_dataset = make_dataset
