"""The interface of a model MCTS plans with (acme/agents/tf/mcts/models/base.py): an environment
that can also save and reload its state around a rollout and be kept in step with the real
environment."""

import abc

from acme_amd import dm_env


class Model(dm_env.Environment, abc.ABC):

    @abc.abstractmethod
    def load_checkpoint(self):
        """Goes back to the state of the last save_checkpoint()."""

    @abc.abstractmethod
    def save_checkpoint(self):
        """Remembers the current state (the search reloads it after each simulation)."""

    @abc.abstractmethod
    def update(self, timestep, action, next_timestep):
        """Takes in one real transition; returns the model's own timestep for it."""

    @abc.abstractmethod
    def reset(self, initial_state=None):
        """Resets the model, optionally to a given first observation."""

    @property
    @abc.abstractmethod
    def needs_reset(self) -> bool:
        """Whether the model must be reset before it is stepped."""
