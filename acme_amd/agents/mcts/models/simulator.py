"""A perfect model: a private deep copy of the true environment
(acme/agents/tf/mcts/models/simulator.py).  It assumes that the environment, its random state
included, copies with `copy.deepcopy` and that its dynamics are deterministic within an
episode."""

import copy
import dataclasses

from acme_amd import dm_env
from acme_amd.agents.mcts.models import base


@dataclasses.dataclass
class Checkpoint:
    needs_reset: bool
    environment: dm_env.Environment


class Simulator(base.Model):

    def __init__(self, env: dm_env.Environment):
        self._env = copy.deepcopy(env)
        self._needs_reset = True
        self.save_checkpoint()

    def update(self, timestep, action, next_timestep):
        # One call per real transition keeps the copy in step with the real environment.
        del timestep, next_timestep
        return self.step(action)

    def save_checkpoint(self):
        self._checkpoint = Checkpoint(needs_reset=self._needs_reset,
                                      environment=copy.deepcopy(self._env))

    def load_checkpoint(self):
        self._env = copy.deepcopy(self._checkpoint.environment)
        self._needs_reset = self._checkpoint.needs_reset

    def step(self, action):
        if self._needs_reset:
            raise ValueError("the simulator must be reset before it is stepped")
        timestep = self._env.step(action)
        self._needs_reset = timestep.last()
        return timestep

    def reset(self, *unused_args, **unused_kwargs):
        self._needs_reset = False
        return self._env.reset()

    def observation_spec(self):
        return self._env.observation_spec()

    def action_spec(self):
        return self._env.action_spec()

    def reward_spec(self):
        return self._env.reward_spec()

    def discount_spec(self):
        return self._env.discount_spec()

    @property
    def needs_reset(self) -> bool:
        return self._needs_reset
