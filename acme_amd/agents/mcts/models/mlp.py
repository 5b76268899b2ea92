"""MLPModel — drop-in for acme/agents/tf/mcts/models/mlp.py:78-221: an environment model learned
from the agent's own transitions, so MCTS can plan without access to the simulator.

Three MLP towers on [flatten(o), onehot(a)] predict the next observation, the reward and a
discount logit (networks.MLPTransitionModel).  Everything the model holds lives on the GPU:

  * the transitions, in a ring of `replay_capacity` rows [o_t, a, r, d, o_tp1] (the oldest row
    is overwritten, as bsuite's Replay does); `update` writes one row with one packed copy;
  * the batch indices of an SGD step, drawn by torch.randint on a seeded device generator with
    no synchronisation (readable as `last_indices`); the step gathers its rows from the ring
    itself (acme_mlp_model_step, two launches);
  * the current state, in one of three packed prediction buffers [next state, reward, logit]:
    `step(action)` is one launch (acme_mlp_model_predict, the action passed by value) from the
    current buffer into a free one and one packed copy back; `save_checkpoint` and
    `load_checkpoint` only switch which buffer is the checkpoint or the current one.

Termination.  The reference takes `scipy.special.softmax` of the single discount logit, which
is 1.0 whatever the logit, so its `step` never returns a termination and a planned episode ends
only with the search's depth.  discount_activation="softmax" (the default) keeps that, since
the agents here are drop-ins; "sigmoid" terminates when sigmoid(logit) < terminal_tol, which
is what the discount tower is trained for.
"""

from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from acme_amd import dm_env, specs
from acme_amd.agents.mcts.models import base
from acme_amd.native import NativeMLPModel
from acme_amd.networks import MLPTransitionModel


class MLPModel(base.Model):

    def __init__(self, environment_spec: specs.EnvironmentSpec, replay_capacity: int,
                 batch_size: int, hidden_sizes: Sequence[int], learning_rate: float = 1e-3,
                 terminal_tol: float = 1e-3, seed: int = 0, device=None,
                 discount_activation: str = "softmax"):
        if discount_activation not in ("softmax", "sigmoid"):
            raise ValueError("discount_activation must be 'softmax' or 'sigmoid', got "
                             f"{discount_activation!r}")
        if replay_capacity < 1 or batch_size < 1:
            raise ValueError("replay_capacity and batch_size must be >= 1")
        self._obs_spec = environment_spec.observations
        self._action_spec = environment_spec.actions
        self._batch_size = int(batch_size)
        self._terminal_tol = terminal_tol
        self._sigmoid = discount_activation == "sigmoid"
        net = MLPTransitionModel(self._obs_spec.shape, self._action_spec.num_values,
                                 hidden_sizes)
        self._D = D = net.obs_dim
        self._native = NativeMLPModel(obs_dim=D, hidden=net.hidden, num_actions=net.num_actions,
                                      max_batch=self._batch_size, max_rows=1,
                                      learning_rate=learning_rate, device=device)
        self._native.set_params(net.init(seed))
        dev = self._native.device
        self._capacity = int(replay_capacity)
        self._ring = torch.zeros(self._capacity, 2 * D + 3, dtype=torch.float32, device=dev)
        self._num_added = 0
        self._generator = torch.Generator(device=dev)
        self._generator.manual_seed(seed)
        self.last_indices = None
        # The packed prediction buffers: the current state, the checkpoint, a free one.
        self._bufs = torch.zeros(3, D + 2, dtype=torch.float32, device=dev)
        self._cur, self._ckpt = 0, None
        self._needs_reset = True

    # ------------------------------------------------------------------ state
    def _free(self) -> int:
        return next(i for i in range(3) if i != self._cur and i != self._ckpt)

    def _set_state(self, observation) -> None:
        """Uploads a true observation into a free buffer, which becomes the current one (the
        checkpoint's buffer is never written)."""
        flat = np.ascontiguousarray(np.asarray(observation, np.float32).reshape(-1))
        if flat.size != self._D:
            raise ValueError(f"observation of shape {np.shape(observation)} does not hold "
                             f"{self._D} values")
        i = self._free()
        self._bufs[i, :self._D].copy_(torch.from_numpy(flat))
        self._cur = i

    def step(self, action):
        if self._needs_reset:
            raise ValueError("Model must be reset with an initial timestep.")
        D, nxt = self._D, self._free()
        self._native.predict_packed(self._bufs[self._cur:self._cur + 1], int(action),
                                    out=self._bufs[nxt:nxt + 1])
        self._cur = nxt
        host = self._bufs[nxt].cpu().numpy()
        observation = host[:D].reshape(self._obs_spec.shape).copy()
        reward, logit = float(host[D]), float(host[D + 1])
        # softmax over the single logit is 1 (the reference's rule): no termination.
        discount = 1.0 / (1.0 + np.exp(-logit)) if self._sigmoid else 1.0
        if discount < self._terminal_tol:
            self._needs_reset = True
            return dm_env.termination(reward=reward, observation=observation)
        return dm_env.transition(reward=reward, observation=observation)

    def reset(self, initial_state=None):
        if initial_state is None:
            raise ValueError("Model must be reset with an initial state.")
        self._set_state(initial_state)
        self._needs_reset = False
        return dm_env.restart(np.array(initial_state, copy=True))

    def update(self, timestep, action, next_timestep):
        # The true transition goes into the ring: one packed row, one copy.
        D = self._D
        row = np.empty(2 * D + 3, np.float32)
        row[:D] = np.asarray(timestep.observation, np.float32).reshape(-1)
        row[D:D + 3] = (action, next_timestep.reward, next_timestep.discount)
        row[D + 3:] = np.asarray(next_timestep.observation, np.float32).reshape(-1)
        self._ring[self._num_added % self._capacity].copy_(torch.from_numpy(row))
        self._num_added += 1
        # The synthetic step is taken before the true next observation is copied in.
        ts = self.step(action)
        self._set_state(next_timestep.observation)
        if ts.last() or next_timestep.last():
            self._needs_reset = True
        if self.size >= self._batch_size:
            self.last_indices = torch.randint(
                0, self.size, (self._batch_size,), generator=self._generator,
                device=self._native.device, dtype=torch.int32)
            self._native.step(self._ring, self.last_indices)
        return ts

    def save_checkpoint(self):
        if self._needs_reset:
            raise ValueError("Cannot save checkpoint: model must be reset first.")
        self._ckpt = self._cur

    def load_checkpoint(self):
        if self._ckpt is None:
            raise ValueError("Cannot load checkpoint: none was saved.")
        self._needs_reset = False
        self._cur = self._ckpt

    # ------------------------------------------------------------------ the rest
    def action_spec(self):
        return self._action_spec

    def observation_spec(self):
        return self._obs_spec

    @property
    def needs_reset(self) -> bool:
        return self._needs_reset

    @property
    def size(self) -> int:
        """Transitions in the ring."""
        return min(self._num_added, self._capacity)

    @property
    def num_steps(self) -> int:
        """SGD steps taken."""
        return self._native.num_steps

    @property
    def native(self) -> NativeMLPModel:
        return self._native

    @property
    def state_row(self) -> torch.Tensor:
        """The current state on the device, float32 [D]: a read-only view of the current
        prediction buffer's row (the device search reads its root from it in place)."""
        if self._needs_reset:
            raise ValueError("Model must be reset with an initial timestep.")
        return self._bufs[self._cur, :self._D]

    @property
    def sigmoid_discount(self) -> bool:
        """discount_activation == 'sigmoid': step() can return a termination."""
        return self._sigmoid

    @property
    def terminal_tol(self) -> float:
        return self._terminal_tol
