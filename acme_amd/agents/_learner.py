"""What the learners in acme_amd.agents.*.learning share: the host code above native.py.

`Learner` is the base of every learner (counter, logger and the end of a step; `native`,
`num_steps`, `state`; the Adam-moment restore).  `PlaneLearner` adds what the learners on the
f16 plane engine share (DQN, IMPALA, R2D2): the lazy step-guard check and the checkpoint with
the applied count and the plane scales.  The functions below them prepare the recurrent
learners' batches and acting inputs (IMPALA, R2D2).
"""

from __future__ import annotations

import time
from typing import Dict, Optional

import numpy as np
import torch

from acme_amd import core
from acme_amd.utils import counting, loggers


class Learner(core.Learner, core.Saveable):
    """A learner over one native handle (`self._native`, an acme_amd.native._NativeLearner)."""

    _counter_args = ()      # counting.Counter's arguments when the caller passes no counter
    _log_time_delta = 1.0   # the default TerminalLogger's

    def _init_bookkeeping(self, counter: Optional[counting.Counter],
                          logger: Optional[loggers.Logger]) -> None:
        self._counter = counter or counting.Counter(*self._counter_args)
        self._logger = logger or loggers.TerminalLogger("learner",
                                                        time_delta=self._log_time_delta)
        self._timestamp = None

    def _finish_step(self, result: Dict, skipped: int = 0) -> None:
        """The end of every step(): counts the step with the wall time since the previous
        one and logs `result` (device scalars: fetched only when a line is emitted)."""
        now = time.time()
        elapsed = now - self._timestamp if self._timestamp else 0
        self._timestamp = now
        if skipped:
            result["skipped_steps"] = skipped
        result.update(self._counter.increment(steps=1, walltime=elapsed))
        self._logger.write(result)

    @property
    def native(self):
        return self._native

    @property
    def num_steps(self) -> int:
        return self._native.num_steps

    @property
    def state(self) -> Dict:
        return self.save()

    def _restore_moments(self, optimizer: Dict) -> None:
        n = self._native
        for buf, src in ((n.m, optimizer["m"]), (n.v, optimizer["v"])):
            for k, t in n.views(buf).items():
                t.copy_(torch.as_tensor(np.asarray(src[k], np.float32)).view(t.shape))


class PlaneLearner(Learner):
    """A learner whose native handle has the plane-scale and step-guard state
    (native._PlaneState).  A step whose f16 planes overflowed (or, for the recurrent learners,
    whose LSTM unroll timed out) is skipped on the device; the learner sees the count lazily
    at its next step()."""

    _algorithm = ""     # names the learner in messages
    _skip_causes = ""   # "skipped ...": the end of the message on_plane_overflow="raise" raises
    _overflow_modes = ("skip", "raise")
    _has_target = True  # the checkpoint has a "target_network"

    def _init_guard(self, on_plane_overflow: str) -> None:
        if on_plane_overflow not in self._overflow_modes:
            modes = [repr(m) for m in self._overflow_modes]
            raise ValueError(f"on_plane_overflow must be {', '.join(modes[:-1])} or {modes[-1]}")
        self._on_overflow = on_plane_overflow
        self._skips_seen = 0

    def _check_guard(self) -> int:
        """Skipped steps the device has reported so far (a pinned host word: no
        synchronisation); on a new one, raise, or have the planes re-split and the scales
        recalibrated before the next step."""
        n = self._native.skipped_steps
        if n != self._skips_seen:
            self._skips_seen = n
            if self._on_overflow == "raise":
                raise FloatingPointError(
                    f"{self._algorithm} learner: {n} step(s) {self._skip_causes}")
            self._native.params_changed()
        return n

    def save(self) -> Dict:
        n = self._native
        state = {"network": n.get_params("params")}
        if self._has_target:
            state["target_network"] = n.get_params("target")
        # Adam's t is the updates applied (step() calls minus skipped steps), num_steps the
        # step() calls (the target period counts those).  Restoring the f16 plane scales
        # (csrc/gemm_p3.h) keeps a resumed run bit-identical to an uninterrupted one.
        state.update(optimizer={"m": n.get_params("m"), "v": n.get_params("v"),
                                "step": n.applied_steps},
                     num_steps=n.num_steps, plane_scales=n.scale_state())
        return state

    def restore(self, state: Dict) -> None:
        n, opt = self._native, state["optimizer"]
        n.set_params(state["network"], *([state["target_network"]] if self._has_target else ()))
        self._restore_moments(opt)
        # New parameters recalibrate the scales at the next step, unless a scale state is
        # restored after this call (set_params has made it too: it only sets flags).
        n.params_changed()
        if "plane_scales" in state:
            n.set_scale_state(state["plane_scales"])
        # num_steps before the applied count: acme_r2d2_set_num_steps also writes Adam's count.
        n.num_steps = int(state["num_steps"])
        # Round-4 R2D2 checkpoints have "step" = num_steps and the applied count under
        # "applied_steps"; no other learner ever wrote that key, so it is read for all.
        n.applied_steps = int(opt.get("applied_steps", opt.get("step", state["num_steps"])))


# ---------------------------------------------------------------- recurrent learners
def obs_dtype(network) -> torch.dtype:
    """The dtype a network descriptor's observations reach the device in."""
    return torch.uint8 if network.obs_dtype == "uint8" else torch.float32


def state_parts(core_state):
    """(hidden, cell) of an LSTMState or of the dict a dataset may hand out instead."""
    if isinstance(core_state, dict):
        return core_state["hidden"], core_state["cell"]
    hidden, cell = core_state
    return hidden, cell


def check_oar(observation, network_name: str) -> None:
    if not hasattr(observation, "observation"):
        raise ValueError(f"{network_name} takes OAR observations "
                         "(wrap the environment in ObservationActionRewardWrapper)")


def to_device(device, non_blocking: bool = False):
    """convert(x, dtype): a host array (or anything np.asarray takes) as a device tensor."""
    def convert(x, dtype):
        return torch.as_tensor(np.asarray(x)).to(device, dtype, non_blocking=non_blocking)
    return convert


def sequence_batch(data, frames_dtype):
    """The six contiguous [B, T, ...] tensors a recurrent native step takes, from a sequence
    sample's Step(observation=OAR(...), action, reward, discount, ...): frames, previous
    action, previous reward, action, reward, discount."""
    obs = data.observation
    B, T = int(data.action.shape[0]), int(data.action.shape[1])
    c = lambda x, t: x.to(t).contiguous()  # noqa: E731
    frames = obs.observation.reshape((B, T, -1)) if frames_dtype == torch.float32 \
        else obs.observation
    return (c(frames, frames_dtype), c(obs.action.reshape(B, T), torch.int32),
            c(obs.reward.reshape(B, T), torch.float32), c(data.action.reshape(B, T), torch.int32),
            c(data.reward.reshape(B, T), torch.float32),
            c(data.discount.reshape(B, T), torch.float32))


def initial_core_state(extras):
    """The stored core state at t = 0 as two [B, H] float32 views of the [B, T, H] extras."""
    hidden, cell = state_parts(extras["core_state"])
    return hidden.to(torch.float32)[:, 0], cell.to(torch.float32)[:, 0]


def acting_inputs(convert, frames_dtype, observation, prev_action, prev_reward, hidden, cell):
    """The five device tensors of a batched network step for `rows` actors (policy_step,
    q_step) from host arrays: frames [rows, -1], previous action and reward [rows], core
    state [rows, H]."""
    rows = int(np.asarray(prev_action).shape[0])
    return (convert(observation, frames_dtype).reshape(rows, -1),
            convert(prev_action, torch.int32), convert(prev_reward, torch.float32),
            convert(hidden, torch.float32).contiguous(),
            convert(cell, torch.float32).contiguous())
