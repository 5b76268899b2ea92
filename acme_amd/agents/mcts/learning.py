"""AZLearner — drop-in for acme/agents/tf/mcts/learning.py:29-90.

Same constructor arguments and `step()` contract: one call draws a batch of transitions
(o_t, a_t, r_t, d_t, o_tp1, {'pi': search policy}) from the dataset iterator and runs the whole
AlphaZero step on the GPU (acme_az_step: the policy-value network on both observations, the TD
value loss plus the soft-label cross-entropy of the logits against pi, the backward, Adam), then
counts and logs.  The losses are device scalars handed to the logger; nothing synchronises the
host with the device.

`network` is an acme_amd.networks.PolicyValueMLP, `optimizer` anything acme_amd.optimizers
unpacks to plain Adam.  `evaluate` is the network call the MCTS actor makes per tree node: one
native launch on the learner's parameters for up to `batch_size` rows, more rows in chunks of
that many (the reference shares the network object between the actor and the learner).
"""

from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from acme_amd import optimizers
from acme_amd.agents._learner import Learner
from acme_amd.native import NativeAZ
from acme_amd.networks import PolicyValueMLP
from acme_amd.utils import counting, loggers


class AZLearner(Learner):

    _log_time_delta = 30.0  # the reference's TerminalLogger('learner', time_delta=30.)

    def __init__(self, network: PolicyValueMLP, optimizer, dataset, discount: float,
                 logger: Optional[loggers.Logger] = None,
                 counter: Optional[counting.Counter] = None, batch_size: Optional[int] = None,
                 seed: int = 0, device=None):
        if not isinstance(network, PolicyValueMLP):
            raise ValueError("acme_amd's AZ learner takes a networks.PolicyValueMLP, not a "
                             f"{type(network).__name__}")
        adam, clip = optimizers.unpack(optimizer)
        if clip is not None:
            raise ValueError("the AZ learner does not clip gradients")
        self._network = network
        self._iterator = iter(dataset)
        B = batch_size or getattr(dataset, "batch_size", None) or 256
        self._native = NativeAZ(
            obs_dim=network.obs_dim, hidden=network.hidden, num_actions=network.num_actions,
            max_batch=B, max_eval_rows=B, activate_final=network.activate_final,
            discount=discount, learning_rate=adam.learning_rate, adam_beta1=adam.beta1,
            adam_beta2=adam.beta2, adam_epsilon=adam.epsilon, device=device)
        self._native.set_params(network.init(seed))
        self._init_bookkeeping(counter, logger)

    def step(self):
        sample = next(self._iterator)
        o_t, _, r_t, d_t, o_tp1, extras = sample.data
        B = int(r_t.shape[0])
        f = lambda x: x.reshape(B, -1).to(torch.float32).contiguous()  # noqa: E731
        n = self._native
        n.step(f(o_t), f(r_t).reshape(B), f(d_t).reshape(B), f(o_tp1), f(extras["pi"]))
        self._finish_step({"loss": n.loss, "value_loss": n.value_loss,
                           "policy_loss": n.policy_loss})

    def evaluate(self, observations):
        """(probs, values) of a batch of observations as host arrays; a single unbatched
        observation (the network's obs_shape, or flat) gives (probs [A], float)."""
        n = self._native
        x = np.asarray(observations, np.float32)
        batched = x.ndim >= 2 and int(np.prod(x.shape[1:])) == n.obs_dim
        single = not batched and x.size == n.obs_dim
        if not (batched or single):
            raise ValueError(f"observations of shape {x.shape} do not hold {n.obs_dim} features")
        x = x.reshape(-1, n.obs_dim)
        A, step = n.num_actions, n.max_eval_rows  # more rows than that go in chunks
        dev = torch.from_numpy(np.ascontiguousarray(x)).to(n.device)
        outs = [n.evaluate_packed(dev[i:i + step]) for i in range(0, x.shape[0], step)]
        probs, values = [], []
        for i, out in enumerate(o.cpu().numpy() for o in outs):
            rows = min(step, x.shape[0] - i * step)
            probs.append(out[:rows * A].reshape(rows, A))
            values.append(out[rows * A:])
        probs, values = np.concatenate(probs), np.concatenate(values)
        return (probs[0], float(values[0])) if single else (probs, values)

    def get_variables(self, names: List[str]) -> List[Dict[str, np.ndarray]]:
        # As the TF learner: the online network's variables whatever the names.
        del names
        return [self._native.get_params("params")]

    def save(self) -> Dict:
        n = self._native
        return {"params": n.get_params("params"),
                "optimizer": {"m": n.get_params("m"), "v": n.get_params("v"),
                              "step": n.num_steps},
                "num_steps": n.num_steps}

    def restore(self, state: Dict):
        n = self._native
        n.set_params(state["params"])
        self._restore_moments(state["optimizer"])
        n.num_steps = int(state["num_steps"])
