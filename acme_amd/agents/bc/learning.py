"""BCLearner — drop-in for acme/agents/tf/bc/learning.py.

Same constructor arguments and `step()` contract: one call draws a batch of transitions
(o_tm1, a_tm1, r_t, d_t, o_t) from the dataset iterator, uses the first two, and runs the whole
behavioural-cloning step on the GPU (acme_bc_step: the network, the sparse-label softmax
cross-entropy, the backward, Adam and the gradients' global norm), then counts and logs.  `loss`
and `gradient_norm` are device scalars handed to the logger; nothing synchronises the host with
the device.

`network` is an acme_amd.networks.MLP (the reference example's Flatten -> MLP([64, 64, A])).
`make_policy` gives the evaluator of examples/bsuite/run_bc.py: a callable for FeedForwardActor
that runs the network and the epsilon-greedy selection on the learner's parameters in one native
call.  `checkpoint` is accepted for the reference's signature; `save` / `restore` hold the state.
"""

from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from acme_amd.agents._learner import Learner
from acme_amd.native import NativeBC
from acme_amd.networks import MLP
from acme_amd.utils import counting, loggers


class BCLearner(Learner):

    def __init__(self, network: MLP, learning_rate: float, dataset,
                 counter: Optional[counting.Counter] = None,
                 logger: Optional[loggers.Logger] = None, checkpoint: bool = True,
                 batch_size: Optional[int] = None, seed: int = 0, device=None):
        if not isinstance(network, MLP):
            raise ValueError("acme_amd's BC learner takes a networks.MLP, not a "
                             f"{type(network).__name__}")
        if network.obs_dtype != "float32":
            raise ValueError("the BC learner takes float32 observations, not "
                             f"{network.obs_dtype}")
        del checkpoint
        self._network = network
        self._iterator = iter(dataset)
        B = batch_size or getattr(dataset, "batch_size", None) or 256
        self._native = NativeBC(obs_dim=network.obs_dim, hidden=network.hidden,
                                num_actions=network.num_actions, max_batch=B, max_act_rows=B,
                                learning_rate=learning_rate, device=device)
        self._native.set_params(network.init(seed))
        self._init_bookkeeping(counter, logger)

    def step(self):
        sample = next(self._iterator)
        o_tm1, a_tm1 = sample.data[:2]
        B = int(a_tm1.shape[0])
        n = self._native
        n.step(o_tm1.reshape(B, -1).to(torch.float32).contiguous(),
               a_tm1.reshape(B).to(torch.int32).contiguous())
        self._finish_step({"loss": n.loss, "gradient_norm": n.gradient_norm})

    def _rows(self, observations) -> torch.Tensor:
        n = self._native
        x = np.asarray(observations, np.float32)
        if x.size % n.obs_dim or (x.ndim < 2 and x.size != n.obs_dim):
            raise ValueError(f"observations of shape {x.shape} do not hold {n.obs_dim} features")
        return torch.from_numpy(np.ascontiguousarray(x.reshape(-1, n.obs_dim))).to(n.device)

    def logits(self, observations) -> np.ndarray:
        """The network's logits [rows, A] for a batch of observations, as a host array; more
        rows than the learner's batch size go in chunks of that many."""
        n = self._native
        dev, step = self._rows(observations), n.max_act_rows
        outs = [n.act(dev[i:i + step])[0] for i in range(0, dev.shape[0], step)]
        return torch.cat(outs).cpu().numpy()

    def make_policy(self, epsilon: float = 0.0, seed: int = 0):
        """A callable for FeedForwardActor: batched observations in, int32 actions out, drawn by
        acme_epsilon_greedy's rule from (seed, the number of calls so far, row)."""
        native, rows, calls = self._native, self._rows, [0]

        def policy(batched_obs) -> np.ndarray:
            out = native.act_packed(rows(batched_obs), epsilon, seed, calls[0],
                                    with_logits=False)
            calls[0] += 1
            return out.cpu().numpy()

        return policy

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
