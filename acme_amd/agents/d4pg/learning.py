"""D4PGLearner — drop-in for acme/agents/tf/d4pg/learning.py:35-270.

Same constructor arguments and `step()` contract: one call draws a batch from the
dataset iterator and runs the whole D4PG step on the GPU (acme_d4pg_step: start-of-step
target copy, target/online policy and critic forwards, categorical L2-projection loss,
dpg loss with dqda norm clipping, per-network global-norm clipping, two Adams), then
counts and logs.  Losses are device scalars handed to the logger; nothing synchronises
the host with the device.

`policy_network` / `critic_network` are descriptors from acme_amd.networks
(LayerNormMLPPolicy, DistributionalCritic); the observation networks must be the
identity (the reference's control-suite setup, examples/control_suite/run_d4pg.py:66).
Optimizers are anything with a `learning_rate` (acme_amd.optimizers.Adam); the default is
Adam(1e-4) for both (learning.py:113-114).
"""

from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from acme_amd.agents._learner import Learner
from acme_amd.native import NativeD4PG
from acme_amd.utils import counting, loggers


def _is_identity(fn) -> bool:
    if fn is None or fn == "identity":
        return True
    try:
        x = np.arange(3.0)
        return fn(x) is x
    except Exception:
        return False


def _learning_rate(optimizer, default: float = 1e-4) -> float:
    return float(getattr(optimizer, "learning_rate", default)) if optimizer is not None else default


class D4PGLearner(Learner):
    """Also the base of DDPGLearner and MPOLearner, which build another native handle from
    the same pieces (`_check_networks`, `_init_params`, Learner's `_init_bookkeeping`)."""

    _algorithm = "D4PG"  # names the learner in messages

    def __init__(self, policy_network, critic_network, target_policy_network,
                 target_critic_network, discount: float, target_update_period: int, dataset,
                 observation_network=lambda x: x, target_observation_network=lambda x: x,
                 policy_optimizer=None, critic_optimizer=None, clipping: bool = True,
                 counter: Optional[counting.Counter] = None,
                 logger: Optional[loggers.Logger] = None, checkpoint: bool = True,
                 batch_size: Optional[int] = None, seed: int = 0, device=None):
        B = self._check_networks(policy_network, critic_network, observation_network,
                                 target_observation_network, dataset, batch_size)
        self._native = NativeD4PG(
            obs_dim=policy_network.obs_dim, act_dim=policy_network.act_dim, max_batch=B,
            policy_sizes=policy_network.layer_sizes, critic_sizes=critic_network.layer_sizes,
            num_atoms=critic_network.num_atoms, vmin=critic_network.vmin,
            vmax=critic_network.vmax, action_min=policy_network.action_min,
            action_max=policy_network.action_max, discount=discount,
            target_update_period=target_update_period,
            policy_learning_rate=_learning_rate(policy_optimizer),
            critic_learning_rate=_learning_rate(critic_optimizer),
            clipping=clipping, device=device)
        self._init_params(target_policy_network, target_critic_network, seed)
        self._init_bookkeeping(counter, logger)

    def _check_networks(self, policy_network, critic_network, observation_network,
                        target_observation_network, dataset, batch_size) -> int:
        """The identity and size checks; keeps the networks and the dataset iterator and
        returns the batch size the native learner is built for."""
        if not (_is_identity(observation_network) and _is_identity(target_observation_network)):
            raise ValueError(f"acme_amd's {self._algorithm} learner supports identity "
                             "observation networks (flat observations) only")
        if critic_network.obs_dim != policy_network.obs_dim or \
                critic_network.act_dim != policy_network.act_dim:
            raise ValueError("policy and critic disagree on observation / action sizes")
        self._policy_network = policy_network
        self._critic_network = critic_network
        self._iterator = iter(dataset)
        return batch_size or getattr(dataset, "batch_size", None) or 256

    def _init_params(self, target_policy_network, target_critic_network, seed: int) -> None:
        """Online and target parameters from init(seed + 0..3), into the native buffers."""
        init = dict(self._policy_network.init(seed))
        init.update(self._critic_network.init(seed + 1))
        tinit = dict(target_policy_network.init(seed + 2))
        tinit.update(target_critic_network.init(seed + 3))
        self._native.set_params(init, tinit)

    def _native_step(self) -> None:
        """Draws a batch and runs the native step on it."""
        sample = next(self._iterator)
        o_tm1, a_tm1, r_t, d_t, o_t = sample.data[:5]
        B = int(r_t.shape[0])
        f = lambda x: x.reshape(B, -1).to(torch.float32).contiguous()  # noqa: E731
        self._native.step(f(o_tm1), f(a_tm1), f(r_t).reshape(B), f(d_t).reshape(B), f(o_t))

    def step(self):
        self._native_step()
        self._finish_step({"critic_loss": self._native.critic_loss,
                           "policy_loss": self._native.policy_loss})

    def policy(self, observations, use_target: bool = False) -> np.ndarray:
        x = torch.as_tensor(np.asarray(observations, np.float32))
        return self._native.policy(x, use_target).cpu().numpy()

    def get_variables(self, names: List[str]) -> List[Dict[str, np.ndarray]]:
        # As the TF learner (learning.py:117-122, 269-270): 'critic' -> target critic,
        # 'policy' -> target (observation + policy) network; host copies.
        target = self._native.get_params("target")
        out = []
        for name in names:
            if name not in ("critic", "policy"):
                raise KeyError(name)
            out.append({k: v for k, v in target.items() if k.startswith(name + "/")})
        return out

    def save(self) -> Dict:
        n = self._native
        return {"params": n.get_params("params"), "target": n.get_params("target"),
                "optimizer": {"m": n.get_params("m"), "v": n.get_params("v")},
                "num_steps": n.num_steps}

    def restore(self, state: Dict):
        n = self._native
        n.set_params(state["params"], state["target"])
        self._restore_moments(state["optimizer"])
        n.num_steps = int(state["num_steps"])
