"""DDPGLearner — drop-in for acme/agents/tf/ddpg/learning.py:36-260.

Same constructor arguments and `step()` contract: one call draws a batch from the dataset
iterator and runs the whole DDPG step on the GPU (acme_ddpg_step: start-of-step target
copy, target/online policy and critic forwards, TD loss mean(0.5 (r + discount d q_t -
q_tm1)^2), dpg loss with dqda norm clipping, per-network global-norm clipping, two Adams),
then counts and logs.  Losses are device scalars handed to the logger; nothing synchronises
the host with the device.

`policy_network` / `critic_network` are descriptors from acme_amd.networks
(LayerNormMLPPolicy, LayerNormMLPCritic); the observation networks must be the identity.
Everything but the construction of the native learner (step, policy, get_variables, save /
restore) is D4PGLearner's: the two native handles have one surface.
"""

from __future__ import annotations

from typing import Optional

from acme_amd.agents.d4pg.learning import D4PGLearner, _learning_rate
from acme_amd.native import NativeDDPG
from acme_amd.utils import counting, loggers


class DDPGLearner(D4PGLearner):

    _algorithm = "DDPG"

    def __init__(self, policy_network, critic_network, target_policy_network,
                 target_critic_network, discount: float, target_update_period: int, dataset,
                 observation_network=lambda x: x, target_observation_network=lambda x: x,
                 policy_optimizer=None, critic_optimizer=None, clipping: bool = True,
                 counter: Optional[counting.Counter] = None,
                 logger: Optional[loggers.Logger] = None, checkpoint: bool = True,
                 batch_size: Optional[int] = None, seed: int = 0, device=None):
        B = self._check_networks(policy_network, critic_network, observation_network,
                                 target_observation_network, dataset, batch_size)
        self._native = NativeDDPG(
            obs_dim=policy_network.obs_dim, act_dim=policy_network.act_dim, max_batch=B,
            policy_sizes=policy_network.layer_sizes, critic_sizes=critic_network.layer_sizes,
            action_min=policy_network.action_min, action_max=policy_network.action_max,
            discount=discount, target_update_period=target_update_period,
            policy_learning_rate=_learning_rate(policy_optimizer),
            critic_learning_rate=_learning_rate(critic_optimizer),
            clipping=clipping, device=device)
        self._init_params(target_policy_network, target_critic_network, seed)
        self._init_bookkeeping(counter, logger)
