"""CRRLearner — drop-in for acme/agents/tf/crr/recurrent_learning.py:36-409 with stateless
(feed-forward) networks.

An offline learner: it trains from a fixed dataset of sequences and has no actor.  Same
constructor arguments and `step()` contract as RCRRLearner: one call draws a batch of [B, T]
sequences from the dataset iterator and runs the whole CRR step on the GPU (acme_crr_step: the
online policy at o_tm1 and the target policy at o_t, two sets of sampled actions through the two
critics, the categorical critic loss against the mixture of the sampled target distributions,
the advantage-weighted behaviour-cloning policy loss, per-network global-norm clipping, two
Adams, the post-update target copy), then counts and logs.  Losses are device scalars handed to
the logger; nothing synchronises the host with the device.

With stateless networks the reference's loop over t (:229-329) carries nothing from t to t + 1,
so the [B, T] sequences are flattened to R = B (T - 1) independent transitions, row
b (T - 1) + (t - 1); the summed losses are divided by T as the reference does (:331-334).
Recurrent cores are not supported.

`policy_network` / `critic_network` are descriptors from acme_amd.networks
(LayerNormMLPGaussianPolicy, DistributionalCritic).  `accelerator_strategy`, `behavior_network`
and `cwp_network` (a distribution strategy and two snapshot-only networks) must be None.
"""

from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from acme_amd import _lib
from acme_amd.agents.d4pg.learning import D4PGLearner, _learning_rate
from acme_amd.native import NativeCRR
from acme_amd.networks import DistributionalCritic, LayerNormMLPGaussianPolicy
from acme_amd.utils import counting, loggers


class CRRLearner(D4PGLearner):
    """save / restore / get_variables (the TARGET networks, recurrent_learning.py:158-161) are
    D4PGLearner's; `policy_distribution` is as on MPOLearner."""

    _algorithm = "CRR"

    def __init__(self, policy_network, critic_network, target_policy_network,
                 target_critic_network, dataset, accelerator_strategy=None,
                 behavior_network=None, cwp_network=None, policy_optimizer=None,
                 critic_optimizer=None, discount: float = 0.99, target_update_period: int = 100,
                 num_action_samples_td_learning: int = 1,
                 num_action_samples_policy_weight: int = 4,
                 baseline_reduce_function: str = "mean", clipping: bool = True,
                 policy_improvement_modes: str = "exp", ratio_upper_bound: float = 20.0,
                 beta: float = 1.0, counter: Optional[counting.Counter] = None,
                 logger: Optional[loggers.Logger] = None, checkpoint: bool = False,
                 batch_size: Optional[int] = None, seed: int = 0, device=None):
        for name, value in (("accelerator_strategy", accelerator_strategy),
                            ("behavior_network", behavior_network),
                            ("cwp_network", cwp_network)):
            if value is not None:
                raise ValueError(f"acme_amd's CRR learner does not support {name}: it must be "
                                 "None")
        for nets, kind in (((policy_network, target_policy_network), LayerNormMLPGaussianPolicy),
                           ((critic_network, target_critic_network), DistributionalCritic)):
            for net in nets:
                if not isinstance(net, kind):
                    raise ValueError(
                        "acme_amd's CRR learner takes a LayerNormMLPGaussianPolicy policy and a "
                        f"DistributionalCritic critic, not a {type(net).__name__}")
        for name, n in (("num_action_samples_td_learning", num_action_samples_td_learning),
                        ("num_action_samples_policy_weight", num_action_samples_policy_weight)):
            if not 1 <= n <= _lib.MPO_MAX_SAMPLES:
                raise ValueError(f"{name} must be in [1, {_lib.MPO_MAX_SAMPLES}]")
        self._check_networks(policy_network, critic_network, None, None, dataset, batch_size)
        # The batch size and the sequence length come from the first sample, as the reference
        # takes T (recurrent_learning.py:128-129); that sample is the first step's batch.
        self._first = next(self._iterator)
        action = self._first.data.action
        B, T = int(action.shape[0]), int(action.shape[1])
        if batch_size is not None and batch_size != B:
            raise ValueError(f"batch_size is {batch_size} but the dataset yields batches of {B}")
        self._sequence_length = T
        self._native = NativeCRR(
            obs_dim=policy_network.obs_dim, act_dim=policy_network.act_dim,
            max_batch=B * (T - 1), sequence_length=T, policy_sizes=policy_network.layer_sizes,
            critic_sizes=critic_network.layer_sizes, num_atoms=critic_network.num_atoms,
            vmin=critic_network.vmin, vmax=critic_network.vmax, discount=discount,
            target_update_period=target_update_period,
            num_action_samples_td_learning=num_action_samples_td_learning,
            num_action_samples_policy_weight=num_action_samples_policy_weight,
            baseline_reduce_function=baseline_reduce_function,
            policy_improvement_modes=policy_improvement_modes,
            ratio_upper_bound=ratio_upper_bound, beta=beta,
            policy_learning_rate=_learning_rate(policy_optimizer),
            critic_learning_rate=_learning_rate(critic_optimizer), clipping=clipping,
            init_scale=policy_network.init_scale, min_scale=policy_network.min_scale,
            seed=seed, device=device)
        self._init_params(target_policy_network, target_critic_network, seed)
        self._init_bookkeeping(counter, logger)

    @staticmethod
    def flatten(sample):
        """The R = B (T - 1) transitions (o_tm1, a_tm1, r_t, d_t, o_t) of a [B, T, ...] sequence
        sample, row b (T - 1) + (t - 1)."""
        d = sample.data
        return NativeCRR.flatten_sequences(d.observation, d.action, d.reward, d.discount)

    def _native_step(self) -> None:
        sample = self._first if self._first is not None else next(self._iterator)
        self._first = None
        self._native.step(*self.flatten(sample))

    def step(self):
        self._native_step()
        n = self._native
        self._finish_step({"critic_loss": n.critic_loss, "policy_loss": n.policy_loss,
                           "policy_loss_coef": n.policy_loss_coef})

    def policy(self, observations, use_target: bool = False) -> np.ndarray:
        """The distribution's mean."""
        return self.policy_distribution(observations, use_target)[0]

    def policy_distribution(self, observations, use_target: bool = False):
        """(mean, stddev) of the policy's diagonal Gaussian as host arrays."""
        x = torch.as_tensor(np.asarray(observations, np.float32))
        mean, stddev = self._native.policy_distribution(x, use_target)
        return mean.cpu().numpy(), stddev.cpu().numpy()


RCRRLearner = CRRLearner  # the reference's name (acme/agents/tf/crr/__init__.py)
