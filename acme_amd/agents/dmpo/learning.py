"""DistributionalMPOLearner — drop-in for acme/agents/tf/dmpo/learning.py:34-300.

Same constructor arguments and `step()` contract as the reference: MPOLearner with a
distributional critic.  One call draws a batch from the dataset iterator and runs the whole
step on the GPU (acme_dmpo_step: MPO's policy side, sampling, loss and duals; the categorical
critic over the num_samples actions of each state, the mixture of their distributions as the
bootstrap target, the categorical projection loss), then counts and logs the reference's
fetches: critic_loss, policy_loss and the MPO stats.

`policy_network` is a LayerNormMLPGaussianPolicy, `critic_network` a DistributionalCritic
(acme_amd.networks.make_dmpo_networks); the observation networks must be the identity.
`policy_loss_module` is an MPOLoss, as for MPOLearner.
"""

from __future__ import annotations

from typing import Dict

from acme_amd.agents.mpo.learning import MPOLearner, MPOLoss  # noqa: F401
from acme_amd.native import NativeDMPO
from acme_amd.networks import DistributionalCritic


class DistributionalMPOLearner(MPOLearner):
    """Everything is MPOLearner's but the native handle and the critic it is configured from."""

    _algorithm = "DMPO"
    checkpoint_subdirectory = "dmpo_learner"  # the reference Checkpointer's (learning.py:117)
    _native_type = NativeDMPO
    _critic_type = DistributionalCritic

    @staticmethod
    def _critic_config(critic_network) -> Dict:
        return dict(num_atoms=critic_network.num_atoms, vmin=critic_network.vmin,
                    vmax=critic_network.vmax)
