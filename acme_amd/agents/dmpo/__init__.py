"""Distributional MPO agent + learner (drop-in for acme.agents.tf.dmpo)."""
from acme_amd.agents.dmpo.agent import DistributionalMPO  # noqa: F401
from acme_amd.agents.dmpo.learning import DistributionalMPOLearner  # noqa: F401
from acme_amd.agents.mpo.learning import MPOLoss  # noqa: F401
