"""MPO agent + learner (drop-in for acme.agents.tf.mpo)."""
from acme_amd.agents.mpo.agent import MPO  # noqa: F401
from acme_amd.agents.mpo.learning import MPOLearner, MPOLoss  # noqa: F401
