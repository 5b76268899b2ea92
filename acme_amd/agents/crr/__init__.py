"""CRR learner (drop-in for acme.agents.tf.crr, which exports the learner only)."""
from acme_amd.agents.crr.learning import CRRLearner, RCRRLearner  # noqa: F401
