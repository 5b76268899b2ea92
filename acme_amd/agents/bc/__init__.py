"""BC learner (drop-in for acme.agents.tf.bc, which exports the learner only)."""
from acme_amd.agents.bc.learning import BCLearner  # noqa: F401
