"""DDPG agent + learner (drop-in for acme.agents.tf.ddpg)."""
from acme_amd.agents.ddpg.agent import DDPG  # noqa: F401
from acme_amd.agents.ddpg.learning import DDPGLearner  # noqa: F401
