"""MCTS agent + AlphaZero learner (drop-in for acme.agents.tf.mcts)."""
from acme_amd.agents.mcts.acting import MCTSActor  # noqa: F401
from acme_amd.agents.mcts.agent import MCTS  # noqa: F401
from acme_amd.agents.mcts.learning import AZLearner  # noqa: F401
