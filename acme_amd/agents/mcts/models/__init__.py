"""Models the MCTS agent plans with (the learned MLP model of the reference is not built)."""
from acme_amd.agents.mcts.models.base import Model  # noqa: F401
from acme_amd.agents.mcts.models.simulator import Simulator  # noqa: F401
