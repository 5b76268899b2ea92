"""Models the MCTS agent plans with: a copy of the true environment, or a learned MLP model."""
from acme_amd.agents.mcts.models.base import Model  # noqa: F401
from acme_amd.agents.mcts.models.mlp import MLPModel  # noqa: F401
from acme_amd.agents.mcts.models.simulator import Simulator  # noqa: F401
