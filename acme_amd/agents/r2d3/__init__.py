"""R2D3: the R2D2 learner fed by replay sequences with demonstration sequences mixed in."""
from acme_amd.agents.r2d3.agent import R2D3  # noqa: F401
