"""Datasets: the learner-side iterator over replay (acme/datasets)."""
from acme_amd.datasets.reverb import make_reverb_dataset, make_dataset  # noqa: F401
from acme_amd.datasets.demonstrations import (  # noqa: F401
    DemonstrationStore, SequenceDemonstrationStore, mix_demonstrations,
    mix_sequence_demonstrations)
