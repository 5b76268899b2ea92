"""DQfD agent (drop-in for acme.agents.tf.dqfd): DQN with demonstrations in every batch."""
from acme_amd.agents.dqfd.agent import DQfD  # noqa: F401
from acme_amd.agents.dqfd.demonstrations import DemonstrationRecorder  # noqa: F401
