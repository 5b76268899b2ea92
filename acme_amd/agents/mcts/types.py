"""Type aliases of the MCTS agent (acme/agents/tf/mcts/types.py): scalar discrete actions,
array observations, scalar rewards and discounts; an evaluation function maps an observation to
(prior probabilities over the actions, value)."""

from typing import Callable, Tuple, Union

import numpy as np

Action = Union[int, np.int32, np.int64]
Observation = np.ndarray
Reward = Union[float, np.float32, np.float64]
Discount = Union[float, np.float32, np.float64]
Probs = np.ndarray
Value = float
EvaluationFn = Callable[[Observation], Tuple[Probs, Value]]
