"""IMPALAMLPNetwork's tensors, and what acme_impala_mlp_create refuses before it touches the GPU:
every field one past its limit, by error code and name."""

import ctypes

import numpy as np
import pytest

from acme_amd import _lib
from acme_amd.networks import IMPALAMLPNetwork


def test_network_tensors_and_forget_bias():
    net = IMPALAMLPNetwork(10, (50, 50), 20, 3)
    assert net.tensor_shapes() == [
        ("mlp/linear_0/w", (10, 50)), ("mlp/linear_0/b", (50,)),
        ("mlp/linear_1/w", (50, 50)), ("mlp/linear_1/b", (50,)),
        ("lstm/w_i", (50, 80)), ("lstm/w_h", (20, 80)), ("lstm/b", (80,)),
        ("policy_value_network/linear/w", (20, 3)), ("policy_value_network/linear/b", (3,)),
        ("policy_value_network/linear_1/w", (20, 1)), ("policy_value_network/linear_1/b", (1,))]
    p = net.init(3)
    assert {k: v.shape for k, v in p.items()} == dict(net.tensor_shapes())
    b = p["lstm/b"]
    assert (b[20:40] == 1).all() and not b[:20].any() and not b[40:].any()  # gates i, f, g, o
    assert np.abs(p["lstm/w_i"]).max() <= 2 / np.sqrt(50) and net.obs_dtype == "float32"
    state = net.initial_state(4)
    assert state.hidden.shape == state.cell.shape == (4, 20) and not state.hidden.any()


@pytest.mark.parametrize("field,value", [
    ("obs_dim", 0), ("obs_dim", _lib.IMPALA_MLP_MAX_WIDTH + 1),
    ("num_hidden", 0), ("num_hidden", _lib.IMPALA_MLP_MAX_HIDDEN + 1),
    ("hidden", 0), ("hidden", _lib.IMPALA_MLP_MAX_WIDTH + 1),
    ("lstm_size", 0), ("lstm_size", _lib.IMPALA_MLP_MAX_LSTM + 1),
    ("num_actions", 0), ("num_actions", _lib.IMPALA_MLP_MAX_ACTIONS + 1),
    ("max_batch", 0), ("max_batch", _lib.IMPALA_MLP_MAX_ROWS + 1),
    ("max_sequence_length", 1), ("max_sequence_length", _lib.IMPALA_MLP_MAX_T + 1)])
def test_create_names_the_field_it_refuses(field, value):
    cfg = _lib.IMPALAMLPConfig(
        obs_dim=4, num_actions=3, max_batch=2, max_sequence_length=3, lstm_size=20, num_hidden=1,
        discount=0.99, entropy_cost=0.01, baseline_cost=0.5, max_abs_reward=float("inf"),
        max_gradient_norm=1e10, learning_rate=1e-3, adam_beta1=0.9, adam_beta2=0.999,
        adam_epsilon=1e-8)
    cfg.hidden[0] = 8
    if field == "hidden":
        cfg.hidden[0] = value
    else:
        setattr(cfg, field, value)
    h = ctypes.c_void_p()
    rc = _lib.lib().acme_impala_mlp_create(ctypes.byref(cfg), ctypes.byref(h))
    assert rc == _lib.ACME_ERR_INVALID
    assert field.encode() in _lib.lib().acme_last_error()
