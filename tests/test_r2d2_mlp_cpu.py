"""R2D2MLPNetwork's tensors, the acme_r2d2_mlp_* names, what acme_r2d2_mlp_create refuses before
it touches the GPU (every field one past its limit, by error code and name), and the float64
oracle on the reference test's case."""

import ctypes
import os
import re

import numpy as np
import pytest

from acme_amd import _lib
from acme_amd.networks import R2D2MLPNetwork

NAMES = ["create", "destroy", "flat_size", "num_tensors", "tensor_info", "bind", "step", "q_step",
         "num_steps", "set_num_steps", "debug_buffer"]


def test_network_tensors_and_forget_bias():
    net = R2D2MLPNetwork(40, 20, (50, 50), 5)
    assert net.tensor_shapes() == [
        ("lstm/w_i", (40, 80)), ("lstm/w_h", (20, 80)), ("lstm/b", (80,)),
        ("mlp/linear_0/w", (20, 50)), ("mlp/linear_0/b", (50,)),
        ("mlp/linear_1/w", (50, 50)), ("mlp/linear_1/b", (50,)),
        ("mlp/linear_2/w", (50, 5)), ("mlp/linear_2/b", (5,))]
    p = net.init(3)
    assert {k: v.shape for k, v in p.items()} == dict(net.tensor_shapes())
    b = p["lstm/b"]
    assert (b[20:40] == 1).all() and not b[:20].any() and not b[40:].any()  # gates i, f, g, o
    assert np.abs(p["lstm/w_i"]).max() <= 2 / np.sqrt(40)
    assert net.obs_dtype == "float32" and net.obs_shape == (40,) and net.torso == "lstm_mlp"
    state = net.initial_state(4)
    assert state.hidden.shape == state.cell.shape == (4, 20) and not state.hidden.any()


def test_names_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "acme_hip.h")).read()
    for name in NAMES:
        sym = f"acme_r2d2_mlp_{name}"
        assert re.search(rf"\b{sym}\(", header), sym
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), sym), sym


@pytest.mark.parametrize("field,value", [
    ("obs_dim", 0), ("obs_dim", _lib.R2D2_MLP_MAX_WIDTH + 1),
    ("num_hidden", 0), ("num_hidden", _lib.R2D2_MLP_MAX_HIDDEN + 1),
    ("hidden", 0), ("hidden", _lib.R2D2_MLP_MAX_WIDTH + 1),
    ("lstm_size", 0), ("lstm_size", _lib.R2D2_MLP_MAX_LSTM + 1),
    ("num_actions", 0), ("num_actions", _lib.R2D2_MLP_MAX_ACTIONS + 1),
    ("max_batch", 0), ("max_batch", _lib.R2D2_MLP_MAX_ROWS + 1),
    ("max_sequence_length", 1), ("max_sequence_length", _lib.R2D2_MLP_MAX_T + 1),
    ("burn_in_length", -1), ("burn_in_length", 8), ("n_step", 0)])
def test_create_names_the_field_it_refuses(field, value):
    cfg = _lib.R2D2MLPConfig(
        obs_dim=4, num_actions=3, max_batch=2, max_sequence_length=9, burn_in_length=2,
        lstm_size=20, num_hidden=1, n_step=5, store_lstm_state=1, target_update_period=100,
        max_replay_size=1000, max_priority_weight=0.9, importance_sampling_exponent=0.2,
        discount=0.99, learning_rate=1e-3, adam_beta1=0.9, adam_beta2=0.999, adam_epsilon=1e-3)
    cfg.hidden[0] = 8
    if field == "hidden":
        cfg.hidden[0] = value
    else:
        setattr(cfg, field, value)
    if field == "max_sequence_length":
        cfg.burn_in_length = 0  # so that the length itself is what is refused
    h = ctypes.c_void_p()
    rc = _lib.lib().acme_r2d2_mlp_create(ctypes.byref(cfg), ctypes.byref(h))
    assert rc == _lib.ACME_ERR_INVALID
    assert field.encode() in _lib.lib().acme_last_error()


def test_oracle_on_the_reference_case():
    from tests import test_r2d2_mlp_gpu as cases
    ref = cases._reference(1)  # noqa: SLF001  (asserts the margins)
    assert np.isfinite(ref["loss"]) and ref["loss"] > 0
    assert ref["errors"].shape == (6, 10) and ref["q"].shape == (7, 10, 5)
