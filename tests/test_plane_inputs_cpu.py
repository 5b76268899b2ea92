"""The inputs of tests/test_plane_inputs_gpu.py against the float64 oracle alone (no GPU), as
tests/test_acting_cpu.py does for the acting edges: each schedule's frames must produce the
edge they are there for, and each pair of the guard-window cases must move the gradients by
the factor the window's arithmetic assumes.
"""

import numpy as np
import pytest

from oracle import dqn_oracle as DQ
from tests import limit_cases as C
from tests import test_dqn_gpu as dqn_t

ACTS = ("x1", "x2", "x3", "h")
HEAD_BIASES = ("duelling_q_network/mlp/linear_1/b", "duelling_q_network/mlp_1/linear_1/b")


def _step(net, params, target, batch):
    out, grads = DQ.dqn_loss_and_grads(dqn_t._cfg(net), params, target, batch, np.float64)
    assert np.isfinite(out["loss"])
    return out, grads


def test_every_schedule_is_batches_of_five_uint8_stacks():
    for name in C.DQN_PLANE_SCHEDULES:
        net, _, _, batches, _ = C.dqn_plane_schedule(name)
        assert len(batches) == 3, name
        for b in batches:
            for k in ("o_tm1", "o_t"):
                assert b[k].dtype == np.uint8 and b[k].shape == (5,) + net.obs_shape, (name, k)


def test_black_first_zeroes_every_activation_and_weight_gradient():
    net, params, target, batches, _ = C.dqn_plane_schedule("black_first")
    black = batches[0]
    assert not black["o_tm1"].any() and not black["o_t"].any()
    out, grads = _step(net, params, target, black)
    for k in ACTS:
        assert out["cache"][k].size and not out["cache"][k].any(), k
    for k in ("dzh", "dz3", "dz2", "dz1"):  # the input-gradient chain below the head dZ
        assert out["cache"][k].size and not out["cache"][k].any(), k
    for k, g in grads.items():  # the head's bias gradients are sums of the head dZ alone
        assert (np.abs(g).max() > 0) == (k in HEAD_BIASES), k
    assert np.abs(out["td_error"]).max() > 0  # r + 0 - 0: the rewards alone
    # The batches after it are live.
    out2, grads2 = _step(net, params, target, batches[1])
    assert all(out2["cache"][k].max() > 0 for k in ACTS)
    assert all(np.abs(g).max() > 0 for g in grads2.values())


def test_black_between_has_its_black_batch_in_the_middle():
    net, params, target, batches, lr = C.dqn_plane_schedule("black_between")
    assert lr == 0.0  # the biases stay zero: the black batch is black_first's, mid-run
    assert batches[0]["o_tm1"].any() and batches[2]["o_tm1"].any()
    assert not batches[1]["o_tm1"].any() and not batches[1]["o_t"].any()
    out, _ = _step(net, params, target, batches[1])
    for k in ACTS:
        assert not out["cache"][k].any(), k


def test_black_after_update_leaves_activations_far_below_the_window():
    """One update at the default learning rate moves every bias by about that rate (Adam's
    first step), so the black batch's x1 is those biases alone: positive, and more than 2^8
    below the first batch's maximum, where the guard must call an underflow whatever the
    mantissa (limit_cases.DQN_WINDOW_JUMPS)."""
    net, params, target, batches, lr = C.dqn_plane_schedule("black_after_update")
    assert lr == 1e-3 and not batches[1]["o_tm1"].any() and not batches[1]["o_t"].any()
    cfg = dqn_t._cfg(net, learning_rate=lr)
    z = {k: np.zeros_like(v) for k, v in params.items()}
    state = dict(params=params, target=target, m=z, v=dict(z), num_steps=0)
    out, _, state = DQ.dqn_step(cfg, state, batches[0], np.float64)
    live = np.abs(out["cache"]["x1"]).max()
    _, cache = DQ.forward(cfg, state["params"], batches[1]["o_tm1"], np.float64)
    assert 0 < cache["x1"].max() < 2.0 ** -8 * live


def test_black_biased_keeps_every_layer_alive():
    net, params, target, batches, _ = C.dqn_plane_schedule("black_biased")
    assert not batches[0]["o_tm1"].any() and not batches[0]["o_t"].any()
    out, grads = _step(net, params, target, batches[0])
    for k in ACTS:
        assert out["cache"][k].max() > 0, k
    # Black frames reach conv1 as zeros: its weight gradient is zero, its bias gradient not.
    assert not grads["atari_torso/conv2_d/w"].any()
    assert np.abs(grads["atari_torso/conv2_d/b"]).max() > 0
    assert np.abs(grads["atari_torso/conv2_d_1/w"]).max() > 0


def test_sparse_frames_are_mostly_black_and_keep_every_layer_alive():
    net, params, target, batches, _ = C.dqn_plane_schedule("sparse")
    for b in batches:
        for k in ("o_tm1", "o_t"):
            assert np.mean(b[k] == 0) >= 0.9, k
            lit = b[k][b[k] > 0]
            assert lit.size and lit.min() >= 128
        # o_t is o_tm1 one stack position on.
        np.testing.assert_array_equal(b["o_t"][..., :3], b["o_tm1"][..., 1:])
        assert (b["o_t"][..., 3] != b["o_tm1"][..., 3]).any()
        out, grads = _step(net, params, target, b)
        for k in ACTS:
            assert out["cache"][k].max() > 0, k
        assert all(np.abs(g).max() > 0 for g in grads.values())


def test_dark_then_saturated_moves_x1_by_two_to_the_seven_to_eight():
    net, params, target, batches, _ = C.dqn_plane_schedule("dark_then_saturated")
    assert batches[0]["o_tm1"].max() == 1 and batches[2]["o_tm1"].max() == 1
    assert batches[1]["o_tm1"].min() == 255 and batches[1]["o_t"].min() == 255
    cfg = dqn_t._cfg(net)
    for p in (params, target):  # the online activations and the target's T records
        amax = [np.abs(DQ.forward(cfg, p, b["o_t"], np.float64)[1]["x1"]).max() for b in batches]
        for dark in (amax[0], amax[2]):
            assert 2.0 ** 7 <= amax[1] / dark <= 2.0 ** 8, (amax[1] / dark)


def test_uncalibrated_case_underflows_at_scale_one():
    """The guard calls an underflow when a tensor's maximum times its scale is below 1
    (rescale.h): at the restored scale 1 that is x3's and the hidden layer's maxima
    themselves."""
    net, params, target, batch = C.dqn_uncalibrated_case()
    out, _ = _step(net, params, target, batch)
    for k in ("x3", "h"):
        assert 0 < out["cache"][k].max() < 1, k


@pytest.mark.parametrize("name", sorted(C.DQN_WINDOW_JUMPS))
def test_window_pair_scales_every_gradient_by_g(name):
    net, params, target, first, second, g = C.dqn_window_case(name)
    r0, r1 = float(first["r_t"][0]), float(second["r_t"][0])
    assert r1 == g * r0 and (first["r_t"] == r0).all() and (second["r_t"] == r1).all()
    for k in ("o_tm1", "o_t", "a_tm1", "d_t", "probabilities"):
        np.testing.assert_array_equal(first[k], second[k])
    assert not first["d_t"].any()
    o1, g1 = _step(net, params, target, first)
    o2, g2 = _step(net, params, target, second)
    assert np.abs(o1["q_tm1"]).max() <= 2.0 ** -7 * min(r0, r1)
    assert np.abs(o1["td_error"]).max() < 1 and np.abs(o2["td_error"]).max() < 1
    for k in g1:
        a1, a2 = np.abs(g1[k]).max(), np.abs(g2[k]).max()
        assert a1 > 0, k
        assert abs(a2 / a1 / g - 1.0) <= 0.01, (k, a2 / a1, g)
