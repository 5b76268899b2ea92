"""The edge inputs of tests/test_acting_gpu.py against the float64 oracle alone (no GPU), as
tests/test_limits_cpu.py does for the declared-limit cases: black frames under zero biases
must produce the edge they are there for (every activation tensor identically zero, q the
head's biases), and the same frames under non-zero biases must not (every conv layer has a
positive activation), so the two GPU cases keep checking two different things.
"""

import numpy as np

from oracle import dqn_oracle as DQ
from tests import limit_cases as C
from tests import test_dqn_gpu as dqn_t

ACTS = ("x1", "x2", "x3", "h")


def _forward(name, which):
    net, params, target, frames = C.dqn_acting_edge(name)
    q, cache = DQ.forward(dqn_t._cfg(net), target if which else params, frames, np.float64)
    assert q.dtype == np.float64 and np.isfinite(q).all()
    return q, cache


def test_black_frames_with_zero_biases_zero_every_activation():
    for which in (0, 1):
        q, cache = _forward("black_zero_bias", which)
        for k in ACTS:
            assert cache[k].size and not cache[k].any(), k
        np.testing.assert_array_equal(q, np.zeros_like(q))  # the head's biases, here 0


def test_black_frames_with_biases_keep_every_layer_alive():
    for which in (0, 1):
        q, cache = _forward("black_biased", which)
        for k in ACTS:
            assert cache[k].max() > 0, k
        # Constant over the frames (each sees the same input; a BLAS may sum the rows in
        # different orders, so to float64 rounding), and not the zero answer.
        np.testing.assert_allclose(q, np.broadcast_to(q[:1], q.shape), rtol=1e-12, atol=1e-14)
        assert np.abs(q).max() > 1e-3


def test_saturated_frame_is_the_largest_input():
    net, params, _, frames = C.dqn_acting_edge("saturated")
    assert frames.shape == (1,) + net.obs_shape and frames.min() == 255
    x0 = DQ.obs_to_float(frames, np.float64)
    np.testing.assert_array_equal(x0, np.ones_like(x0))
    q, cache = _forward("saturated", 0)
    for k in ACTS:
        assert cache[k].max() > 0, k
