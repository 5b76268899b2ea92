"""The image-resident convolutions (gemm_p3i.h, gemm_p3c12.h, gemm_p3s.h) at the batches where
their blocks are half empty or partial, and their stage depths against one another.

Tolerances are tests/test_dqn_gpu.py's (fp32 kernels against the f64 oracle): q, loss, TD
errors and priorities rtol 1e-5, gradients conditioned on the kernel's own ReLU pattern.
"""

import numpy as np
import pytest
import torch

from oracle import dqn_oracle as O
from tests import test_dqn_gpu as dqn_t

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B", [1, 3, 5])
def test_small_batches_match_oracle(B):
    """B = 1, 3, 5: a two-frame block (conv2_fwd, conv3_dgrad, conv2_dgrad) half empty, the
    last block partial."""
    from acme_amd.networks import DQNAtariNetwork
    net = DQNAtariNetwork(18)
    rng = np.random.default_rng(100 + B)
    params, target = net.init(seed=1), net.init(seed=2)
    batch = dqn_t._batch(rng, B, net.obs_shape, net.num_actions)
    d = dqn_t._learner(net, B)
    d.set_params(params, target)
    q = torch.empty(B, net.num_actions, device="cuda")
    d.forward_backward(*dqn_t._dev(batch), q_tm1=q)
    torch.cuda.synchronize()
    masks = dqn_t._relu_masks(d, net, batch, params, B)
    out, grads = O.dqn_loss_and_grads(dqn_t._cfg(net), params, target, batch, np.float64,
                                      masks=masks)
    np.testing.assert_allclose(q.cpu().numpy(), out["q_tm1"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(d.loss.item(), out["loss"], rtol=1e-5)
    np.testing.assert_allclose(d.td_error[:B].cpu().numpy(), out["td_error"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(d.priorities[:B].cpu().numpy(), out["priorities"], rtol=1e-5,
                               atol=1e-6)
    dqn_t._check_grads(d.get_params("grads"), grads)


@pytest.mark.parametrize("B", [3, 37])
def test_stage_depth_bitwise(B):
    """ACME_V_BK32=1 at creation runs every image-resident kernel at a stage depth of 32 k;
    the default learner runs each at its own.  A stage's 32-k groups run in k order with the
    same MFMA terms, so two full steps (online forward and backward, and the target forward:
    the fused conv1 -> conv2 kernel and conv3_fwd on the side stream) agree bit for bit.
    conv3_dgrad's default depth does not divide its K (576 = 4 x 128 + 64), so the default
    learner also runs the shorter last stage."""
    from acme_amd._lib import lib
    from acme_amd.networks import DQNAtariNetwork
    net = DQNAtariNetwork(18)
    p0, t0 = net.init(3), net.init(4)
    lib().acme_tune_set(b"BK32", 1)  # read once, at the learner's creation
    try:
        a = dqn_t._learner(net, B)
    finally:
        lib().acme_tune_set(b"BK32", 0)
    b = dqn_t._learner(net, B)
    a.set_params(p0, t0)
    b.set_params(p0, t0)
    rng = np.random.default_rng(B)
    for _ in range(2):
        dev = dqn_t._dev(dqn_t._batch(rng, B, (84, 84, 4), 18))
        a.step(*dev)
        b.step(*dev)
        torch.cuda.synchronize()
        assert a.loss.item() == b.loss.item(), B
        for buf in ("grads", "params", "m", "v"):
            ga, gb = a.get_params(buf), b.get_params(buf)
            for k in ga:
                np.testing.assert_array_equal(ga[k], gb[k], err_msg=f"B={B} {buf}/{k}")
