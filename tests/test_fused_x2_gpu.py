"""The DQN step's forwards with conv3 inside conv2's launch (csrc/gemm_p3c12.h: conv1 -> conv2
-> conv3 for the target forward, conv2 -> conv3 for the online one; x2 stays in LDS wherever
the backward does not read it) against the separate conv3_fwd launches (a learner created
with ACME_V_FUSE_X2=0).  The fused kernels keep every sum's order and scale, so every result
is compared bit for bit: loss, TD errors, priorities, the target's q values, gradients,
parameters, target, both Adam moments and the plane scale records.

Learners with FUSE_X2 = 1 (target only), 2 (online only) and 3 (both) against 0, three full
steps of which one copies the target, at B = 1 and 3 (a two-frame online block holds one frame
whose x2 goes to HBM and one whose x2 does not) and B = 37 (the x1-fed blocks of the unfused
kernels are partial), and once more with the fused learner's image-resident kernels at a 32-k
stage depth (ACME_V_BK32=1).  Equal conv3 gradients show that the o_tm1 rows' stored x2 is
right, equal loss that the rows that only lived in LDS are.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

A = 18
MAXB = 37
FUSE_X2_DEFAULT = 3  # the shipped default (csrc/torso.h kFuseX2Default)
_pairs = {}


def _make(fuse, bk32):
    from acme_amd._lib import lib
    from acme_amd.native import NativeDQN
    lib().acme_tune_set(b"FUSE_X2", fuse)  # both read once, at creation
    lib().acme_tune_set(b"BK32", 1 if bk32 else 0)
    try:
        return NativeDQN(network="nature", num_actions=A, max_batch=MAXB, obs_dtype="uint8",
                         target_update_period=3)
    finally:
        lib().acme_tune_set(b"FUSE_X2", FUSE_X2_DEFAULT)
        lib().acme_tune_set(b"BK32", 0)


def _pair(fuse, bk32=False):
    """(fused learner, separate-launch learner) per (FUSE_X2, BK32), shared by the cases: the
    two always take the same calls, so their plane scales have the same history and they stay
    comparable from case to case."""
    key = (fuse, bk32)
    if key not in _pairs:
        _pairs[key] = (_make(fuse, bk32), _make(0, False))
    return _pairs[key]


def _batch(rng, B):
    o1 = rng.integers(0, 256, (B, 84, 84, 4), dtype=np.uint8)
    o2 = rng.integers(0, 256, (B, 84, 84, 4), dtype=np.uint8)
    rr = (rng.standard_normal(B) * 1.5).astype(np.float32)
    dd = np.where(rng.random(B) < 0.2, 0.0, 0.99 ** 4).astype(np.float32)
    vals = (o1, rng.integers(0, A, B).astype(np.int32), rr, dd, o2, rng.uniform(1e-6, 1e-3, B))
    return [torch.as_tensor(v).cuda().contiguous() for v in vals]


def _assert_same(a, b, B, tag):
    torch.cuda.synchronize()
    assert a.loss.item() == b.loss.item(), tag
    assert np.isfinite(a.loss.item()), tag
    assert torch.equal(a.td_error[:B], b.td_error[:B]), tag
    assert torch.equal(a.priorities[:B], b.priorities[:B]), tag
    np.testing.assert_array_equal(a.debug_buffer("q_tg")[:B * A], b.debug_buffer("q_tg")[:B * A],
                                  err_msg=f"{tag} q_tg")
    for buf in ("grads", "params", "target", "m", "v"):
        ga, gb = a.get_params(buf), b.get_params(buf)
        for k in ga:
            np.testing.assert_array_equal(ga[k], gb[k], err_msg=f"{tag} {buf}/{k}")
    np.testing.assert_array_equal(a.scale_state(), b.scale_state(), err_msg=f"{tag} scales")


def _run(fused, ref, B, seed, per_step):
    from acme_amd.networks import DQNAtariNetwork
    net = DQNAtariNetwork(A)
    p0, t0 = net.init(seed), net.init(seed + 1)
    fused.set_params(p0, t0)
    ref.set_params(p0, t0)
    rng = np.random.default_rng(100 * B + seed)
    t_before = ref.get_params("target")
    n_fused, n_ref = fused.fused_x2_launches(), ref.fused_x2_launches()
    for step in range(3):  # the learners' step counts differ from case to case: a target copy
        dev = _batch(rng, B)  # falls on one of any three consecutive steps
        fused.step(*dev)
        ref.step(*dev)
        _assert_same(fused, ref, B, (B, step))
    # (a step may be issued more than once: the first steps calibrate the plane scales)
    done = fused.fused_x2_launches() - n_fused
    assert done >= 3 * per_step and done % per_step == 0, "conv3 did not run fused"
    assert ref.fused_x2_launches() == n_ref == 0
    t_after = ref.get_params("target")
    assert any(not np.array_equal(t_before[k], t_after[k]) for k in t_before), "no target copy"
    g = ref.get_params("grads")
    assert np.abs(g["atari_torso/conv2_d_2/w"]).max() > 0, "no conv3 gradient"


@pytest.mark.parametrize("fuse", [1, 2, 3])
@pytest.mark.parametrize("B", [1, 3, 37])
def test_fused_equals_separate_launches(B, fuse):
    _run(*_pair(fuse), B, 3, bin(fuse).count("1"))


def test_fused_at_bk32_equals_separate_launches():
    _run(*_pair(3, bk32=True), 37, 5, 2)
