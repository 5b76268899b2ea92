"""The online head inside the loss launch (kernels.hip dqn_head_loss_dz_kernel) against the
launches it replaced, fc_head_fwd + loss_head_dz (a learner created with ACME_V_HEAD_FUSE=0):
the same sums in the same order, so every result is compared bit for bit.

Cases: B = 1, 3 and 37 over three steps, in the TF and the JAX loss forms; every batch of more
than one row has a row with action 0 and one with action A - 1, a row with d = 0, and its
smallest probability (the importance-weight normaliser) in the last row.  test_tied_selector:
two advantage columns made identical and largest, so every selector row's maximum is tied and
the first index must win.

Compared after every step: parameters, target, Adam moments, loss, TD errors, the step's
priorities, the online q rows (b and B + b), and the table's raw priorities and tree levels.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

A = 18
_pairs = {}


def _make(max_batch, fuse, semantics):
    from acme_amd._lib import lib
    from acme_amd.native import NativeDQN
    lib().acme_tune_set(b"HEAD_FUSE", 1 if fuse else 0)  # read once, at creation
    try:
        return NativeDQN(network="nature", num_actions=A, max_batch=max_batch, obs_dtype="uint8",
                         target_update_period=3, semantics=semantics)
    finally:
        lib().acme_tune_set(b"HEAD_FUSE", 1)  # the shipped default


def _pair(semantics):
    if semantics not in _pairs:
        _pairs[semantics] = (_make(37, True, semantics), _make(37, False, semantics))
    return _pairs[semantics]


def _batch(rng, B):
    o1 = rng.integers(0, 256, (B, 84, 84, 4), dtype=np.uint8)
    o2 = rng.integers(0, 256, (B, 84, 84, 4), dtype=np.uint8)
    a = rng.integers(0, A, B).astype(np.int32)
    r = (rng.standard_normal(B) * 1.5).astype(np.float32)
    d = np.full(B, 0.99 ** 4, np.float32)
    probs = rng.uniform(1e-5, 1e-3, B)
    a[0] = 0          # B = 1: action 0, then A - 1 on the next step (see _steps)
    d[B // 2] = 0.0   # a terminal row
    if B > 1:
        a[-1] = A - 1
        probs[-1] = 1e-6  # the smallest probability, in the last row
    return [o1, a, r, d, o2, probs]


def _tables():
    from acme_amd.native import NativeReplay
    n = 75
    rows = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)
    tables = [NativeReplay(65, [4], prioritized=True, priority_exponent=0.6, seed=77)
              for _ in range(2)]
    for t in tables:
        t.insert([rows], np.linspace(0.5, 2.0, n))
    torch.cuda.synchronize()
    return tables


def _assert_same(a, b, ta, tb, B, tag):
    torch.cuda.synchronize()
    assert a.loss.item() == b.loss.item(), tag
    assert torch.equal(a.priorities[:B], b.priorities[:B]), tag
    assert torch.equal(a.td_error[:B], b.td_error[:B]), tag
    qa, qb = (x.debug_buffer("q_on")[:2 * B * A] for x in (a, b))
    np.testing.assert_array_equal(qa, qb, err_msg=f"{tag} q")
    for buf in ("params", "target", "m", "v"):
        ga, gb = a.get_params(buf), b.get_params(buf)
        for k in ga:
            np.testing.assert_array_equal(ga[k], gb[k], err_msg=f"{tag} {buf}/{k}")
    np.testing.assert_array_equal(ta.debug_state()["raw"], tb.debug_state()["raw"], err_msg=str(tag))
    for i, (x, y) in enumerate(zip(ta.debug_levels(), tb.debug_levels())):
        np.testing.assert_array_equal(x, y, err_msg=f"{tag} level {i}")
    return qa.reshape(2 * B, A)


def _steps(a, b, B, p0, t0, seed, steps=3):
    a.set_params(p0, t0)
    b.set_params(p0, t0)
    ta, tb = _tables()
    rng = np.random.default_rng(seed)
    q = None
    for step in range(steps):
        keys = ta.sample(B, step)["keys"]
        assert torch.equal(keys, tb.sample(B, step)["keys"])
        vals = _batch(rng, B)
        if B == 1 and step == 1:
            vals[1][0] = A - 1
        dev = [torch.as_tensor(v).cuda().contiguous() for v in vals]
        a.step(*dev, priority_update=(ta.handle, keys))
        b.step(*dev, priority_update=(tb.handle, keys))
        q = _assert_same(a, b, ta, tb, B, (B, step))
    return q


@pytest.mark.parametrize("semantics", ["tf", "jax"])
@pytest.mark.parametrize("B", [1, 3, 37])
def test_fused_head_equals_separate_launches(B, semantics):
    from acme_amd.networks import DQNAtariNetwork
    net = DQNAtariNetwork(A)
    a, b = _pair(semantics)
    _steps(a, b, B, net.init(7), net.init(8), seed=10 * B + (semantics == "jax"))


def test_tied_selector():
    """Advantage columns 5 and 11 identical with the largest bias: q[:, 5] == q[:, 11] is every
    row's maximum, and tf.argmax takes index 5."""
    from acme_amd.networks import DQNAtariNetwork
    net = DQNAtariNetwork(A)
    p0, t0 = net.init(9), net.init(10)
    tied = 0
    for k, v in p0.items():
        if "mlp_1/linear_1" in k and v.shape[-1] == A:  # the advantage head's w [H, A] / b [A]
            v = v.copy()
            v[..., 11] = v[..., 5]
            if v.ndim == 1:
                v[5] = v[11] = 50.0
            p0[k] = v
            tied += 1
    assert tied == 2, sorted(p0)
    a, b = _pair("tf")
    q = _steps(a, b, 3, p0, t0, seed=99, steps=1)
    assert (q[:, 5] == q[:, 11]).all() and (q.argmax(axis=1) == 5).all(), q
