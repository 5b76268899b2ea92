"""The flat-buffer layout every native learner builds through the shared add_tensor, and the
head-kind check of the actor-critic step exports.

Names and shapes are pinned by the learners' own suites; the offsets, which the data-parallel
bucket and MPO's dual offset are computed from, are pinned here."""

import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

AC = dict(obs_dim=3, act_dim=2, max_batch=4, policy_sizes=(8, 4), critic_sizes=(8, 4))


def _dqn_mlp():
    from acme_amd.native import NativeDQN
    return NativeDQN(network="mlp", num_actions=3, max_batch=4, obs_dtype="float32", obs_dim=6,
                     hidden=(16, 16))


def _dqn_nature():
    from acme_amd.native import NativeDQN
    return NativeDQN(network="nature", num_actions=18, max_batch=4, obs_dtype="uint8")


def _d4pg():
    from acme_amd.native import NativeD4PG
    return NativeD4PG(num_atoms=5, **AC)


def _ddpg():
    from acme_amd.native import NativeDDPG
    return NativeDDPG(**AC)


def _mpo():
    from acme_amd.native import NativeMPO
    return NativeMPO(num_samples=2, **AC)


def _impala():
    from acme_amd.native import NativeIMPALA
    return NativeIMPALA(num_actions=5, max_batch=3, max_sequence_length=2, torso="flat",
                        obs_dim=12, lstm_size=8, head_size=4)


def _r2d2():
    from acme_amd.native import NativeR2D2
    return NativeR2D2(num_actions=5, max_batch=3, max_sequence_length=6, burn_in_length=2,
                      torso="flat", obs_dim=12, lstm_size=16, head_size=8, n_step=3)


def _align64(x: int) -> int:
    return (x + 63) & ~63


@pytest.mark.parametrize("make", [_dqn_mlp, _dqn_nature, _d4pg, _ddpg, _mpo, _impala, _r2d2],
                         ids=lambda f: f.__name__.lstrip("_"))
def test_tensor_offsets_are_packed_and_aligned(make):
    n = make()
    names = [t[0] for t in n.tensors]
    offsets = [t[1] for t in n.tensors]
    numels = [int(np.prod(t[2])) for t in n.tensors]
    assert len(offsets) >= 2
    assert offsets[0] == 0
    assert all(a < b for a, b in zip(offsets, offsets[1:])), offsets
    for i in range(len(offsets) - 1):
        assert offsets[i + 1] == _align64(offsets[i] + numels[i]), (names[i], offsets, numels)
    assert n.flat_size == _align64(offsets[-1] + numels[-1])
    if hasattr(n, "policy_size"):  # the actor-critic kinds: policy group, critic group[, duals]
        first = lambda prefix: next(o for name, o in zip(names, offsets)  # noqa: E731
                                    if name.startswith(prefix))
        assert n.policy_size == first("critic/")
        if hasattr(n, "dual_offset"):
            assert n.dual_offset == first("mpo/")


def _d4pg_batch(n, B=4):
    from acme_amd import _lib
    from acme_amd._lib import ptr
    g = torch.Generator(device="cpu").manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g).cuda().contiguous()  # noqa: E731
    keep = [r(B, n.obs_dim), r(B, n.act_dim), r(B), torch.full((B,), 0.99).cuda(),
            r(B, n.obs_dim)]
    b = _lib.D4PGBatch()
    b.o_tm1, b.a_tm1, b.r_t, b.d_t, b.o_t = (ptr(t) for t in keep)
    b.batch = B
    return b, keep


def test_step_exports_reject_the_wrong_head_kind():
    from acme_amd import _lib
    from acme_amd._lib import lib, stream_ptr
    mpo, ddpg = _mpo(), _ddpg()
    for n in (mpo, ddpg):
        n.params.normal_(generator=torch.Generator(device="cuda").manual_seed(1))
    before = [n.params.clone() for n in (mpo, ddpg)]
    torch.cuda.synchronize()

    # D4PG's step on an MPO learner would run over buffers MPO sizes differently.
    b, keep = _d4pg_batch(mpo)
    out = _lib.D4PGOutputs()
    rc = lib().acme_d4pg_step(mpo._h, ctypes.byref(b), ctypes.byref(out), stream_ptr())
    assert rc == _lib.ACME_ERR_INVALID
    assert b"MPO" in lib().acme_last_error()

    mb = _lib.MPOBatch()
    mb.o_tm1, mb.a_tm1, mb.r_t, mb.d_t, mb.o_t = b.o_tm1, b.a_tm1, b.r_t, b.d_t, b.o_t
    mb.batch = b.batch
    mout = _lib.MPOOutputs()
    rc = lib().acme_mpo_step(ddpg._h, ctypes.byref(mb), ctypes.byref(mout), stream_ptr())
    assert rc == _lib.ACME_ERR_INVALID

    # Nothing was launched or counted.
    torch.cuda.synchronize()
    for n, p in zip((mpo, ddpg), before):
        assert n.num_steps == 0
        assert torch.equal(n.params, p)
    del keep
