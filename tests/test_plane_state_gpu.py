"""The plane-scale and step-guard state the DQN, IMPALA and R2D2 learners share
(csrc/plane_guard.h behind acme_*_scale_state / _set_scale_state / _set_num_steps): a restored
IMPALA scale state resumes bit for bit, every learner refuses a malformed scale state, the
learners without planes have none, and R2D2's step count still moves Adam's."""

import numpy as np
import pytest
import torch

from oracle import impala_oracle as IO
from tests import test_impala_gpu as TI

pytestmark = pytest.mark.gpu


def _dqn(network):
    from acme_amd.native import NativeDQN
    if network == "nature":  # uint8 frames: the plane path
        return NativeDQN(network="nature", num_actions=18, max_batch=4, obs_dtype="uint8")
    return NativeDQN(network="mlp", num_actions=3, max_batch=4, obs_dtype="float32", obs_dim=6,
                     hidden=(8,))


def _impala(torso):
    from acme_amd.native import NativeIMPALA
    if torso == "atari":  # B * T = 64 frames: the fewest that take the plane path
        return NativeIMPALA(num_actions=18, max_batch=4, max_sequence_length=16, torso="atari",
                            lstm_size=256, head_size=64)
    return NativeIMPALA(num_actions=5, max_batch=2, max_sequence_length=4, torso="flat",
                        obs_dim=12, lstm_size=8, head_size=4)


def _r2d2(torso):
    from acme_amd.native import NativeR2D2
    if torso == "atari":
        return NativeR2D2(num_actions=18, max_batch=3, max_sequence_length=6, burn_in_length=2,
                          torso="atari", lstm_size=512, head_size=64)
    return NativeR2D2(num_actions=5, max_batch=2, max_sequence_length=4, burn_in_length=1,
                      torso="flat", obs_dim=12, lstm_size=8, head_size=8)


def test_impala_scale_state_restore():
    """Two steps on learner A (Atari torso, 64 frames: the plane path), then its parameters,
    Adam moments, counts and scale state copied into a fresh learner B (set_params, then
    set_scale_state): one more step on the same batch gives the same bits in both, and
    neither skips a step."""
    B, T = 4, 16
    cfg = IO.IMPALAConfig(num_actions=18, torso="atari", lstm_size=256, head_size=64,
                          entropy_cost=0.01, baseline_cost=0.5)
    a = TI._native(cfg, B, T)
    a.set_params(TI._params(cfg, 11))
    for seed in (12, 13):
        TI._run(a, TI._batch(cfg, B, T, seed))
    state = a.scale_state()
    assert state.size > 0 and state.size % 4 == 0
    b = TI._native(cfg, B, T)
    b.set_params(a.get_params("params"))
    b.m.copy_(a.m)
    b.v.copy_(a.v)
    b.num_steps = a.num_steps
    b.applied_steps = a.applied_steps
    b.set_scale_state(state)
    np.testing.assert_array_equal(b.scale_state(), state)
    batch = TI._batch(cfg, B, T, 14)
    for n in (a, b):
        TI._run(n, batch)
    for buf in ("params", "m", "v"):
        np.testing.assert_array_equal(getattr(b, buf).cpu().numpy(), getattr(a, buf).cpu().numpy(),
                                      err_msg=buf)
    np.testing.assert_array_equal(b.metrics.cpu().numpy(), a.metrics.cpu().numpy())
    assert a.skipped_steps == 0 and b.skipped_steps == 0
    assert a.guard_state()["applied"] == b.guard_state()["applied"] == 3


@pytest.mark.parametrize("make,kind", [(_dqn, "nature"), (_impala, "atari"), (_r2d2, "atari")])
def test_set_scale_state_checks_its_argument(make, kind):
    """At each learner's smallest plane-path shape: one float too few, or an entry that is no
    power of two, is ACME_ERR_INVALID (ValueError); the state itself is accepted."""
    n = make(kind)
    state = n.scale_state()
    assert state.size > 0 and state.size % 4 == 0
    with pytest.raises(ValueError):
        n.set_scale_state(state[:-1])
    bad = state.copy()
    bad[1] = 3.0
    with pytest.raises(ValueError):
        n.set_scale_state(bad)
    n.set_scale_state(state)
    np.testing.assert_array_equal(n.scale_state(), state)


@pytest.mark.parametrize("make,kind", [(_dqn, "mlp"), (_impala, "flat"), (_r2d2, "flat")])
def test_no_scale_state_without_planes(make, kind):
    n = make(kind)
    assert n.scale_state().size == 0
    n.set_scale_state(np.zeros(0, np.float32))
    assert n.scale_state().size == 0


def test_r2d2_num_steps_moves_adam_count():
    """acme_r2d2_set_num_steps also writes Adam's count (guard->applied)."""
    n = _r2d2("flat")
    assert n.guard_state()["applied"] == 0
    n.num_steps = 7
    assert n.num_steps == 7
    assert n.guard_state()["applied"] == 7
    torch.cuda.synchronize()
