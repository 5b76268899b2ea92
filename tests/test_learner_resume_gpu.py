"""The learners' save / restore at the learner level, where no other test resumes them:
IMPALALearner (flat and Atari torso) and D4PGLearner restored into a learner built from
another seed continue bit for bit; R2D2Learner reads the round-4 optimizer form; and every
learner's checkpoint has exactly its documented keys.  The learners take their batches from
a list (they accept any iterable), so both sides of a comparison see the same device tensors.
"""

import numpy as np
import pytest
import torch

from oracle import impala_oracle as IO
from tests import test_d4pg_gpu as TD
from tests import test_impala_gpu as TI
from tests import test_r2d2_learner_gpu as TR

pytestmark = pytest.mark.gpu


def _sequence_sample(b, with_logits):
    """A [B, T] sequence batch of the tests' numpy form as the ReplaySample a sequence dataset
    yields: Step(OAR, action, reward, discount, start, extras) of device tensors."""
    from acme_amd.adders.reverb import Step
    from acme_amd.networks import LSTMState
    from acme_amd.replay import ReplaySample, SampleInfo
    from acme_amd.wrappers import OAR
    d = lambda x: torch.as_tensor(x).cuda()  # noqa: E731
    state = d(b["state"])  # [B, T, 2, H]
    extras = {"core_state": LSTMState(state[:, :, 0], state[:, :, 1])}
    if with_logits:
        extras["logits"] = d(b["behaviour_logits"])
    B, T = b["action"].shape
    data = Step(observation=OAR(d(b["obs"]), d(b["prev_action"]), d(b["prev_reward"])),
                action=d(b["action"]), reward=d(b["reward"]), discount=d(b["discount"]),
                start_of_episode=torch.zeros(B, T, dtype=torch.bool, device="cuda"),
                extras=extras)
    info = None
    if "probabilities" in b:
        info = SampleInfo(key=torch.arange(B, dtype=torch.int64, device="cuda"),
                          probability=d(np.asarray(b["probabilities"], np.float64)),
                          table_size=None, priority=None)
    return ReplaySample(info=info, data=data)


def _same_buffers(a, b, names, what):
    for name in names:
        np.testing.assert_array_equal(getattr(a, name).cpu().numpy(),
                                      getattr(b, name).cpu().numpy(), err_msg=f"{what}: {name}")


@pytest.mark.parametrize("torso", ["flat", "atari"])
def test_impala_learner_resume(torso):
    """Learner A: two steps, save(), two more.  Learner B (another seed) restored from that
    state runs the same last two batches: after each, parameters, Adam moments, metrics and
    both step counts are A's bit for bit.  On the Atari torso (64 frames, the plane path)
    B's scale state is A's right after the restore and neither learner skips a step."""
    from acme_amd.agents.impala import IMPALALearner
    from acme_amd.networks import IMPALAAtariNetwork
    from acme_amd.utils import loggers
    if torso == "atari":  # B * T = 64 frames: the fewest that take the plane path
        B, T = 4, 16
        cfg = IO.IMPALAConfig(num_actions=18, torso="atari", lstm_size=256, head_size=64,
                              entropy_cost=0.01, baseline_cost=0.5)
    else:
        B, T = 2, 4
        cfg = IO.IMPALAConfig(num_actions=5, torso="flat", obs_dim=12, lstm_size=8, head_size=4,
                              entropy_cost=0.01, baseline_cost=0.5)
    net = IMPALAAtariNetwork(cfg.num_actions, lstm_size=cfg.lstm_size, head_size=cfg.head_size,
                             torso=cfg.torso, obs_dim=cfg.obs_dim)
    samples = [_sequence_sample(TI._batch(cfg, B, T, 30 + k), True) for k in range(4)]

    def make(seed, batches):
        return IMPALALearner(None, net, batches, learning_rate=cfg.learning_rate,
                             entropy_cost=0.01, baseline_cost=0.5, batch_size=B,
                             sequence_length=T, seed=seed, logger=loggers.NoOpLogger())

    a, b = make(1, samples), make(2, samples[2:])
    for _ in range(2):
        a.step()
    state = a.save()
    assert state["num_steps"] == 2 and state["optimizer"]["step"] == 2
    b.restore(state)
    if torso == "atari":
        assert state["plane_scales"].size > 0
        np.testing.assert_array_equal(b.native.scale_state(), a.native.scale_state())
    for k in (2, 3):
        a.step()
        b.step()
        torch.cuda.synchronize()
        _same_buffers(a.native, b.native, ("params", "m", "v", "metrics"), f"step {k}")
        assert a.num_steps == b.num_steps == k + 1
        assert a.native.applied_steps == b.native.applied_steps == k + 1
    if torso == "atari":
        assert a.native.skipped_steps == 0 and b.native.skipped_steps == 0


def _actor_critic_networks(kind):
    """Each actor-critic learner's networks at the golden D4PG step's sizes."""
    from acme_amd import networks as N
    policy_cls = N.LayerNormMLPPolicy if kind in ("d4pg", "ddpg") else N.LayerNormMLPGaussianPolicy
    policy = policy_cls(24, 6, (32, 32, 32))
    if kind in ("d4pg", "dmpo"):
        critic = N.DistributionalCritic(24, 6, (64, 64, 32))
    else:
        critic = N.LayerNormMLPCritic(24, 6, (64, 64, 32))
    return policy, critic


def _transition_sample(cfg, B, seed):
    from acme_amd.replay import ReplaySample
    return ReplaySample(info=None, data=tuple(TD._dev(TD._batch(cfg, B, seed))))


def test_d4pg_learner_resume():
    """As the IMPALA test, at the golden step's shape (B = 8), with a target period of 3 so
    that the target copy at the start of the fourth step falls after the restore: it happens
    only if the restored step count is right."""
    from acme_amd.agents.d4pg import D4PGLearner
    from acme_amd.utils import loggers
    from tests.golden.make_d4pg_golden import golden_cfg
    cfg, B = golden_cfg(), 8
    policy, critic = _actor_critic_networks("d4pg")
    samples = [_transition_sample(cfg, B, 40 + k) for k in range(4)]

    def make(seed, batches):
        return D4PGLearner(policy, critic, policy, critic, discount=0.99,
                           target_update_period=3, dataset=batches, batch_size=B, seed=seed,
                           logger=loggers.NoOpLogger())

    a, b = make(0, samples), make(7, samples[2:])
    for _ in range(2):
        a.step()
    b.restore(a.save())
    assert b.num_steps == 2
    for k in (2, 3):
        before = a.native.target.clone()
        a.step()
        b.step()
        torch.cuda.synchronize()
        _same_buffers(a.native, b.native, ("params", "target", "m", "v", "critic_loss",
                                           "policy_loss"), f"step {k}")
        assert a.num_steps == b.num_steps == k + 1
        assert bool((a.native.target != before).any()) == (k == 3)  # the copy, in both


def _r2d2_flat_learner(seed, batches=()):
    from acme_amd.agents.r2d2 import R2D2Learner
    from acme_amd.networks import R2D2AtariNetwork
    from acme_amd.utils import loggers
    net = R2D2AtariNetwork(5, lstm_size=8, head_size=8, torso="flat", obs_dim=12)
    return R2D2Learner(None, net, net, burn_in_length=1, sequence_length=4, dataset=batches,
                       n_step=3, max_replay_size=1000, target_update_period=2, batch_size=2,
                       seed=seed, logger=loggers.NoOpLogger())


def test_r2d2_restores_round4_optimizer_form():
    """A checkpoint whose optimizer is in the round-4 form ("step" = num_steps, the applied
    count under "applied_steps") restores to the same counts as the current form ("step" =
    the applied count).  The two counts differ here, as after a skipped step."""
    cfg = TR._cfg(lstm_size=8, burn_in_length=1)
    samples = [_sequence_sample(TR._batch(cfg, 2, 4, 50 + k), False) for k in range(2)]
    a = _r2d2_flat_learner(3, samples)
    for _ in range(2):
        a.step()
    state = a.save()
    assert state["num_steps"] == 2 and state["optimizer"]["step"] == 2
    current = dict(state, optimizer=dict(state["optimizer"], step=1))
    legacy = dict(state, optimizer=dict(state["optimizer"], step=2, applied_steps=1))
    counts = []
    for ckpt in (current, legacy):
        b = _r2d2_flat_learner(4)
        b.restore(ckpt)
        counts.append((b.num_steps, b.native.guard_state()["applied"]))
        _same_buffers(a.native, b.native, ("params", "target", "m", "v"), "restored")
    assert counts == [(2, 1), (2, 1)]


_PLANE_KEYS = {"network", "optimizer", "num_steps", "plane_scales"}
_ACTOR_CRITIC_KEYS = {"params", "target", "optimizer", "num_steps"}


def _make_learner(kind):
    from acme_amd.utils import loggers
    log = loggers.NoOpLogger()
    if kind == "dqn":
        from acme_amd.agents.dqn import DQNLearner
        from acme_amd.networks import MLP
        net = MLP(6, (8,), 3)
        return DQNLearner(net, net, discount=0.99, importance_sampling_exponent=0.2,
                          learning_rate=1e-3, target_update_period=2, dataset=(), batch_size=4,
                          logger=log)
    if kind == "impala":
        from acme_amd.agents.impala import IMPALALearner
        from acme_amd.networks import IMPALAAtariNetwork
        net = IMPALAAtariNetwork(5, lstm_size=8, head_size=4, torso="flat", obs_dim=12)
        return IMPALALearner(None, net, (), learning_rate=1e-3, batch_size=2, sequence_length=4,
                             logger=log)
    if kind == "r2d2":
        return _r2d2_flat_learner(0)
    policy, critic = _actor_critic_networks(kind)
    common = dict(discount=0.99, dataset=(), batch_size=8, logger=log)
    if kind in ("d4pg", "ddpg"):
        from acme_amd.agents.d4pg import D4PGLearner
        from acme_amd.agents.ddpg import DDPGLearner
        cls = D4PGLearner if kind == "d4pg" else DDPGLearner
        return cls(policy, critic, policy, critic, target_update_period=3, **common)
    from acme_amd.agents.dmpo import DistributionalMPOLearner
    from acme_amd.agents.mpo import MPOLearner
    cls = MPOLearner if kind == "mpo" else DistributionalMPOLearner
    return cls(policy, critic, policy, critic, num_samples=4, target_policy_update_period=3,
               target_critic_update_period=3, **common)


@pytest.mark.parametrize("kind,keys,opt_keys", [
    ("dqn", _PLANE_KEYS | {"target_network"}, {"m", "v", "step"}),
    ("impala", _PLANE_KEYS, {"m", "v", "step"}),
    ("r2d2", _PLANE_KEYS | {"target_network"}, {"m", "v", "step"}),
    ("d4pg", _ACTOR_CRITIC_KEYS, {"m", "v"}),
    ("ddpg", _ACTOR_CRITIC_KEYS, {"m", "v"}),
    ("mpo", _ACTOR_CRITIC_KEYS, {"m", "v"}),
    ("dmpo", _ACTOR_CRITIC_KEYS, {"m", "v"}),
])
def test_checkpoint_dict_shape(kind, keys, opt_keys):
    """The exact key set of save() and of its optimizer, and the value types: parameter and
    moment dicts of float32 arrays over the learner's tensor names, int counts, a float32
    array of plane scales.  `state` is the same checkpoint."""
    learner = _make_learner(kind)
    state = learner.save()
    assert set(state) == keys and set(state["optimizer"]) == opt_keys
    assert set(learner.state) == keys
    names = {name for name, _, _ in learner.native.tensors}
    tensors = [state[k] for k in keys - {"optimizer", "num_steps", "plane_scales"}]
    for d in tensors + [state["optimizer"]["m"], state["optimizer"]["v"]]:
        assert set(d) == names
        assert all(isinstance(v, np.ndarray) and v.dtype == np.float32 for v in d.values())
    assert type(state["num_steps"]) is int and state["num_steps"] == 0
    if "step" in opt_keys:
        assert type(state["optimizer"]["step"]) is int
        scales = state["plane_scales"]
        assert isinstance(scales, np.ndarray) and scales.dtype == np.float32
