"""DMPO's Python layer without a GPU: the network descriptors, the learner's argument checks and
the agent's gating numbers (acme/agents/tf/dmpo/learning.py:36-58, agent.py:47-69, 186-199)."""

import inspect

import numpy as np
import pytest

from tests import dmpo_oracle as O


def _spec():
    from acme_amd import specs
    return specs.BoundedArray((6,), np.float32, -1.0, 1.0)


def test_network_descriptors_match_oracle():
    from acme_amd.networks import (DistributionalCritic, LayerNormMLPGaussianPolicy,
                                   make_dmpo_networks)
    cfg = O.DMPOConfig()
    nets = make_dmpo_networks(24, _spec())
    assert isinstance(nets["policy"], LayerNormMLPGaussianPolicy)  # MPO's, reused
    assert isinstance(nets["critic"], DistributionalCritic)        # D4PG's, reused
    assert nets["policy"].tensor_shapes() == O.policy_tensor_shapes(cfg)
    assert nets["critic"].tensor_shapes() == O.critic_tensor_shapes(cfg)
    assert nets["policy"].tensor_shapes() + nets["critic"].tensor_shapes() + \
        O.dual_tensor_shapes(cfg) == O.dmpo_tensor_shapes(cfg)
    assert (nets["critic"].vmin, nets["critic"].vmax, nets["critic"].num_atoms) == (-150.0, 150.0, 51)
    np.testing.assert_array_equal(nets["critic"].values, O.support(cfg, np.float32))
    small = make_dmpo_networks(7, _spec(), (36, 100), (64, 44), vmin=-2.0, vmax=3.0, num_atoms=5,
                               init_scale=0.7, min_scale=1e-3)
    c2 = O.DMPOConfig(obs_dim=7, policy_sizes=(36, 100), critic_sizes=(64, 44), num_atoms=5,
                      vmin=-2.0, vmax=3.0)
    assert small["critic"].tensor_shapes() == O.critic_tensor_shapes(c2)
    assert small["policy"].tensor_shapes() == O.policy_tensor_shapes(c2)
    assert (small["policy"].init_scale, small["policy"].min_scale) == (0.7, 1e-3)


def _learner(cls, nets, **kw):
    args = dict(discount=0.99, num_samples=20, target_policy_update_period=100,
                target_critic_update_period=100, dataset=iter(()))
    args.update(kw)
    return cls(nets["policy"], nets["critic"], nets["policy"], nets["critic"], **args)


def test_learner_argument_checks():
    from acme_amd.agents.dmpo import DistributionalMPOLearner
    from acme_amd.agents.mpo import MPOLearner
    from acme_amd.networks import make_dmpo_networks, make_mpo_networks
    dnets, mnets = make_dmpo_networks(24, _spec()), make_mpo_networks(24, _spec())
    with pytest.raises(ValueError, match="DMPO learner supports identity observation networks"):
        _learner(DistributionalMPOLearner, dnets, observation_network=lambda x: x * 2.0)
    with pytest.raises(ValueError, match="policy_loss_module must be an acme_amd.agents.mpo.MPOLoss"):
        _learner(DistributionalMPOLearner, dnets, policy_loss_module=object())
    with pytest.raises(ValueError, match="DMPO learner takes a DistributionalCritic"):
        _learner(DistributionalMPOLearner, mnets)
    with pytest.raises(ValueError, match="MPO learner takes a LayerNormMLPCritic"):
        _learner(MPOLearner, dnets)


def test_learner_takes_the_references_arguments():
    """learning.py:36-58, in order, then this package's own (batch_size, seed, device)."""
    from acme_amd.agents.dmpo import DistributionalMPOLearner
    from acme_amd.agents.mpo import MPOLearner
    names = list(inspect.signature(DistributionalMPOLearner.__init__).parameters)[1:]
    assert names[:19] == [
        "policy_network", "critic_network", "target_policy_network", "target_critic_network",
        "discount", "num_samples", "target_policy_update_period", "target_critic_update_period",
        "dataset", "observation_network", "target_observation_network", "policy_loss_module",
        "policy_optimizer", "critic_optimizer", "dual_optimizer", "clipping", "counter", "logger",
        "checkpoint"]
    assert issubclass(DistributionalMPOLearner, MPOLearner)
    assert DistributionalMPOLearner.checkpoint_subdirectory == "dmpo_learner"
    assert MPOLearner.checkpoint_subdirectory == "mpo_learner"


def test_agent_defaults_and_gating_numbers():
    """agent.py:47-69: the defaults; :186-199: min_observations = max(batch_size,
    min_replay_size), observations_per_step = batch_size / samples_per_insert."""
    from acme_amd.agents import dmpo
    from acme_amd.agents.agent import Agent
    sig = inspect.signature(dmpo.DistributionalMPO.__init__).parameters
    want = dict(discount=0.99, batch_size=256, prefetch_size=4, target_policy_update_period=100,
                target_critic_update_period=100, min_replay_size=1000, max_replay_size=1000000,
                samples_per_insert=32.0, policy_loss_module=None, policy_optimizer=None,
                critic_optimizer=None, n_step=5, num_samples=20, clipping=True, logger=None,
                counter=None, checkpoint=True, replay_table_name="priority_table")
    for k, v in want.items():
        assert sig[k].default == v, k
    assert list(sig)[1:4] == ["environment_spec", "policy_network", "critic_network"]
    # The gating arithmetic at the defaults: wait for 1000 observations, then one learner step
    # every 8 observations.
    gate = Agent(actor=None, learner=None, min_observations=max(256, 1000),
                 observations_per_step=256 / 32.0)
    assert gate._countdown == -1000  # noqa: SLF001
    assert (gate._obs_per_update, gate._steps_per_update) == (8, 1)  # noqa: SLF001
    src = inspect.getsource(dmpo.DistributionalMPO.__init__)
    assert "min_observations=max(batch_size, min_replay_size)" in src
    assert "observations_per_step=float(batch_size) / samples_per_insert" in src


def test_package_exports():
    import acme_amd.agents.dmpo as dmpo
    from acme_amd import _lib, native
    from acme_amd.agents.dmpo import agent, learning
    assert dmpo.DistributionalMPO is agent.DistributionalMPO
    assert dmpo.DistributionalMPOLearner is learning.DistributionalMPOLearner
    assert issubclass(native.NativeDMPO, native.NativeMPO)
    assert native.NativeDMPO._prefix == "acme_dmpo"  # noqa: SLF001
    for name in ("create", "destroy", "flat_size", "policy_size", "dual_offset", "num_tensors",
                 "tensor_info", "bind", "init_duals", "step", "policy", "num_steps",
                 "set_num_steps", "debug_buffer"):
        assert hasattr(_lib.lib(), f"acme_dmpo_{name}"), name
        assert f"acme_dmpo_{name}" in _lib.EXPORTED_SYMBOLS
    # acme_dmpo_config = { acme_mpo_config mpo; int32 num_atoms; float vmin, vmax; }
    import ctypes
    assert _lib.DMPOConfig.mpo.offset == 0
    assert _lib.DMPOConfig.num_atoms.offset == ctypes.sizeof(_lib.MPOConfig)
    cfg = _lib.DMPOConfig()
    cfg.num_samples, cfg.num_atoms = 20, 51  # the MPO fields are reachable directly
    assert cfg.mpo.num_samples == 20


def test_create_rejects_bad_supports_without_a_gpu():
    """Argument validation happens before anything touches the device."""
    import ctypes
    from acme_amd import _lib
    L = _lib.lib()

    def create(**kw):
        cfg = _lib.DMPOConfig()
        cfg.obs_dim, cfg.act_dim, cfg.max_batch = 7, 3, 8
        cfg.num_policy_layers = cfg.num_critic_layers = 1
        cfg.policy_sizes[0] = cfg.critic_sizes[0] = 16
        cfg.num_samples = 4
        cfg.target_policy_update_period = cfg.target_critic_update_period = 1
        cfg.epsilon = cfg.epsilon_mean = cfg.epsilon_stddev = cfg.epsilon_penalty = 0.1
        cfg.init_scale = 0.3
        cfg.num_atoms, cfg.vmin, cfg.vmax = 5, -2.0, 3.0
        for k, v in kw.items():
            setattr(cfg, k, v)
        h = ctypes.c_void_p()
        rc = L.acme_dmpo_create(ctypes.byref(cfg), ctypes.byref(h))
        return rc, L.acme_last_error().decode()

    for kw, msg in ((dict(num_atoms=1), "num_atoms"), (dict(num_atoms=65), "num_atoms"),
                    (dict(vmax=-2.0), "vmax must exceed vmin"), (dict(vmax=-3.0), "vmax"),
                    (dict(num_samples=65), "num_samples"),
                    (dict(max_batch=_lib.MPO_MAX_ROWS // 4 + 1), "max_batch \\* num_samples")):
        rc, err = create(**kw)
        assert rc == _lib.ACME_ERR_INVALID, kw
        assert msg.replace("\\", "") in err, (kw, err)
