"""MPO's Python layer without a GPU: the loss settings, the network descriptors and the
learner's argument checks (acme/agents/tf/mpo/learning.py:86-93,
acme/tf/networks/distributional.py:70-129)."""

import numpy as np
import pytest

from tests import mpo_oracle as O


def test_mpo_loss_defaults_are_the_reference_learners():
    """losses.MPO as MPOLearner builds it (learning.py:86-93) with losses.MPO's own defaults for
    the rest (mpo.py:60-62)."""
    from acme_amd.agents.mpo import MPOLoss
    loss = MPOLoss()
    assert (loss.epsilon, loss.epsilon_penalty, loss.epsilon_mean, loss.epsilon_stddev) == \
        (1e-1, 1e-3, 1e-3, 1e-6)
    assert (loss.init_log_temperature, loss.init_log_alpha_mean, loss.init_log_alpha_stddev) == \
        (1.0, 1.0, 10.0)
    assert loss.per_dim_constraining is True and loss.action_penalization is True
    cfg = O.MPOConfig()  # the oracle's defaults are the same settings
    for k in ("epsilon", "epsilon_penalty", "epsilon_mean", "epsilon_stddev",
              "init_log_temperature", "init_log_alpha_mean", "init_log_alpha_stddev",
              "per_dim_constraining", "action_penalization"):
        assert getattr(loss, k) == getattr(cfg, k), k


def test_network_descriptors_match_oracle():
    from acme_amd import specs
    from acme_amd.networks import LayerNormMLPCritic, make_mpo_networks
    cfg = O.MPOConfig()
    nets = make_mpo_networks(24, specs.BoundedArray((6,), np.float32, -1.0, 1.0))
    assert nets["policy"].tensor_shapes() == O.policy_tensor_shapes(cfg)
    assert nets["critic"].tensor_shapes() == O.critic_tensor_shapes(cfg)
    assert isinstance(nets["critic"], LayerNormMLPCritic)  # DDPG's, reused
    assert (nets["policy"].init_scale, nets["policy"].min_scale) == (0.3, 1e-6)
    assert nets["policy"].tensor_shapes()[-4:] == [
        ("policy/multivariate_normal_diag_head/linear/w", (256, 6)),
        ("policy/multivariate_normal_diag_head/linear/b", (6,)),
        ("policy/multivariate_normal_diag_head/linear_1/w", (256, 6)),
        ("policy/multivariate_normal_diag_head/linear_1/b", (6,))]


def test_gaussian_head_initialisation():
    """VarianceScaling(1e-4) (fan-in, truncated normal) head weights, zero biases; the initial
    stddev is init_scale + min_scale up to the effect of the tiny weights."""
    from acme_amd.networks import LayerNormMLPGaussianPolicy
    net = LayerNormMLPGaussianPolicy(24, 6, (256, 256, 256))
    init = net.init(0)
    assert [(k, v.shape) for k, v in init.items()] == net.tensor_shapes()
    head = "policy/multivariate_normal_diag_head"
    for layer in ("linear", "linear_1"):
        w = init[f"{head}/{layer}/w"]
        assert w.std() == pytest.approx(np.sqrt(1e-4 / 256), rel=0.1)  # 1536 draws
        assert np.abs(w).max() <= 2.0 * np.sqrt(1e-4 / 256) / 0.87962566103423978 * 1.0001
        assert not init[f"{head}/{layer}/b"].any()
    cfg = O.MPOConfig()
    o = np.random.default_rng(0).standard_normal((32, 24)).astype(np.float32)
    mean, stddev, _ = O.policy_forward(cfg, init, o, np.float64)
    # |h| <= 1 (elu of bounded inputs is not bounded by 1 above, but these are small), so the
    # scale layer's output is at most a few 1e-2: stddev moves by a few percent of 0.3.
    np.testing.assert_allclose(stddev, 0.3 + 1e-6, rtol=0.05)
    assert np.abs(mean).max() < 0.1
    other = LayerNormMLPGaussianPolicy(24, 6, (256, 256, 256), init_scale=0.7, min_scale=1e-3)
    c2 = O.MPOConfig(init_scale=0.7, min_scale=1e-3)
    _, s2, _ = O.policy_forward(c2, other.init(0), o, np.float64)
    np.testing.assert_allclose(s2, 0.7 + 1e-3, rtol=0.05)


def test_learner_rejects_non_identity_observation_network():
    from acme_amd import specs
    from acme_amd.agents.mpo import MPOLearner
    from acme_amd.networks import make_mpo_networks
    nets = make_mpo_networks(24, specs.BoundedArray((6,), np.float32, -1.0, 1.0))
    with pytest.raises(ValueError, match="identity observation networks"):
        MPOLearner(nets["policy"], nets["critic"], nets["policy"], nets["critic"], discount=0.99,
                   num_samples=20, target_policy_update_period=100,
                   target_critic_update_period=100, dataset=iter(()),
                   observation_network=lambda x: x * 2.0)


def test_package_exports():
    import acme_amd.agents.mpo as mpo
    from acme_amd import _lib, native
    from acme_amd.agents.mpo import agent, learning
    assert mpo.MPO is agent.MPO and mpo.MPOLearner is learning.MPOLearner
    assert mpo.MPOLoss is learning.MPOLoss
    assert issubclass(native.NativeMPO, native._NativeActorCritic)  # noqa: SLF001
    # The stats' order is the header's enum.
    assert _lib.MPO_STATS[0] == "dual_alpha_mean" and _lib.MPO_STATS[-1] == "pi_stddev_cond"
    assert len(_lib.MPO_STATS) == 13
    for name in ("create", "destroy", "flat_size", "policy_size", "dual_offset", "num_tensors",
                 "tensor_info", "bind", "init_duals", "step", "policy", "num_steps",
                 "set_num_steps", "debug_buffer"):
        assert hasattr(_lib.lib(), f"acme_mpo_{name}"), name
