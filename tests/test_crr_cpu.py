"""CRR's native exports and Python layer without a GPU: the acme_crr_* symbols against the
header's prototypes, the learner's argument checks (acme/agents/tf/crr/recurrent_learning.py:
43-65), acme_crr_create's refusals and the flattening of [B, T] sequences into transitions."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import crr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("create", "destroy", "flat_size", "policy_size", "num_tensors", "tensor_info", "bind",
           "step", "policy", "num_steps", "set_num_steps", "debug_buffer")


def _spec():
    from acme_amd import specs
    return specs.BoundedArray((6,), np.float32, -1.0, 1.0)


def test_exports_match_the_header():
    from acme_amd import _lib
    text = open(os.path.join(ROOT, "include", "acme_hip.h")).read()
    protos = re.findall(r"^(int|int32_t|int64_t) (acme_crr_\w+)\(([^;]*)\);", text, re.M)
    assert {n for _, n, _ in protos} == {f"acme_crr_{e}" for e in EXPORTS}
    res = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    L = _lib.lib()
    for ret, name, args in protos:
        assert hasattr(L, name), f"{name} declared in include/acme_hip.h but not exported"
        assert name in _lib.EXPORTED_SYMBOLS
        fn = getattr(L, name)
        assert fn.restype is res[ret], name
        assert len(fn.argtypes) == len(args.split(",")), (name, args)
    # acme_crr_config, field by field in the header's order.
    body = re.search(r"typedef struct acme_crr_config \{(.*?)\} acme_crr_config;", text, re.S)
    fields = []
    for decl in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"\[.*\]", "", f).strip() for f in decl.split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in _lib.CRRConfig._fields_]  # noqa: SLF001
    assert _lib.CRRConfig.seed.offset % 8 == 0 and ctypes.sizeof(_lib.CRRConfig) % 8 == 0
    assert [f[0] for f in _lib.CRROutputs._fields_] == [  # noqa: SLF001
        "critic_loss", "policy_loss", "policy_loss_coef"]
    from acme_amd import native
    assert native.NativeCRR._prefix == "acme_crr"  # noqa: SLF001
    assert issubclass(native.NativeCRR, native._NativeActorCritic)  # noqa: SLF001


def test_package_exports():
    import acme_amd.agents.crr as crr
    from acme_amd.agents.crr import learning
    assert crr.CRRLearner is learning.CRRLearner
    assert crr.RCRRLearner is crr.CRRLearner
    assert not hasattr(crr, "agent")  # the reference's crr/__init__.py exports the learner only


def test_learner_takes_the_references_arguments():
    """recurrent_learning.py:43-65, in order, then this package's own."""
    from acme_amd.agents.crr import CRRLearner
    sig = inspect.signature(CRRLearner.__init__).parameters
    names = list(sig)[1:]
    assert names[:22] == [
        "policy_network", "critic_network", "target_policy_network", "target_critic_network",
        "dataset", "accelerator_strategy", "behavior_network", "cwp_network", "policy_optimizer",
        "critic_optimizer", "discount", "target_update_period", "num_action_samples_td_learning",
        "num_action_samples_policy_weight", "baseline_reduce_function", "clipping",
        "policy_improvement_modes", "ratio_upper_bound", "beta", "counter", "logger", "checkpoint"]
    assert names[22:] == ["batch_size", "seed", "device"]
    want = dict(discount=0.99, target_update_period=100, num_action_samples_td_learning=1,
                num_action_samples_policy_weight=4, baseline_reduce_function="mean", clipping=True,
                policy_improvement_modes="exp", ratio_upper_bound=20.0, beta=1.0,
                checkpoint=False)
    for k, v in want.items():
        assert sig[k].default == v, k


def _learner(nets, **kw):
    from acme_amd.agents.crr import CRRLearner
    args = dict(dataset=iter(()))
    args.update(kw)
    return CRRLearner(nets["policy"], nets["critic"], nets["policy"], nets["critic"], **args)


def test_learner_argument_checks():
    """Every refusal comes before the dataset is read or the device touched."""
    from acme_amd.networks import make_d4pg_networks, make_dmpo_networks, make_mpo_networks
    nets = make_dmpo_networks(24, _spec())
    types = "LayerNormMLPGaussianPolicy policy and a DistributionalCritic critic"
    with pytest.raises(ValueError, match=types + ", not a LayerNormMLPCritic"):
        _learner(make_mpo_networks(24, _spec()))
    with pytest.raises(ValueError, match=types + ", not a LayerNormMLPPolicy"):
        _learner(make_d4pg_networks(24, _spec()))
    for name in ("accelerator_strategy", "behavior_network", "cwp_network"):
        with pytest.raises(ValueError, match=f"does not support {name}: it must be None"):
            _learner(nets, **{name: object()})
    for name in ("num_action_samples_td_learning", "num_action_samples_policy_weight"):
        for n in (0, 65):
            with pytest.raises(ValueError, match=name + r" must be in \[1, 64\]"):
                _learner(nets, **{name: n})
    # With valid arguments the next thing it does is read the dataset's first sample.
    with pytest.raises(StopIteration):
        _learner(nets)


def test_flattening_order():
    """NativeCRR.flatten_sequences: row b (T - 1) + (t - 1) = (o[b, t-1], a[b, t-1], r[b, t-1],
    d[b, t-1], o[b, t]), the oracle's flatten_sequences."""
    from acme_amd.native import NativeCRR
    B, T, od, A = 3, 4, 5, 2
    rng = np.random.default_rng(0)
    seq = dict(observation=rng.standard_normal((B, T, od)).astype(np.float32),
               action=rng.standard_normal((B, T, A)).astype(np.float32),
               reward=rng.standard_normal((B, T)).astype(np.float32),
               discount=rng.random((B, T)).astype(np.float32))
    got = NativeCRR.flatten_sequences(*[torch.as_tensor(seq[k]) for k in (
        "observation", "action", "reward", "discount")])
    want = O.flatten_sequences(seq)
    for g, k in zip(got, ("o_tm1", "a_tm1", "r_t", "d_t", "o_t")):
        assert g.is_contiguous() and g.dtype == torch.float32
        np.testing.assert_array_equal(g.numpy(), want[k], err_msg=k)
    assert got[0].shape == (B * (T - 1), od) and got[2].shape == (B * (T - 1),)
    i = 1 * (T - 1) + (3 - 1)
    np.testing.assert_array_equal(got[4][i].numpy(), seq["observation"][1, 3])
    np.testing.assert_array_equal(got[1][i].numpy(), seq["action"][1, 2])


def test_create_rejects_bad_configurations_without_a_gpu():
    """Argument validation happens before anything touches the device."""
    from acme_amd import _lib
    L = _lib.lib()

    def create(**kw):
        cfg = _lib.CRRConfig()
        cfg.obs_dim, cfg.act_dim, cfg.max_batch = 7, 3, 8
        cfg.num_policy_layers = cfg.num_critic_layers = 1
        cfg.policy_sizes[0] = cfg.critic_sizes[0] = 16
        cfg.num_atoms, cfg.vmin, cfg.vmax = 5, -2.0, 3.0
        cfg.num_action_samples_td_learning, cfg.num_action_samples_policy_weight = 1, 4
        cfg.ratio_upper_bound, cfg.beta, cfg.init_scale = 20.0, 1.0, 0.3
        cfg.target_update_period, cfg.sequence_length = 1, 2
        for k, v in kw.items():
            setattr(cfg, k, v)
        h = ctypes.c_void_p()
        rc = L.acme_crr_create(ctypes.byref(cfg), ctypes.byref(h))
        return rc, L.acme_last_error().decode()

    rows = _lib.MPO_MAX_ROWS
    for kw, msg in ((dict(num_action_samples_td_learning=0), "num_action_samples_td_learning"),
                    (dict(num_action_samples_td_learning=65), "num_action_samples_td_learning"),
                    (dict(num_action_samples_policy_weight=0), "num_action_samples_policy_weight"),
                    (dict(num_action_samples_policy_weight=65), "num_action_samples_policy_weight"),
                    (dict(max_batch=rows // 5 + 1), "max_batch * (1 + max("),
                    (dict(max_batch=rows // 9 + 1, num_action_samples_td_learning=8),
                     "max_batch * (1 + max("),
                    (dict(baseline_reduce_function=3), "baseline_reduce_function"),
                    (dict(policy_improvement_modes=-1), "policy_improvement_modes"),
                    (dict(beta=0.0), "beta"), (dict(sequence_length=1), "sequence_length"),
                    (dict(num_atoms=1), "num_atoms"), (dict(vmax=-2.0), "vmax must exceed vmin"),
                    (dict(target_update_period=0), "target_update_period")):
        rc, err = create(**kw)
        assert rc == _lib.ACME_ERR_INVALID, kw
        assert msg in err, (kw, err)
