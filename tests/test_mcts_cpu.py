"""The MCTS agent's Python layer and acme_az_create's refusals without a GPU: the exports
against the header, the constructors' argument checks, the Catch board and the actor on a
host-side evaluation."""

import ctypes
import os
import re

import numpy as np
import pytest

from acme_amd import specs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("create", "destroy", "flat_size", "num_tensors", "tensor_info", "bind", "step",
           "evaluate", "num_steps", "set_num_steps", "debug_buffer")


def test_exports_match_the_header():
    from acme_amd import _lib, native
    text = open(os.path.join(ROOT, "include", "acme_hip.h")).read()
    protos = re.findall(r"^(int|int32_t|int64_t) (acme_az_\w+)\(([^;]*)\);", text, re.M)
    assert {n for _, n, _ in protos} == {f"acme_az_{e}" for e in EXPORTS}
    res = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    L = _lib.lib()
    for ret, name, args in protos:
        assert name in _lib.EXPORTED_SYMBOLS
        fn = getattr(L, name)
        assert fn.restype is res[ret], name
        assert len(fn.argtypes) == len(args.split(",")), (name, args)
    for struct, cls in (("acme_az_config", _lib.AZConfig), ("acme_az_batch", _lib.AZBatch),
                        ("acme_az_outputs", _lib.AZOutputs)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S)
        fields = []
        for decl in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";"):
            decl = decl.strip()
            if decl:
                names = decl.rsplit(None, 1)[1] if "," not in decl else decl.split(None, 1)[1]
                fields += [re.sub(r"\[.*\]", "", f).strip(" *") for f in names.split(",")]
        assert fields == [f[0] for f in cls._fields_], struct  # noqa: SLF001
    for macro, value in (("ACME_AZ_MAX_WIDTH", _lib.AZ_MAX_WIDTH),
                         ("ACME_AZ_MAX_ACTIONS", _lib.AZ_MAX_ACTIONS),
                         ("ACME_AZ_MAX_ROWS", _lib.AZ_MAX_ROWS),
                         ("ACME_AZ_FUSED_MAX_ROWS", _lib.AZ_FUSED_MAX_ROWS),
                         ("ACME_AZ_FUSED_MAX_WIDTH", _lib.AZ_FUSED_MAX_WIDTH)):
        assert int(re.search(r"#define %s (\d+)" % macro, text).group(1)) == value
    assert native.NativeAZ._prefix == "acme_az"  # noqa: SLF001
    assert issubclass(native.NativeAZ, native._NativeLearner)  # noqa: SLF001
    assert native.NativeAZ._has_target is False  # noqa: SLF001


def test_create_rejects_bad_configurations_without_a_gpu():
    """Argument validation happens before anything touches the device; the message names the
    field."""
    from acme_amd import _lib
    L = _lib.lib()

    def create(**kw):
        cfg = _lib.AZConfig()
        cfg.obs_dim, cfg.num_actions, cfg.max_batch, cfg.max_eval_rows = 10, 5, 8, 1
        cfg.num_hidden = 2
        cfg.hidden[0] = cfg.hidden[1] = 50
        cfg.discount, cfg.learning_rate = 1.0, 1e-3
        cfg.adam_beta1, cfg.adam_beta2, cfg.adam_epsilon = 0.9, 0.999, 1e-8
        hidden = kw.pop("hidden", None)
        for k, v in kw.items():
            setattr(cfg, k, v)
        if hidden is not None:
            cfg.hidden[hidden[0]] = hidden[1]
        h = ctypes.c_void_p()
        rc = L.acme_az_create(ctypes.byref(cfg), ctypes.byref(h))
        return rc, L.acme_last_error().decode()

    W, A, R = _lib.AZ_MAX_WIDTH, _lib.AZ_MAX_ACTIONS, _lib.AZ_MAX_ROWS
    for kw, msg in ((dict(num_hidden=0), "num_hidden"),
                    (dict(num_hidden=_lib.MAX_MLP_LAYERS + 1), "num_hidden"),
                    (dict(obs_dim=0), "obs_dim"), (dict(obs_dim=W + 1), "obs_dim"),
                    (dict(hidden=(0, 0)), "hidden[0]"), (dict(hidden=(1, W + 1)), "hidden[1]"),
                    (dict(num_actions=0), "num_actions"), (dict(num_actions=A + 1), "num_actions"),
                    (dict(max_batch=0), "max_batch"), (dict(max_batch=R + 1), "max_batch"),
                    (dict(max_eval_rows=0), "max_eval_rows"),
                    (dict(max_eval_rows=R + 1), "max_eval_rows"),
                    (dict(activate_final=2), "activate_final"),
                    (dict(adam_epsilon=0.0), "adam_epsilon"),
                    (dict(learning_rate=-1.0), "learning_rate")):
        rc, err = create(**kw)
        assert rc == _lib.ACME_ERR_INVALID, kw
        assert msg in err, (kw, err)
    with pytest.raises(ValueError, match="num_actions"):
        _lib.check(create(num_actions=0)[0])


def _spec(num_actions=3, obs_shape=(2, 3)):
    return specs.EnvironmentSpec(
        observations=specs.Array(obs_shape, np.float32), actions=specs.DiscreteArray(num_actions),
        rewards=specs.Array((), np.float32), discounts=specs.BoundedArray((), np.float32, 0., 1.))


def test_constructors_refuse_what_is_out_of_scope():
    from acme_amd.agents.mcts import MCTS, AZLearner, MCTSActor
    from acme_amd.agents.mcts.models import Simulator
    from acme_amd.environments.catch import Catch
    from acme_amd.networks import MLP, PolicyValueMLP
    from acme_amd.optimizers import Adam, optix
    env = Catch(rows=2, columns=3)
    spec = specs.make_environment_spec(env)
    model = Simulator(env)
    common = dict(model=model, optimizer=Adam(1e-3), n_step=1, discount=1.0, replay_capacity=100,
                  num_simulations=10, environment_spec=spec, batch_size=10)
    with pytest.raises(ValueError, match="takes a networks.PolicyValueMLP, not a MLP"):
        MCTS(network=MLP(6, (50,), 3), **common)
    with pytest.raises(ValueError, match="num_actions = 5, the environment spec 3"):
        MCTS(network=PolicyValueMLP(6, (50,), 5), **common)
    with pytest.raises(ValueError, match="obs_dim = 7"):
        MCTS(network=PolicyValueMLP(7, (50,), 3), **common)
    with pytest.raises(ValueError, match="takes a networks.PolicyValueMLP, not a MLP"):
        AZLearner(MLP(6, (50,), 3), Adam(1e-3), iter(()), discount=1.0)
    with pytest.raises(ValueError, match="does not clip gradients"):
        AZLearner(PolicyValueMLP(6, (50,), 3),
                  optix.chain(optix.clip_by_global_norm(1.0), optix.adam(1e-3)), iter(()), 1.0)
    with pytest.raises(ValueError, match="variable_client: it must be None"):
        MCTSActor(spec, model, lambda o: (np.ones(3) / 3, 0.0), 1.0, 10, variable_client=object())
    with pytest.raises(ValueError, match="evaluate"):
        MCTSActor(spec, model, object(), 1.0, 10)


def test_catch_board():
    import copy
    from acme_amd.environments.catch import Catch
    env = Catch(rows=4, columns=5, seed=1)
    ts = env.reset()
    assert ts.first() and ts.observation.shape == (4, 5) and ts.observation.dtype == np.float32
    assert ts.observation.sum() == 2.0 and ts.observation[3, 2] == 1.0
    assert ts.observation[0, env._ball_x] == 1.0 and env._paddle_x == 2  # noqa: SLF001
    twin = copy.deepcopy(env)
    target = env._ball_x  # noqa: SLF001
    total = 0.0
    for t in range(3):
        dx = int(np.sign(target - env._paddle_x))  # noqa: SLF001
        ts = env.step(1 + dx)
        total += ts.reward
        assert ts.last() == (t == 2) and ts.reward.dtype == np.float32
    assert total == 1.0 and ts.discount == 0.0
    for a in (0, 0, 0):  # the copy plays its own game: hard left from the middle
        ts2 = twin.step(a)
    assert twin._paddle_x == 0 and ts2.reward == (1.0 if target == 0 else -1.0)  # noqa: SLF001
    assert env.step(1).first()  # a step after the end starts the next episode
    # The same seed gives the same sequence of balls.
    a, b = Catch(seed=7), Catch(seed=7)
    assert [a.reset().observation.argmax() for _ in range(5)] == \
           [b.reset().observation.argmax() for _ in range(5)]
    assert env.action_spec().num_values == 3
    with pytest.raises(ValueError):
        Catch(rows=1)


class _Adder:
    def __init__(self):
        self.first, self.steps = None, []

    def add_first(self, timestep):
        self.first = timestep

    def add(self, action, next_timestep, extras=()):
        self.steps.append((action, next_timestep, extras))


def test_actor_plans_and_stores_the_search_policy():
    """MCTSActor on a host-side evaluation: legal actions, the visit distribution stored with
    the transition, the model kept in step with the environment."""
    from acme_amd.agents.mcts import MCTSActor
    from acme_amd.agents.mcts.models import Simulator
    from acme_amd.environments.catch import Catch
    env = Catch(rows=3, columns=3, seed=2)
    spec = specs.make_environment_spec(env)
    model, adder = Simulator(env), _Adder()
    np.random.seed(0)
    actor = MCTSActor(spec, model, lambda o: (np.ones(3) / 3, 0.0), discount=1.0,
                      num_simulations=60, adder=adder)
    ts = env.reset()
    actor.observe_first(ts)
    ret = 0.0
    while not ts.last():
        action = actor.select_action(ts.observation)
        assert action.dtype == np.int32 and 0 <= action < 3
        ts = env.step(action)
        actor.observe(action, ts)
        actor.update()
        ret += ts.reward
    assert adder.first.first() and len(adder.steps) == 2
    for _, _, extras in adder.steps:
        pi = extras["pi"]
        assert pi.dtype == np.float32 and pi.shape == (3,) and (pi >= 0).all()
        assert abs(pi.sum() - 1.0) < 1e-6
    assert model.needs_reset  # it followed the real episode to its end
    # Every stored policy is a visit distribution over 60 simulations.
    for _, _, extras in adder.steps:
        np.testing.assert_allclose(extras["pi"] * 60, np.round(extras["pi"] * 60), atol=1e-4)
