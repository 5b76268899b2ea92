"""Demonstration sequences mixed into sequence batches on the GPU (acme_seq_demo_mix,
csrc/demos.hip; acme_amd/datasets/demonstrations.py; acme_amd/agents/r2d3) against the
numpy oracle tests/r2d3_oracle.py, bit for bit.

  * test_mixed_sequences_equal_oracle: is_demo, the info fields, every data field (the copied
    leaves, start_of_episode, the zeroed extras) and the untouched replay rows (those of a
    twin table drawn without the mix), over tests/r2d3_cases.py: steps of 3 bytes (the byte
    path), 12 (4-byte), 16 and 28,224 bytes (16-byte; rows of several chunks), plain and
    OAR-nested observations, T = 2, 5, 9, B = 1, 5, 33, one episode of one step, periods 1, 4
    and beyond every length, ratios 0, 0.25, 0.5 and 1.  tests/test_r2d3_cpu.py asserts on the
    oracle that these cases hold padded and unpadded windows, windows at and after an
    episode's start, and both kinds of row.
  * test_prefetch_depth_does_not_change_the_batches: prefetch 0 and 3, with host inserts.
  * test_sentinel_key_through_update_priorities: a mixed batch's keys through
    client.update_priorities; the tree equals, bit for bit, a twin's that received the replay
    rows' updates only.
  * test_teacher_forced_step: R2D2Learner.step() (store_lstm_state=False) on mixed batches
    against oracle/r2d2_oracle.loss_and_grads at test_r2d2_agent_gpu's shapes and tolerances.
  * test_agent_runs: the reference's r2d3/agent_test.py.
"""

import numpy as np
import pytest
import torch

from acme_amd import replay, specs
from acme_amd.adders import reverb as adders
from acme_amd.datasets import (SequenceDemonstrationStore, make_reverb_dataset,
                               mix_sequence_demonstrations)
from acme_amd.networks import LSTMState
from acme_amd.utils import tree
from acme_amd.wrappers import OAR
from tests import r2d3_oracle as O
from tests.r2d3_cases import CASES, DRAWS, MIX_SEED, OBS, case_id

pytestmark = pytest.mark.gpu

H = 4
NAME = adders.DEFAULT_PRIORITY_TABLE


def _signature(nb, oar):
    shape, dtype = OBS[nb]
    action, reward = specs.Array((), np.int32, "action"), specs.Array((), np.float32, "reward")
    obs = specs.Array(shape, dtype, "observation")
    spec = specs.EnvironmentSpec(OAR(obs, action, reward) if oar else obs, action, reward,
                                 specs.Array((), np.float32, "discount"))
    extras = {"core_state": LSTMState(specs.Array((H,), np.float32),
                                      specs.Array((H,), np.float32))}
    return adders.SequenceAdder.signature(spec, extras)


def _obs(rng, n, nb, oar):
    shape, dtype = OBS[nb]
    if dtype == np.uint8:
        o = rng.integers(1, 256, (n,) + shape, dtype=np.uint8)
    else:
        o = rng.standard_normal((n,) + shape).astype(np.float32)
    if oar:
        return OAR(o, rng.integers(1, 1 << 20, n).astype(np.int32),
                   rng.standard_normal(n).astype(np.float32))
    return o


def _episodes(rng, lengths, nb, oar):
    return [(_obs(rng, L, nb, oar), rng.integers(1, 1 << 20, L).astype(np.int32),
             (rng.standard_normal(L) * 3).astype(np.float32),
             rng.uniform(0.5, 1.0, L).astype(np.float32)) for L in lengths]


def _item(rng, nb, oar, T, i):
    """A stored sequence without a zero byte pattern in its flag and extras fields, so that
    an overlay that skipped them would show."""
    return adders.Step(
        observation=_obs(rng, T, nb, oar), action=np.full(T, -1 - i, np.int32),
        reward=rng.standard_normal(T).astype(np.float32),
        discount=np.full(T, 0.25, np.float32), start_of_episode=np.full(T, i % 2 == 0),
        extras={"core_state": LSTMState(rng.uniform(1, 2, (T, H)).astype(np.float32),
                                        rng.uniform(1, 2, (T, H)).astype(np.float32))})


def _table(nb, oar, T, items, seed, capacity=None, sampler=None):
    """A sequence table holding `items` random T-step items (the same for equal arguments);
    item i has priority 1 + i / 100."""
    rng = np.random.default_rng(1000 + items)
    table = replay.Table(NAME, sampler or replay.selectors.Uniform(), replay.selectors.Fifo(),
                         capacity or max(items, 1), replay.rate_limiters.MinSize(1),
                         signature=_signature(nb, oar), seed=seed)
    for i in range(items):
        table.insert(_item(rng, nb, oar, T, i), 1.0 + 0.01 * i)
    table.flush()
    assert table.sequence_length == T
    return table


def _host(sample):
    torch.cuda.synchronize()
    info = sample.info
    return dict(keys=info.key.view(torch.int64).cpu().numpy().view(np.uint64),
                probability=info.probability.cpu().numpy(),
                table_size=info.table_size.cpu().numpy(), priority=info.priority.cpu().numpy(),
                data=[x.cpu().numpy() for x in tree.flatten(sample.data)])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


INFO = ("keys", "probability", "table_size", "priority")


def _assert_same(got, want, tag):
    for k in INFO:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{tag} {k}")
    assert len(got["data"]) == len(want["data"])
    for f, (g, w) in enumerate(zip(got["data"], want["data"])):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, f)
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=f"{tag} field {f}")


def _check_batch(got, plain, is_demo_gpu, episodes, lengths, step, ratio, period, T, B, tag):
    """`got` (a mixed batch) against the oracle's overlay of `plain` (the twin's batch)."""
    is_demo, rows = O.mix(lengths, MIX_SEED, step, ratio, period, T, B)
    np.testing.assert_array_equal(is_demo_gpu, is_demo.astype(np.uint8), err_msg=f"{tag} is_demo")
    leaves = [tree.flatten(tuple(ep)) for ep in episodes]
    K = len(leaves[0])
    want = {k: (v.copy() if k != "data" else [x.copy() for x in v]) for k, v in plain.items()}
    assert len(want["data"]) == K + 3  # + start_of_episode and the two extras leaves
    for j, (e, first, to) in rows.items():
        want["keys"][j] = O.DEMO_KEY
        want["probability"][j] = 1.0
        want["table_size"][j] = 1
        want["priority"][j] = 1.0
        for k in range(K):
            want["data"][k][j] = O.window(leaves[e][k], first, to, T)
        want["data"][K][j] = first == 0
        for x in want["data"][K + 1:]:
            x[j] = 0
    _assert_same(got, want, tag)
    return is_demo


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_mixed_sequences_equal_oracle(case):
    nb, oar, T, B, lengths, period, ratio = case
    rng = np.random.default_rng([nb, T, B, period])
    episodes = _episodes(rng, lengths, nb, oar)
    items = 20 if nb < 1024 else 4
    table, twin = (_table(nb, oar, T, items, seed=9) for _ in range(2))
    assert table.fields[0].nbytes == T * nb
    store = SequenceDemonstrationStore(episodes, table)
    mixed = iter(mix_sequence_demonstrations(make_reverb_dataset(table, batch_size=B), store,
                                             ratio, period, T, seed=MIX_SEED))
    plain = iter(make_reverb_dataset(twin, batch_size=B))
    assert mixed.holds_last_batches == 2 and mixed.last_frames_f16 is None
    demos = 0
    for step in range(DRAWS):
        got = _host(next(mixed))
        flags = mixed.last_is_demo.cpu().numpy()
        ref = _host(next(plain))
        if ratio == 0.0:  # the plain dataset's batch, bit for bit
            _assert_same(got, ref, f"{case_id(case)} draw {step} plain")
        demos += _check_batch(got, ref, flags, episodes, lengths, step, ratio, period, T, B,
                              f"{case_id(case)} draw {step}").sum()
    if ratio in (0.0, 1.0):
        assert demos == int(ratio) * DRAWS * B
    else:
        assert 0 < demos < DRAWS * B


def test_sequence_length_and_layout_mismatch():
    rng = np.random.default_rng(0)
    table = _table(12, False, 9, 6, seed=1)
    store = SequenceDemonstrationStore(_episodes(rng, [5, 6], 12, False), table)
    with pytest.raises(ValueError, match="sequence_length 8 is not the table's 9"):
        mix_sequence_demonstrations(make_reverb_dataset(table, batch_size=4), store, 0.5, 1, 8)
    with pytest.raises(ValueError, match="per-step fields"):
        mix_sequence_demonstrations(make_reverb_dataset(_table(16, False, 9, 6, seed=1),
                                                        batch_size=4), store, 0.5, 1, 9)
    # a table whose sequence length is fixed only by its first item: refused at the first draw
    late = replay.Table(NAME, replay.selectors.Uniform(), replay.selectors.Fifo(), 10,
                        replay.rate_limiters.MinSize(1), signature=_signature(12, False), seed=1)
    it = iter(mix_sequence_demonstrations(make_reverb_dataset(late, batch_size=4), store, 0.5, 1,
                                          8))
    late.insert(_item(rng, 12, False, 9, 0), 1.0)
    with pytest.raises(ValueError, match="sequence_length 8 is not the table's 9"):
        next(it)
    # one store serves two datasets (it is immutable)
    a = iter(mix_sequence_demonstrations(make_reverb_dataset(table, batch_size=4), store, 1.0, 2,
                                         9))
    b = iter(mix_sequence_demonstrations(make_reverb_dataset(_table(12, False, 9, 6, seed=1),
                                                             batch_size=4), store, 1.0, 2, 9))
    _assert_same(_host(next(a)), _host(next(b)), "two datasets")


def test_prefetch_depth_does_not_change_the_batches():
    """Prefetch 3 issues draw j at next() number j - 3, so an insert made after next() number
    i precedes draw i + 4; the unprefetched run makes the same inserts before the same draw.
    The overlay must stay with its batch in the ring and precede the batch's ready event."""
    nb, oar, T, B, P, period, ratio, iters = 16, True, 9, 33, 3, 4, 0.5, 10
    rng = np.random.default_rng(5)
    episodes = _episodes(rng, [1, 2, 9, 40, 4, 17], nb, oar)
    new = [_item(rng, nb, oar, T, 100 + i) for i in range(iters * 3)]

    def run(prefetch):
        table = _table(nb, oar, T, 10, seed=3, capacity=200)
        store = SequenceDemonstrationStore(episodes, table)
        it = iter(mix_sequence_demonstrations(
            make_reverb_dataset(table, batch_size=B, prefetch_size=prefetch), store, ratio,
            period, T, seed=MIX_SEED))

        def insert(i):
            for item in new[3 * i:3 * i + 3]:
                table.insert(item, 1.0)
            table.flush()

        out = []
        for j in range(iters):
            if prefetch == 0 and j - P - 1 >= 0:
                insert(j - P - 1)
            s = next(it)
            flags = it.last_is_demo
            if prefetch:
                insert(j)  # queued right behind next(), no synchronisation
            out.append((_host(s), flags.cpu().numpy()))
        return out

    a, b = run(0), run(P)
    sizes = set()
    for j, ((x, fx), (y, fy)) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(fx, fy, err_msg=f"draw {j}")
        _assert_same(x, y, f"draw {j}")
        sizes.update(x["table_size"][fx == 0].tolist())
        assert 0 < fx.sum() < B
    assert len(sizes) > 1, "the inserts never became visible"


# ------------------------------------------------------------------ the sentinel key
CAP, ALPHA = 1000, 0.6


def _tree_state(native):
    from tests._oracle import computed_top, native_total
    state = native.debug_state()
    levels = native.debug_levels()
    if computed_top([len(x) for x in levels]):
        levels = levels[:-1]  # not maintained by the one-launch update: the total is compared
    return state, levels, native_total(native)


@pytest.mark.parametrize("items", [100, 700])  # slot 614 empty, then holding key 614
def test_sentinel_key_through_update_priorities(items):
    assert int(O.DEMO_KEY) % CAP == 614
    nb, oar, T, B = 12, False, 2, 64
    table, twin = (_table(nb, oar, T, items, seed=31, capacity=CAP,
                          sampler=replay.selectors.Prioritized(ALPHA)) for _ in range(2))
    rng = np.random.default_rng(items)
    store = SequenceDemonstrationStore(_episodes(rng, [1, 2, 9, 40, 4, 17], nb, oar), table)
    it = iter(mix_sequence_demonstrations(make_reverb_dataset(table, batch_size=B), store, 0.5,
                                          1, T, seed=MIX_SEED))
    got = _host(next(it))
    keys, demo = got["keys"], it.last_is_demo.cpu().numpy().astype(bool)
    assert 0 < demo.sum() < B and (keys[~demo] < items).all()
    assert (keys[demo] == O.DEMO_KEY).all()
    before = _tree_state(twin.native)
    clients = [replay.Client(replay.Server([t], port=None)) for t in (table, twin)]
    p = rng.uniform(0.1, 5.0, B)
    as_keys = lambda k: torch.as_tensor(  # noqa: E731
        np.ascontiguousarray(k).view(np.int64)).cuda().view(torch.uint64)
    clients[0].update_priorities(NAME, as_keys(keys), torch.as_tensor(p).cuda())
    clients[1].update_priorities(NAME, as_keys(keys[~demo]), torch.as_tensor(p[~demo]).cuda())
    torch.cuda.synchronize()
    (sa, la, ta), (sb, lb, tb) = _tree_state(table.native), _tree_state(twin.native)
    for k in ("leaves", "raw", "keys"):
        np.testing.assert_array_equal(_bits(sa[k]), _bits(sb[k]), err_msg=k)
    assert len(la) == len(lb)
    for l, (x, y) in enumerate(zip(la, lb)):
        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=f"level {l}")
    assert _bits(np.float64(ta)).tolist() == _bits(np.float64(tb)).tolist()
    assert not np.array_equal(before[0]["leaves"], sb["leaves"]), "the updates never landed"


# ------------------------------------------------------------------ learner and agent
def _oar_episode(rng, L, A, obs_dim):
    act = rng.integers(0, A, L).astype(np.int32)
    rew = (0.3 * rng.standard_normal(L)).astype(np.float32)
    obs = OAR(rng.standard_normal((L, obs_dim)).astype(np.float32),
              np.concatenate([[0], act[:-1]]).astype(np.int32),
              np.concatenate([[0], rew[:-1]]).astype(np.float32))
    dis = np.ones(L, np.float32)
    dis[-1] = 0.0
    return obs, act, rew, dis


def test_teacher_forced_step():
    """R2D2Learner.step() with store_lstm_state=False fed by the mix from a Uniform table,
    against the oracle on the very batches drawn (demonstration rows among them): loss and
    priorities at tests/test_r2d2_agent_gpu.py's shapes and tolerances."""
    from acme_amd.agents.r2d2.learning import R2D2Learner
    from acme_amd.networks import R2D2AtariNetwork
    from acme_amd.testing import fakes
    from acme_amd.utils import loggers
    from acme_amd.wrappers import ObservationActionRewardWrapper
    from oracle import r2d2_oracle as R
    from tests.test_r2d2_agent_gpu import _Recorder, _drive
    A, Hn, obs_dim, B = 5, 16, 6, 4
    burn, trace, period, n_step, size = 2, 5, 3, 3, 1000
    T = burn + trace + 1
    env = ObservationActionRewardWrapper(fakes.DiscreteEnvironment(num_actions=A,
                                                                   obs_shape=(obs_dim,)))
    spec = specs.make_environment_spec(env)
    extra = {"core_state": LSTMState(specs.Array((Hn,), np.float32),
                                     specs.Array((Hn,), np.float32))}
    table = replay.Table(NAME, replay.selectors.Uniform(), replay.selectors.Fifo(), size,
                         replay.rate_limiters.MinSize(1),
                         signature=adders.SequenceAdder.signature(spec, extra), seed=1234)
    server = replay.Server([table], port=None)
    adder = adders.SequenceAdder(client=replay.Client(server), period=period, sequence_length=T)
    _drive(adder, np.random.default_rng(0), A, obs_dim, Hn)
    table.flush()
    assert table.size() > 2 * B and table.sequence_length == T
    rng = np.random.default_rng(3)
    store = SequenceDemonstrationStore([_oar_episode(rng, L, A, obs_dim) for L in (17, 5, 30)],
                                       table)
    mixed = mix_sequence_demonstrations(
        make_reverb_dataset(server_address=server, batch_size=B, sequence_length=T), store, 0.5,
        period, T, seed=MIX_SEED)
    net = R2D2AtariNetwork(A, lstm_size=Hn, head_size=8, torso="flat", obs_dim=obs_dim)
    rec = _Recorder(mixed)
    learner = R2D2Learner(spec, net, net, dataset=rec, burn_in_length=burn, sequence_length=T,
                          reverb_client=replay.Client(server), logger=loggers.NoOpLogger(),
                          n_step=n_step, target_update_period=2, max_replay_size=size,
                          batch_size=B, seed=5, store_lstm_state=False)
    cfg = R.R2D2Config(num_actions=A, torso="flat", obs_dim=obs_dim, lstm_size=Hn, head_size=8,
                       burn_in_length=burn, n_step=n_step, max_replay_size=size,
                       target_update_period=2, store_lstm_state=False)
    n = learner.native
    demos = replays = 0
    for k in range(3):
        params, target = n.get_params("params"), n.get_params("target")
        learner.step()
        torch.cuda.synchronize()
        b = rec.samples[-1]
        demo = b["keys"].view(np.uint64) == O.DEMO_KEY
        demos, replays = demos + int(demo.sum()), replays + int((~demo).sum())
        assert (b["probabilities"][demo] == 1.0).all()
        assert not b["state"][demo].any() and b["state"][~demo].any()
        ref, _ = R.loss_and_grads(cfg, params, target, b)
        np.testing.assert_allclose(n.loss.item(), ref["loss"], rtol=2e-4,
                                   err_msg=f"loss step {k}")
        np.testing.assert_allclose(n.priorities[:B].cpu().numpy(), ref["priorities"],
                                   atol=2.5e-4, rtol=1e-4, err_msg=f"priorities step {k}")
    assert demos > 0 and replays > 0
    assert n.guard_state()["applied"] == 3


def test_agent_runs():
    """agents/tf/r2d3/agent_test.py: 5 episodes of 10 steps, batch 10, ratio 0.5."""
    from acme_amd import dm_env
    from acme_amd.agents.dqfd import DemonstrationRecorder
    from acme_amd.agents.r2d3 import R2D3
    from acme_amd.environment_loop import EnvironmentLoop
    from acme_amd.networks import R2D2AtariNetwork
    from acme_amd.testing import fakes
    from acme_amd.utils import loggers
    from acme_amd.wrappers import ObservationActionRewardWrapper
    A, obs_dim = 5, 6
    environment = ObservationActionRewardWrapper(
        fakes.DiscreteEnvironment(num_actions=A, obs_shape=(obs_dim,), episode_length=10))
    spec = specs.make_environment_spec(environment)
    dummy_action = np.zeros((), dtype=np.int32)
    recorder = DemonstrationRecorder()
    timestep = environment.reset()
    while timestep.step_type is not dm_env.StepType.LAST:
        recorder.step(timestep, dummy_action)
        timestep = environment.step(dummy_action)
    recorder.step(timestep, dummy_action)
    recorder.record_episode()
    net = R2D2AtariNetwork(A, lstm_size=16, head_size=8, torso="flat", obs_dim=obs_dim)
    log = loggers.InMemoryLogger()
    agent = R2D3(environment_spec=spec, network=net, target_network=None,
                 demonstration_dataset=recorder.make_tf_dataset(), demonstration_ratio=0.5,
                 batch_size=10, samples_per_insert=2, min_replay_size=10, burn_in_length=2,
                 trace_length=6, replay_period=4, checkpoint=False, logger=log)
    EnvironmentLoop(environment, agent, logger=loggers.NoOpLogger()).run(num_episodes=5)
    torch.cuda.synchronize()
    learner = agent.learner
    assert learner.num_steps > 0 and np.isfinite(learner.native.loss.item())
    g = learner.native.guard_state()
    assert g["skipped"] == 0 and g["applied"] == learner.num_steps
    table = agent.server.tables[NAME]
    assert table.sequence_length == 9 and not table.native.prioritized
    it = learner._iterator
    seen = 0
    for _ in range(4):
        got = _host(next(it))
        demo = it.last_is_demo.cpu().numpy().astype(bool)
        np.testing.assert_array_equal(got["keys"] == O.DEMO_KEY, demo)
        np.testing.assert_array_equal(got["data"][3][demo], 0)  # the demonstrations' action
        seen += int(demo.sum())
    assert 0 < seen < 40
