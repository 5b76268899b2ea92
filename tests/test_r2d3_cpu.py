"""R2D3's data path without a GPU: the numpy oracle of the sequence demonstration mix
(tests/r2d3_oracle.py) against the reference's window rule and against itself (draw
frequencies), every refusal of SequenceDemonstrationStore / mix_sequence_demonstrations, and
the coverage of the GPU test's cases (tests/r2d3_cases.py) on the oracle alone."""

import math

import numpy as np
import pytest

from acme_amd import replay, specs
from acme_amd.adders import reverb as adders
from acme_amd.datasets import (SequenceDemonstrationStore, make_reverb_dataset,
                               mix_sequence_demonstrations)
from acme_amd.wrappers import OAR
from tests import r2d3_oracle as O
from tests.r2d3_cases import CASES, DRAWS, MIX_SEED

LENGTHS = [1, 2, 9, 40, 4, 17]


# ------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("period", [1, 4, 64])
@pytest.mark.parametrize("T", [2, 9])
def test_window_properties(period, T):
    seen = set()
    for j in range(2048):
        _, e, first, to = O.draw(11, j // 256, j % 256, 0.5, LENGTHS, period, T)
        L = LENGTHS[e]
        assert 0 <= e < len(LENGTHS)
        assert first % period == 0 and 0 <= first < L
        assert 0 < to - first <= T and to == min(first + T, L)
        seen.add((e, first))
    # every multiple of the period below L is a possible first step, and is drawn
    want = {(e, f) for e, L in enumerate(LENGTHS) for f in range(0, L, period)}
    assert seen == want


def test_window_is_the_references_slice_and_pad():
    x = np.arange(1, 11, dtype=np.float32).reshape(5, 2)
    np.testing.assert_array_equal(O.window(x, 4, 5, 3), [[9, 10], [0, 0], [0, 0]])
    np.testing.assert_array_equal(O.window(x, 0, 3, 3), x[:3])
    assert O.window(x, 2, 5, 4).dtype == np.float32


def _within(count, n, p):
    return abs(count - n * p) <= 5.0 * math.sqrt(n * p * (1.0 - p))


@pytest.mark.parametrize("ratio", [0.25, 0.5])
def test_demonstration_share(ratio):
    n = 8192
    hits = sum(O.draw(77, j // 512, j % 512, ratio, LENGTHS, 4)[0] for j in range(n))
    assert _within(hits, n, ratio), hits
    assert not any(O.draw(77, 0, j, 0.0, LENGTHS, 4)[0] for j in range(64))
    assert all(O.draw(77, 0, j, 1.0, LENGTHS, 4)[0] for j in range(64))


def test_draws_differ_from_the_transition_mix():
    from tests import dqfd_oracle as D
    lengths = [40] * 8
    a = [O.draw(5, 0, j, 0.5, lengths, 1)[:2] for j in range(64)]
    b = [D.draw(5, 0, j, 0.5, lengths)[:2] for j in range(64)]
    assert a != b


def test_gpu_cases_cover_their_purpose():
    """The seeds and draw counters of test_r2d3_gpu's cases yield, on the oracle: a padded and
    an unpadded window, a window at an episode's start and one inside it; and in every case
    with 0 < ratio < 1 both a demonstration and a replay row."""
    kinds = set()
    values = {k: set() for k in range(7)}
    for case in CASES:
        nb, oar, T, B, lengths, period, ratio = case
        for k, v in enumerate(case):
            values[k].add(tuple(v) if isinstance(v, list) else v)
        demos = replays = 0
        for step in range(DRAWS):
            is_demo, rows = O.mix(lengths, MIX_SEED, step, ratio, period, T, B)
            demos += int(is_demo.sum())
            replays += int((~is_demo).sum())
            for e, first, to in rows.values():
                kinds.add("padded" if to - first < T else "unpadded")
                kinds.add("first == 0" if first == 0 else "first > 0")
        if 0.0 < ratio < 1.0:
            assert demos and replays, case
        elif ratio == 0.0:
            assert not demos
        else:
            assert not replays
    assert kinds == {"padded", "unpadded", "first == 0", "first > 0"}
    # the parameter values the cases are meant to span
    assert values[0] == {3, 12, 16, 28224}
    assert {(nb, oar) for nb, oar, *_ in CASES} >= {(12, True), (28224, True)}
    assert values[2] >= {2, 9} and all(T == 5 for nb, _, T, *_ in CASES if nb == 28224)
    assert values[3] == {1, 5, 33}
    assert values[4] == {(1, 2, 9, 40, 4, 17), (1,)}
    assert values[5] == {1, 4, 64} and values[6] == {0.0, 0.25, 0.5, 1.0}


# ------------------------------------------------------------------ refusals
H = 4


def _spec(obs=specs.Array((3,), np.float32, "observation"), oar=False):
    action, reward = specs.Array((), np.int32, "action"), specs.Array((), np.float32, "reward")
    if oar:
        obs = OAR(obs, action, reward)
    return specs.EnvironmentSpec(obs, action, reward, specs.Array((), np.float32, "discount"))


EXTRAS = {"core_state": (specs.Array((H,), np.float32), specs.Array((H,), np.float32))}


def _signature(**kw):
    return adders.SequenceAdder.signature(_spec(**kw), EXTRAS)


def _episode(L, oar=False, obs_shape=(3,), obs_dtype=np.float32, action_dtype=np.int32):
    rng = np.random.default_rng(L)
    obs = rng.integers(0, 200, (L,) + obs_shape).astype(obs_dtype)
    act = rng.integers(0, 5, L).astype(action_dtype)
    rew = rng.standard_normal(L).astype(np.float32)
    if oar:
        obs = OAR(obs, act.astype(np.int32), rew)
    return obs, act, rew, np.ones(L, np.float32)


def _table(signature=None):
    """A table that knows its item layout but has no device storage (a Table constructed
    with a signature allocates it): what the checks here read is the layout alone."""
    signature = signature if signature is not None else _signature()
    t = replay.Table(adders.DEFAULT_PRIORITY_TABLE, replay.selectors.Uniform(),
                     replay.selectors.Fifo(), 10, replay.rate_limiters.MinSize(1))
    t._signature = t._structure = signature
    t._fields = replay._layout_from_signature(signature)
    return t


def test_store_accepts_plain_and_nested_observations():
    s = SequenceDemonstrationStore([_episode(1), _episode(7)], _signature())
    assert s.num_episodes == 2 and [f.nbytes for f in s.step_fields] == [12, 4, 4, 4]
    s = SequenceDemonstrationStore([_episode(3, oar=True)], _table(_signature(oar=True)))
    assert [f.nbytes for f in s.step_fields] == [12, 4, 4, 4, 4, 4]
    np.testing.assert_array_equal(s.offsets, [0, 3])
    # leaves of the same kind are converted to the field's dtype
    s = SequenceDemonstrationStore([_episode(3, action_dtype=np.int64)], _signature())
    assert s._host[1].shape == (3, 4)
    # a 3-byte step is packed without padding
    u8 = _signature(obs=specs.Array((3,), np.uint8, "observation"))
    s = SequenceDemonstrationStore([_episode(5, obs_dtype=np.uint8)], u8)
    assert s._host[0].shape == (5, 3)


def test_store_refusals():
    sig = _signature()
    with pytest.raises(ValueError, match="no demonstration episodes"):
        SequenceDemonstrationStore([], sig)
    o, a, r, d = _episode(5)
    with pytest.raises(ValueError, match="length"):
        SequenceDemonstrationStore([(o, a[:4], r, d)], sig)
    with pytest.raises(ValueError, match="length"):
        SequenceDemonstrationStore([(o, a, r, d[:3])], sig)
    with pytest.raises(ValueError, match="expected"):
        SequenceDemonstrationStore([(o, a, r)], sig)
    with pytest.raises(ValueError, match="shape"):
        SequenceDemonstrationStore([_episode(5, obs_shape=(4,))], sig)
    with pytest.raises(ValueError, match="cannot be stored"):  # float frames, uint8 field
        SequenceDemonstrationStore(
            [_episode(5)], _signature(obs=specs.Array((3,), np.uint8, "observation")))
    with pytest.raises(ValueError, match="cannot be stored"):  # float actions, int32 field
        SequenceDemonstrationStore([_episode(5, action_dtype=np.float32)], sig)
    with pytest.raises(ValueError, match="leaves"):  # a plain observation for an OAR table
        SequenceDemonstrationStore([_episode(5)], _signature(oar=True))
    with pytest.raises(ValueError, match="at least 1"):  # an episode without steps
        SequenceDemonstrationStore([_episode(0)], sig)
    # K over the cap: an observation nest of 14 leaves + action, reward, discount = 17
    leaf = specs.Array((), np.float32)
    wide = adders.SequenceAdder.signature(_spec(obs=tuple([leaf] * 14)), EXTRAS)
    ep = (tuple(np.zeros(3, np.float32) for _ in range(14)), np.zeros(3, np.int32),
          np.zeros(3, np.float32), np.ones(3, np.float32))
    with pytest.raises(ValueError, match="at most 16"):
        SequenceDemonstrationStore([ep], wide)
    SequenceDemonstrationStore(
        [(ep[0][:13],) + ep[1:]],
        adders.SequenceAdder.signature(_spec(obs=tuple([leaf] * 13)), EXTRAS))  # K = 16


def test_native_store_refusals():
    from acme_amd.native import NativeDemoStore
    NativeDemoStore(np.array([0, 1]), [3])
    NativeDemoStore(np.array([0, 3]), [12, 4, 4, 4], min_episode_steps=3)
    for offsets, step_bytes in (([0], [4]), ([0, 0], [4]), ([0, 2, 2], [4]), ([0, 2], []),
                                ([0, 2], [4] * 17), ([0, 2], [4, 0]), ([1, 2], [4])):
        with pytest.raises(ValueError):
            NativeDemoStore(np.array(offsets), step_bytes)
    with pytest.raises(ValueError, match="at least 3"):
        NativeDemoStore(np.array([0, 2]), [4], min_episode_steps=3)


def test_transition_mix_refuses_other_stores_without_a_device():
    """acme_demo_mix checks what it asks of the store (four fields, f32 rewards and
    discounts, rows of multiples of 4 bytes, min_episode_steps >= 3) before anything that
    needs a device: the stores here were never uploaded, and the refusal names the layout."""
    import ctypes
    from acme_amd.native import NativeDemoStore
    ptrs = (ctypes.c_void_p * 5)()

    def mix(store):
        store.mix_transitions(0.5, 1, 0.99, 0, 0, 1, ptrs, 0, 0, 0, 0, stream=0)

    with pytest.raises(ValueError, match="min_episode_steps of at least 3"):
        mix(NativeDemoStore(np.array([0, 3]), [12, 4, 4, 4], min_episode_steps=1))
    for step_bytes in ([12, 4, 4], [12, 4, 4, 4, 4], [12, 4, 8, 4], [12, 4, 4, 2]):
        with pytest.raises(ValueError, match="four fields"):
            mix(NativeDemoStore(np.array([0, 3]), step_bytes, min_episode_steps=3))
    for step_bytes in ([3, 4, 4, 4], [12, 6, 4, 4]):
        with pytest.raises(ValueError, match="multiples of 4"):
            mix(NativeDemoStore(np.array([0, 3]), step_bytes, min_episode_steps=3))
    # a store of the right layout gets past these checks: it is refused for not being uploaded
    with pytest.raises(ValueError, match="not been uploaded"):
        mix(NativeDemoStore(np.array([0, 3]), [12, 4, 4, 4], min_episode_steps=3))


def test_transition_and_frame_tables_are_refused():
    o = specs.Array((3,), np.float32)
    transition = (o, specs.Array((), np.int32), specs.Array((), np.float32),
                  specs.Array((), np.float32), o)
    with pytest.raises(ValueError, match="sequence tables"):
        SequenceDemonstrationStore([_episode(5)], _table(transition))
    with pytest.raises(ValueError, match="sequence tables"):
        SequenceDemonstrationStore([_episode(5)], transition)
    store = SequenceDemonstrationStore([_episode(5)], _signature())
    with pytest.raises(ValueError, match="sequence tables"):
        mix_sequence_demonstrations(make_reverb_dataset(_table(transition), batch_size=2), store,
                                    0.5, 1, 3)
    frames = replay.FrameTable.__new__(replay.FrameTable)  # the type alone decides
    with pytest.raises(ValueError, match="FrameTable"):
        SequenceDemonstrationStore([_episode(5)], frames)
    from acme_amd.datasets.reverb import ReplayDataset
    with pytest.raises(ValueError, match="FrameTable"):
        mix_sequence_demonstrations(ReplayDataset(frames, 2), store, 0.5, 1, 3)
    with pytest.raises(ValueError, match="QueueTable"):
        mix_sequence_demonstrations(ReplayDataset(replay.QueueTable("q", 8), 2), store, 0.5, 1, 3)


def test_mix_refusals(monkeypatch):
    table = _table()
    store = SequenceDemonstrationStore([_episode(5), _episode(2)], table)
    dataset = make_reverb_dataset(table, batch_size=4)
    for ratio in (float("nan"), -0.01, 1.01):
        with pytest.raises(ValueError, match="outside"):
            mix_sequence_demonstrations(dataset, store, ratio, 1, 3)
    with pytest.raises(ValueError, match="period"):
        mix_sequence_demonstrations(dataset, store, 0.5, 0, 3)
    with pytest.raises(ValueError, match="sequence_length"):
        mix_sequence_demonstrations(dataset, store, 0.5, 1, 0)
    with pytest.raises(ValueError, match="SequenceDemonstrationStore"):
        mix_sequence_demonstrations(dataset, object(), 0.5, 1, 3)
    with pytest.raises(ValueError, match="make_reverb_dataset"):
        mix_sequence_demonstrations(object(), store, 0.5, 1, 3)
    with pytest.raises(ValueError, match="global sampling"):
        mix_sequence_demonstrations(make_reverb_dataset(table, batch_size=4,
                                                        global_sampling=True), store, 0.5, 1, 3)
    other = SequenceDemonstrationStore(
        [_episode(5, obs_shape=(4,))], _signature(obs=specs.Array((4,), np.float32)))
    with pytest.raises(ValueError, match="per-step fields"):
        mix_sequence_demonstrations(dataset, other, 0.5, 1, 3)
    monkeypatch.setenv("ACME_DATASET_F16", "1")
    with pytest.raises(ValueError, match="ACME_DATASET_F16"):
        mix_sequence_demonstrations(dataset, store, 0.5, 1, 3)
    monkeypatch.delenv("ACME_DATASET_F16")
    mixed = mix_sequence_demonstrations(dataset, store, 0.5, 4, 3, seed=-1)
    assert (mixed.batch_size, mixed.period, mixed.sequence_length) == (4, 4, 3)
    assert mixed.seed == 2 ** 64 - 1 and mixed.element_spec == dataset.element_spec
