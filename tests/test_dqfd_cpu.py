"""DQfD without a GPU: the numpy oracle of the demonstration mix (tests/dqfd_oracle.py)
against hand-computed values and against itself (f32 vs f64, draw frequencies), the
DemonstrationRecorder, and every refusal of DemonstrationStore / mix_demonstrations."""

import math

import numpy as np
import pytest

from acme_amd import dm_env, replay, specs
from acme_amd.agents.dqfd import DemonstrationRecorder
from acme_amd.datasets import DemonstrationStore, mix_demonstrations
from acme_amd.datasets.reverb import ReplayDataset
from tests import dqfd_oracle as O


# ------------------------------------------------------------------ n-step return
def test_hand_computed_episode():
    """L = 6, n = 3, gamma = 0.5; every product below is exact in f32.  The reward is
    shifted by one step, the discounts are not, so d[last - 1] never enters."""
    rewards = np.array([9, 1, 2, 4, 8, 16], np.float32)        # rewards[0] is never read
    discounts = np.array([7, 0.5, 0.25, 1, 1, 0], np.float32)  # nor are the last two here
    # first = 1: last = min(1 + 3, 5) = 4, m = 3:
    #   r_t = r[2] + r[3] * d[1] g + r[4] * d[1] d[2] g^2 = 2 + 4 * .25 + 8 * .03125 = 3.25
    #   d_t = d[1] d[2] g^2 = .03125
    assert O.span(1, 3, 6) == (4, 3)
    assert O.nstep_f32(rewards, discounts, 1, 3, 0.5) == (np.float32(3.25), np.float32(0.03125))
    r64, d64, mass = O.nstep_f64(rewards, discounts, 1, 3, 0.5)
    assert (r64, d64, mass) == (3.25, 0.03125, 3.25)
    # first = 3 = L - 3 (the largest first): last = min(6, 5) = 5, m = 2:
    #   r_t = r[4] + r[5] * d[3] g = 8 + 16 * .5 = 16;  d_t = d[3] g = .5
    assert O.span(3, 3, 6) == (5, 2)
    assert O.nstep_f32(rewards, discounts, 3, 3, 0.5) == (np.float32(16), np.float32(0.5))
    assert O.nstep_f64(rewards, discounts, 3, 3, 0.5)[:2] == (16.0, 0.5)
    # first = 0, n = 1: one term, r_t = r[1], d_t = 1 (an empty product)
    assert O.nstep_f32(rewards, discounts, 0, 1, 0.5) == (np.float32(1), np.float32(1))
    assert O.nstep_f64(rewards, discounts, 0, 1, 0.5)[:2] == (1.0, 1.0)
    # a zero discount inside the window zeroes every later term
    discounts[2] = 0
    assert O.nstep_f32(rewards, discounts, 1, 3, 0.5) == (np.float32(3), np.float32(0))


@pytest.mark.parametrize("n_step", [1, 2, 5, 12, 50])
def test_f32_within_rounding_bound_of_f64(n_step):
    """Each term r * (c_k * g_k) carries at most k roundings in g_k, k in c_k, one in their
    product and one in the term's: 2 k + 2 <= 2 n; the running sum adds at most n - 1 more
    per term.  (3 n + 3) * 2^-24 * sum |term| bounds that to first order; d_t is one
    product chain, 2 n + 1 roundings."""
    rng = np.random.default_rng(n_step)
    u = 2.0 ** -24
    for _ in range(200):
        L = int(rng.integers(3, 41))
        rewards = rng.standard_normal(L).astype(np.float32)
        discounts = rng.uniform(0.3, 1.0, L).astype(np.float32)
        gamma = float(rng.uniform(0.8, 1.0))
        first = int(rng.integers(0, L - 2))
        r32, d32 = O.nstep_f32(rewards, discounts, first, n_step, gamma)
        r64, d64, mass = O.nstep_f64(rewards, discounts, first, n_step, gamma)
        assert r32.dtype == np.float32 and d32.dtype == np.float32
        assert abs(float(r32) - r64) <= (3 * n_step + 3) * u * mass
        assert abs(float(d32) - d64) <= (3 * n_step + 3) * u * d64


# ------------------------------------------------------------------ draw mapping
N_DRAWS = 10240


def _within(count, n, p):
    return abs(count - n * p) <= 5.0 * math.sqrt(n * p * (1.0 - p))


@pytest.mark.parametrize("ratio", [0.25, 0.5])
def test_demonstration_share(ratio):
    lengths = [3, 9, 40]
    hits = sum(O.draw(seed=77, step=j // 512, j=j % 512, ratio=ratio, lengths=lengths)[0]
               for j in range(N_DRAWS))
    assert _within(hits, N_DRAWS, ratio), hits
    assert not any(O.draw(77, 0, j, 0.0, lengths)[0] for j in range(64))
    assert all(O.draw(77, 0, j, 1.0, lengths)[0] for j in range(64))


def test_episode_index_uniform():
    lengths = [3, 4, 5, 6, 7, 8, 9]
    counts = np.zeros(len(lengths), np.int64)
    for j in range(N_DRAWS):
        counts[O.draw(5, j // 512, j % 512, 0.5, lengths)[1]] += 1
    assert counts.sum() == N_DRAWS
    assert all(_within(c, N_DRAWS, 1.0 / len(lengths)) for c in counts), counts


def test_first_step_uniform_and_in_range():
    L = 12  # first in [0, 10)
    counts = np.zeros(L, np.int64)
    for j in range(N_DRAWS):
        counts[O.draw(6, j // 512, j % 512, 0.5, [L])[2]] += 1
    assert counts[L - 2:].sum() == 0, counts
    assert all(_within(c, N_DRAWS, 1.0 / (L - 2)) for c in counts[:L - 2]), counts
    # L = 3: the only first step is 0
    assert {O.draw(6, 0, j, 0.5, [3])[2] for j in range(256)} == {0}


def test_draw_depends_on_step_seed_and_row():
    a = [O.draw(1, 0, j, 0.5, [30, 40]) for j in range(64)]
    assert a != [O.draw(1, 1, j, 0.5, [30, 40]) for j in range(64)]
    assert a != [O.draw(2, 0, j, 0.5, [30, 40]) for j in range(64)]
    assert a != [O.draw(1, 1 << 32, j, 0.5, [30, 40]) for j in range(64)]  # the high word
    assert len(set(a)) > 32


# ------------------------------------------------------------------ recorder
def test_recorder_follows_the_reference():
    rec = DemonstrationRecorder()
    assert rec.episode_reward == 0
    obs = [np.full((2,), i, np.float32) for i in range(4)]
    steps = [dm_env.restart(obs[0]), dm_env.transition(1.5, obs[1]),
             dm_env.transition(2.0, obs[2], discount=0.5), dm_env.termination(4.0, obs[3])]
    for i, ts in enumerate(steps):
        rec.step(ts, np.asarray(i, np.int32))
    assert rec.episode_reward == np.float32(7.5)
    rec.discard_episode()
    assert rec.episode_reward == 0
    with pytest.raises(ValueError):
        rec.make_dataset()
    for i, ts in enumerate(steps):
        rec.step(ts, np.asarray(i, np.int32))
    rec.record_episode()
    assert rec.episode_reward == 0
    rec.step(steps[0], np.asarray(0, np.int32))  # an unfinished episode is not part of it
    demos = rec.make_dataset()
    assert rec.make_tf_dataset() == demos and len(demos) == 1
    o, a, r, d = demos[0]
    np.testing.assert_array_equal(o, np.stack(obs))
    assert a.dtype == np.int32 and a.tolist() == [0, 1, 2, 3]
    # the first step's missing reward and discount are 0, the last step's discount is 0
    assert r.dtype == np.float32 and r.tolist() == [0.0, 1.5, 2.0, 4.0]
    assert d.dtype == np.float32 and d.tolist() == [0.0, 1.0, 0.5, 0.0]


# ------------------------------------------------------------------ refusals
def _signature(obs_shape=(3,), obs_dtype=np.float32):
    o = specs.Array(obs_shape, obs_dtype, "observation")
    return (o, specs.Array((), np.int32, "action"), specs.Array((), np.float32, "reward"),
            specs.Array((), np.float32, "discount"), o)


def _episode(L, obs_shape=(3,)):
    return (np.zeros((L,) + obs_shape, np.float32), np.zeros(L, np.int32),
            np.zeros(L, np.float32), np.ones(L, np.float32))


def _plain_table():
    return replay.Table("t", replay.selectors.Uniform(), replay.selectors.Fifo(), 100)


def test_store_layout_without_a_gpu():
    store = DemonstrationStore([_episode(3), _episode(7)], _signature())
    assert store.num_episodes == 2 and store.offsets.tolist() == [0, 3, 10]
    assert (store.obs_row_bytes, store.action_row_bytes) == (12, 4)


@pytest.mark.parametrize("L", [0, 1, 2])
def test_short_episode_is_refused(L):
    with pytest.raises(ValueError, match="at least 3"):
        DemonstrationStore([_episode(5), _episode(L)], _signature())


def test_no_episodes_is_refused():
    with pytest.raises(ValueError, match="no demonstration episodes"):
        DemonstrationStore([], _signature())


def test_row_mismatch_is_refused():
    with pytest.raises(ValueError, match="do not match"):
        DemonstrationStore([_episode(5, obs_shape=(4,))], _signature(obs_shape=(3,)))
    store = DemonstrationStore([_episode(5)], _signature())
    # a store built for other row bytes than the table's
    store.obs_row_bytes = 16
    table = _plain_table()
    table._fields = replay._layout_from_signature(_signature())  # the layout, no storage
    with pytest.raises(ValueError, match="16-byte observation"):
        mix_demonstrations(ReplayDataset(table, 4), store, 0.5, 1, 0.99)


def test_unsupported_tables_are_refused():
    store = DemonstrationStore([_episode(5)], _signature())
    frame = replay.FrameTable.__new__(replay.FrameTable)  # refused by type, before any use
    queue = replay.QueueTable("q", 8)
    for table in (frame, queue):
        with pytest.raises(ValueError, match="transition tables"):
            mix_demonstrations(ReplayDataset(table, 4), store, 0.5, 1, 0.99)
        with pytest.raises(ValueError, match="transition tables"):
            DemonstrationStore([_episode(5)], table)


def test_global_sampling_is_refused():
    store = DemonstrationStore([_episode(5)], _signature())
    with pytest.raises(ValueError, match="global sampling"):
        mix_demonstrations(ReplayDataset(_plain_table(), 4, global_sampling=True), store, 0.5,
                           1, 0.99)


def test_f16_dataset_copy_is_refused(monkeypatch):
    store = DemonstrationStore([_episode(5)], _signature())
    monkeypatch.setenv("ACME_DATASET_F16", "1")
    with pytest.raises(ValueError, match="ACME_DATASET_F16"):
        mix_demonstrations(ReplayDataset(_plain_table(), 4), store, 0.5, 1, 0.99)


@pytest.mark.parametrize("ratio", [-0.01, 1.01, float("nan"), float("inf")])
def test_ratio_outside_unit_interval_is_refused(ratio):
    store = DemonstrationStore([_episode(5)], _signature())
    with pytest.raises(ValueError, match="outside"):
        mix_demonstrations(ReplayDataset(_plain_table(), 4), store, ratio, 1, 0.99)


def test_accepted_arguments_build_a_dataset():
    store = DemonstrationStore([_episode(5)], _signature())
    for ratio in (0.0, 0.25, 1.0):
        ds = mix_demonstrations(ReplayDataset(_plain_table(), 4, prefetch=4), store, ratio, 5,
                                0.99, seed=3)
        assert ds.batch_size == 4 and ds.demonstration_ratio == ratio
