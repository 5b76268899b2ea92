"""Demonstrations mixed into replay batches — the dataset side of DQfD
(acme/agents/tf/dqfd/agent.py:111-122).

The reference maps each demonstration episode to one n-step transition on a tf.data thread
(_n_step_transition_from_episode, agent.py:160-217) and interleaves the mapped dataset with
the Reverb stream, element by element, with sample_from_datasets([replay, demos],
[1 - ratio, ratio]).  Here the episodes are device arrays (`DemonstrationStore`) and the mix
is one kernel on the dataset's stream (acme_demo_mix, csrc/demos.hip): the table draws and
gathers its full batch, then each row independently becomes a demonstration with probability
`demonstration_ratio` and is overwritten with an n-step transition of a uniformly drawn
episode and first step.  The choice and the draws of row j of draw `step` are one Philox
call keyed by the mix's own seed, so a batch is a function of (table state, table seed, mix
seed, step) whatever the prefetch depth.

A demonstration row reports probability 1, table_size 1 and priority 1 like the
reference's, and the key DEMONSTRATION_KEY = 2**64 - 2 where the reference has 0: key 0 is
this table's first item, and all-ones marks an empty slot, so either would let the learner's
priority write-back touch the table; 2**64 - 2 equals no stored key and the write-back
drops it as stale.

The second half of the module is the same mix for sequence tables (R2D3):
`SequenceDemonstrationStore` and `mix_sequence_demonstrations`, on acme_seq_demo_mix (the
same file).  Both share the store's bookkeeping, the iterator, the refusals and the key.
"""

from __future__ import annotations

import os
from typing import Iterable, Sequence

import numpy as np
import torch

from acme_amd import replay
from acme_amd.adders import reverb as adders
from acme_amd.utils import tree
from acme_amd.datasets.reverb import ReplayDataset, _data_parallel, _TableIterator, _Unbatched

DEMONSTRATION_KEY = 0xFFFFFFFFFFFFFFFE


def _refuse_table(x, kind: str) -> None:
    """The tables no store can be laid out for (`kind`: "transition" or "sequence")."""
    if isinstance(x, (replay.FrameTable, replay.QueueTable)):
        raise ValueError(f"demonstrations are mixed into {kind} tables, not a "
                         f"{type(x).__name__}")
    if isinstance(x, replay.Table) and x.fields is None:
        raise ValueError("the table has no item layout yet: construct it with a signature")


def _transition_fields(table_or_signature):
    """The flattened field layout of a transition table, its signature, or a field list."""
    x = table_or_signature
    _refuse_table(x, "transition")
    if isinstance(x, replay.Table):
        fields = x.fields
    elif isinstance(x, (list, tuple)) and x and all(isinstance(f, replay._Field) for f in x):  # noqa: SLF001
        fields = list(x)
    else:
        fields = replay._layout_from_signature(x)  # noqa: SLF001
    if len(fields) < 5:
        raise ValueError("a transition layout (o_tm1, a_tm1, r_t, d_t, o_t) has five fields, "
                         f"got {len(fields)}")
    o, _, r, d, o2 = fields[:5]
    if (o.shape, o.dtype, o.row_bytes) != (o2.shape, o2.dtype, o2.row_bytes):
        raise ValueError("fields 0 and 4 (the two observations) differ")
    for f in (r, d):
        if f.dtype != np.float32 or f.shape != () or f.row_bytes != 4:
            raise ValueError("fields 2 and 3 (reward and discount) must be float32 scalars")
    return fields


class _Store:
    """What both stores keep: the episodes' lengths and offsets, the native store, and the
    packed host fields (uint8 [total, step_bytes] each) until they go to the device."""

    def _keep(self, lengths, packed, min_episode_steps: int, device) -> None:
        from acme_amd.native import NativeDemoStore
        if not lengths:
            raise ValueError("no demonstration episodes")
        self.lengths = np.asarray(lengths, np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        # Checks the lengths and the step bytes (ValueError for a short episode).
        self._native = NativeDemoStore(self.offsets, [p[0].shape[1] for p in packed],
                                       min_episode_steps)
        self._host = [np.concatenate(p) for p in packed]
        self._device = device

    @property
    def num_episodes(self) -> int:
        return len(self.lengths)

    def upload(self, device=None):
        """Puts the fields on the device (once) and returns the native store."""
        if self._host is not None:
            self._native.upload(self._host, device=device or self._device)
            self._host = None
        return self._native


def _step_bytes(x: np.ndarray, dtype, nbytes: int) -> np.ndarray:
    """[L, nbytes] uint8: the steps of x as `dtype`, C order."""
    x = np.ascontiguousarray(x, dtype=dtype)
    return np.frombuffer(x.tobytes(), np.uint8).reshape(x.shape[0], nbytes)


class DemonstrationStore(_Store):
    """Demonstration episodes held on the device for `mix_demonstrations`.

    episodes: an iterable of (observations [L, ...], actions [L, ...], rewards [L],
    discounts [L]) arrays, one tuple per episode, as DemonstrationRecorder.make_dataset()
    returns them.  As in the reference the first reward and discount and the last action of
    an episode are never used.  table_or_signature: the transition table the store will be
    mixed with, or its signature (NStepTransitionAdder.signature(spec)): observations and
    actions are converted to, and must have the shapes of, its fields 0 and 1.  Every episode
    needs at least 3 steps (the reference draws the first step from [0, L - 2)).

    The rows go to the device when the store is first mixed (or at `upload()`); nothing
    here needs a GPU before that."""

    def __init__(self, episodes: Iterable[Sequence[np.ndarray]], table_or_signature,
                 device=None):
        fields = _transition_fields(table_or_signature)
        fo, fa = fields[0], fields[1]
        self.obs_row_bytes, self.action_row_bytes = fo.row_bytes, fa.row_bytes
        packed = [[], [], [], []]  # observation rows, action rows, rewards, discounts
        lengths = []
        for i, ep in enumerate(episodes):
            if len(ep) != 4:
                raise ValueError(f"episode {i}: expected (observations, actions, rewards, "
                                 f"discounts), got {len(ep)} arrays")
            o, a = np.asarray(ep[0]), np.asarray(ep[1])
            r, d = np.asarray(ep[2], np.float32), np.asarray(ep[3], np.float32)
            L = int(r.shape[0]) if r.ndim == 1 else -1
            if L < 0 or d.shape != (L,) or o.shape[:1] != (L,) or a.shape[:1] != (L,):
                raise ValueError(f"episode {i}: the four arrays must share their length")
            if o.shape[1:] != fo.shape or a.shape[1:] != fa.shape:
                raise ValueError(
                    f"episode {i}: rows of {o.shape[1:]} observations and {a.shape[1:]} actions "
                    f"do not match the table's {fo.shape} ({fo.row_bytes} bytes) and {fa.shape} "
                    f"({fa.row_bytes} bytes)")
            for p, x in zip(packed, (self._rows(o, fo), self._rows(a, fa),
                                     _step_bytes(r, np.float32, 4),
                                     _step_bytes(d, np.float32, 4))):
                p.append(x)
            lengths.append(L)
        self._keep(lengths, packed, 3, device)

    @staticmethod
    def _rows(x: np.ndarray, f) -> np.ndarray:
        """[L, row_bytes] uint8 rows as the table stores them (C order, zero padding)."""
        rows = np.zeros((x.shape[0], f.row_bytes), np.uint8)
        rows[:, :f.nbytes] = _step_bytes(x, f.dtype, f.nbytes)
        return rows


class _MixIterator(_TableIterator):
    """_TableIterator whose every draw is followed, on the same stream and before the batch's
    ready event, by the demonstration overlay.  The table draws with the unpipelined
    acme_replay_sample_gather: the pipelined form copies a batch's rows in the next launch,
    which would overwrite the overlay."""

    def __init__(self, table, batch, timeout, prefetch, mix: "_Mixed"):
        super().__init__(table, batch, timeout, prefetch, shard=None)
        self._mix = mix
        self._launch = None     # the store's overlay launch (_Mixed._launcher)
        self._flags = {}        # keys buffer address -> the slot's is_demo flags
        self.last_is_demo = None  # uint8 [B] of the batch handed out last (if recorded)

    def _open_pipe(self) -> None:
        self._pipe = None
        self._pending = None

    def _f16_frames(self) -> bool:
        return False

    def _alloc(self):
        # Checks the table's layout against the store, uploads it, returns the launch.
        self._launch = self._mix._launcher(self._t)  # noqa: SLF001
        super()._alloc()
        if self._mix.record_is_demo:
            for raw, _, _, info, _ in self._slots:
                self._flags[raw[1]] = torch.zeros(self._rows, dtype=torch.uint8,
                                                  device=info["keys"].device)

    def _draw(self, L, h, raw, ptrs, st, stream=None, fb=None):
        from acme_amd._lib import check
        step = self._t.next_draw() & 0xFFFFFFFFFFFFFFFF
        check(L.acme_replay_sample_gather(h, self._B, step, *raw, ptrs, st), "replay sample")
        flags = self._flags.get(raw[1])
        self._launch(step, self._B, ptrs, raw, 0 if flags is None else flags.data_ptr(), st)
        return self._B

    def _sample_view(self, i: int, n: int):
        self.last_is_demo = self._flags.get(self._slots[i][0][1])
        return super()._sample_view(i, n)


def _mismatch(fields, store) -> str:
    return (f"the store holds {store.obs_row_bytes}-byte observation and "
            f"{store.action_row_bytes}-byte action rows, the table "
            f"{fields[0].row_bytes} and {fields[1].row_bytes}")


class _Mixed:
    """The surface of ReplayDataset (batch_size, element_spec, an iterator with
    holds_last_batches, last_inputs_event, last_frames_f16 = None), plus the iterator's
    `last_is_demo` flags.  A subclass supplies `_launcher`, the store's overlay launch."""

    def __init__(self, dataset: ReplayDataset, store, demonstration_ratio: float, seed: int,
                 record_is_demo: bool):
        self._dataset = dataset
        self.table = dataset.table
        self.store = store
        self.demonstration_ratio = float(demonstration_ratio)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.record_is_demo = bool(record_is_demo)
        self.batched = dataset.batched
        self.batch_size = dataset.batch_size
        self.prefetch = dataset.prefetch
        self.timeout = dataset.timeout

    @property
    def element_spec(self):
        return self._dataset.element_spec

    def __iter__(self):
        if _data_parallel() is not None and self._dataset.global_sampling is not False:
            raise ValueError("demonstrations cannot be mixed into global sampling over shards")
        it = _MixIterator(self.table, self.batch_size, self.timeout, self.prefetch, self)
        return it if self.batched else _Unbatched(it)


class MixedDataset(_Mixed):
    """What mix_demonstrations returns (the surface of _Mixed)."""

    def __init__(self, dataset: ReplayDataset, store: DemonstrationStore,
                 demonstration_ratio: float, n_step: int, discount: float, seed: int,
                 record_is_demo: bool):
        super().__init__(dataset, store, demonstration_ratio, seed, record_is_demo)
        self.n_step = int(n_step)
        self.discount = float(discount)

    def _launcher(self, table):
        """The iterator's hook: checks the table's layout (known by now) against the store,
        puts the store on the table's device and returns launch(step, batch, field pointers,
        raw info pointers, is_demo address, stream), issued behind every draw."""
        fields = _transition_fields(table)
        if (fields[0].row_bytes, fields[1].row_bytes) != (self.store.obs_row_bytes,
                                                          self.store.action_row_bytes):
            raise ValueError(_mismatch(fields, self.store))
        native = self.store.upload(table.native.device)

        def launch(step, batch, ptrs, raw, is_demo, st):
            native.mix_transitions(self.demonstration_ratio, self.n_step, self.discount,
                                   self.seed, step, batch, ptrs, raw[1], raw[2], raw[3], raw[4],
                                   is_demo, st)
        return launch


def _check_mix(name: str, kind: str, dataset, demonstration_ratio) -> float:
    """The refusals both mixes share; returns the ratio as a float."""
    if not isinstance(dataset, ReplayDataset):
        raise ValueError(f"{name} takes the dataset make_reverb_dataset returns")
    table = dataset.table
    if isinstance(table, (replay.FrameTable, replay.QueueTable)):
        raise ValueError(f"demonstrations are mixed into {kind} tables, not a "
                         f"{type(table).__name__}")
    if dataset.global_sampling:
        raise ValueError("demonstrations cannot be mixed into global sampling over shards")
    if os.environ.get("ACME_DATASET_F16", "0") == "1":
        raise ValueError("ACME_DATASET_F16=1 (the dataset's f16 frame copy) is not supported "
                         "with demonstrations: the copy would hold the replaced rows")
    ratio = float(demonstration_ratio)
    if not 0.0 <= ratio <= 1.0:  # also refuses NaN
        raise ValueError(f"demonstration_ratio {demonstration_ratio} is outside [0, 1]")
    return ratio


def mix_demonstrations(dataset: ReplayDataset, store: DemonstrationStore,
                       demonstration_ratio: float, n_step: int, discount: float,
                       seed: int = 0, record_is_demo: bool = True) -> MixedDataset:
    """`dataset` (make_reverb_dataset over a transition table) with each row of every batch
    replaced, with probability demonstration_ratio, by an n-step transition from `store`
    (module docstring).  n_step and discount are the adder's.  At ratio 0 the batches are
    those of `dataset`, bit for bit.  record_is_demo keeps a uint8 flag per row
    (iterator.last_is_demo)."""
    ratio = _check_mix("mix_demonstrations", "transition", dataset, demonstration_ratio)
    table = dataset.table
    if int(n_step) < 1:
        raise ValueError("n_step must be >= 1")
    if not isinstance(store, DemonstrationStore):
        raise ValueError("store must be a DemonstrationStore")
    if table.fields is not None:
        fields = _transition_fields(table)
        if (fields[0].row_bytes, fields[1].row_bytes) != (store.obs_row_bytes,
                                                          store.action_row_bytes):
            raise ValueError(_mismatch(fields, store))
    return MixedDataset(dataset, store, ratio, n_step, discount, seed, record_is_demo)


# ---------------------------------------------------------------- sequences (R2D3)
#
# The dataset side of R2D3 (acme/agents/tf/r2d3/agent.py:99-106): the reference maps each
# demonstration episode to one window of sequence_length steps (_sequence_from_episode,
# agent.py:163-235: a uniformly drawn step rounded down to a multiple of `period`, the steps
# from there zero-padded to the sequence length, start_of_episode = (first == 0) over the
# whole window, all-zero extras) and interleaves that dataset with the Reverb stream.  Here
# it is the same per-row overlay as above with a kernel of its own (acme_seq_demo_mix,
# csrc/demos.hip) that writes any number of per-step fields and spreads a row over as
# many workgroups as its bytes need.


def _sequence_layout(table_or_signature):
    """(per-step fields, K, T) of a sequence table, its signature, or another
    SequenceAdder.signature(...): the per-step _Field of every leaf of Step(observation,
    action, reward, discount, start_of_episode, extras), the number K of leaves in front of
    start_of_episode, and the table's sequence length (None when not yet known)."""
    x = table_or_signature
    _refuse_table(x, "sequence")
    T = None
    if isinstance(x, replay.Table):
        structure, fields, T = x._structure, x.fields, x.sequence_length  # noqa: SLF001
    else:
        structure, fields = x, None
    if not isinstance(structure, adders.Step):
        raise ValueError("demonstration sequences are mixed into sequence tables "
                         "(SequenceAdder.signature), not a table of "
                         f"{type(structure).__name__} items")
    if T == 0:
        raise ValueError("the table stores single steps, not sequences")
    if fields is None:
        fields = replay._layout_from_signature(structure)  # noqa: SLF001
    elif T:  # the stored layout is [T] + the per-step one
        fields = [replay._Field(f.shape[1:], f.dtype, f.nbytes // T, 0)  # noqa: SLF001
                  for f in fields]
    K = len(tree.flatten((structure.observation, structure.action, structure.reward,
                          structure.discount)))
    flag = fields[K]
    if flag.dtype != np.bool_ or flag.shape != ():
        raise ValueError("start_of_episode must be a bool scalar per step")
    return fields, K, T or None


def _same_steps(a, b) -> bool:
    return [(f.shape, f.dtype) for f in a] == [(f.shape, f.dtype) for f in b]


class SequenceDemonstrationStore(_Store):
    """Demonstration episodes held on the device for `mix_sequence_demonstrations`.

    episodes: an iterable of (observations, actions, rewards, discounts), one tuple per
    episode, as DemonstrationRecorder.make_dataset() returns them: every leaf is [L, ...] and
    observations may be a nest (an OAR).  table_or_signature: the sequence table the store
    will be mixed with, or its signature (SequenceAdder.signature(spec, extras)): the leaves
    are converted to the dtypes of, and must have the per-step shapes of, the leading fields
    of that layout (everything in front of start_of_episode).  A leaf whose dtype is of
    another kind than its field's (a float observation for a uint8 field) is refused.  An
    episode needs at least one step.

    The fields go to the device when the store is first mixed (or at `upload()`); nothing
    here needs a GPU before that."""

    def __init__(self, episodes: Iterable[Sequence], table_or_signature, device=None):
        from acme_amd.native import DEMO_MAX_FIELDS
        fields, K, _ = _sequence_layout(table_or_signature)
        if K > DEMO_MAX_FIELDS:
            raise ValueError(f"{K} per-step fields in front of start_of_episode; a store "
                             f"holds at most {DEMO_MAX_FIELDS}")
        self.step_fields = fields[:K]
        packed = [[] for _ in range(K)]
        lengths = []
        for i, ep in enumerate(episodes):
            if len(ep) != 4:
                raise ValueError(f"episode {i}: expected (observations, actions, rewards, "
                                 f"discounts), got {len(ep)} members")
            leaves = [np.asarray(x) for x in tree.flatten(tuple(ep))]
            if len(leaves) != K:
                raise ValueError(f"episode {i}: {len(leaves)} leaves, the table's steps have "
                                 f"{K} in front of start_of_episode")
            L = int(leaves[-1].shape[0]) if leaves[-1].ndim >= 1 else -1
            if L < 0 or any(x.shape[:1] != (L,) for x in leaves):
                raise ValueError(f"episode {i}: every member must have the episode's length "
                                 "as its first dimension")
            for k, (x, f) in enumerate(zip(leaves, self.step_fields)):
                if x.shape[1:] != f.shape:
                    raise ValueError(f"episode {i}, leaf {k}: steps of shape {x.shape[1:]} "
                                     f"do not match the table's {f.shape}")
                if not np.can_cast(x.dtype, f.dtype, casting="same_kind"):
                    raise ValueError(f"episode {i}, leaf {k}: {x.dtype} steps cannot be "
                                     f"stored in the table's {f.dtype} field")
                packed[k].append(_step_bytes(x, f.dtype, f.nbytes))
            lengths.append(L)
        self._keep(lengths, packed, 1, device)


class SequenceMixedDataset(_Mixed):
    """What mix_sequence_demonstrations returns (the surface of _Mixed)."""

    def __init__(self, dataset: ReplayDataset, store: SequenceDemonstrationStore,
                 demonstration_ratio: float, period: int, sequence_length: int, seed: int,
                 record_is_demo: bool):
        super().__init__(dataset, store, demonstration_ratio, seed, record_is_demo)
        self.period = int(period)
        self.sequence_length = int(sequence_length)

    def check_layout(self, table) -> None:
        """ValueError unless `table` (its layout known) stores this mix's sequences of the
        store's steps."""
        fields, K, T = _sequence_layout(table)
        if not _same_steps(fields[:K], self.store.step_fields):
            raise ValueError("the store's per-step fields "
                             f"{[(f.shape, str(f.dtype)) for f in self.store.step_fields]} are "
                             f"not the table's {[(f.shape, str(f.dtype)) for f in fields[:K]]}")
        if T is not None and T != self.sequence_length:
            raise ValueError(f"sequence_length {self.sequence_length} is not the table's {T}")

    def _launcher(self, table):
        from acme_amd.native import SEQ_DEMO_MAX_OUT_FIELDS
        self.check_layout(table)
        if table.sequence_length != self.sequence_length:
            raise ValueError(f"sequence_length {self.sequence_length} is not the table's "
                             f"{table.sequence_length}")
        if len(table.fields) > SEQ_DEMO_MAX_OUT_FIELDS:
            raise ValueError(f"the table's items have {len(table.fields)} fields; the mix "
                             f"writes at most {SEQ_DEMO_MAX_OUT_FIELDS}")
        row_bytes = np.asarray([f.row_bytes for f in table.fields], np.int64)
        logical = np.asarray([f.nbytes for f in table.fields], np.int64)
        native = self.store.upload(table.native.device)

        def launch(step, batch, ptrs, raw, is_demo, st):
            native.mix_sequences(self.demonstration_ratio, self.period, self.sequence_length,
                                 self.seed, step, batch, ptrs, row_bytes, logical, raw[1],
                                 raw[2], raw[3], raw[4], is_demo, st)
        return launch


def mix_sequence_demonstrations(dataset: ReplayDataset, store: SequenceDemonstrationStore,
                                demonstration_ratio: float, period: int, sequence_length: int,
                                seed: int = 0, record_is_demo: bool = True
                                ) -> SequenceMixedDataset:
    """`dataset` (make_reverb_dataset over a sequence table) with each row of every batch
    replaced, with probability demonstration_ratio, by a window of `sequence_length` steps of
    a demonstration episode from `store` (comment above).  period and sequence_length are the
    SequenceAdder's; sequence_length must be the table's (checked here when the table already
    stores sequences, else at the first draw).  At ratio 0 the batches are those of
    `dataset`, bit for bit.  record_is_demo keeps a uint8 flag per row
    (iterator.last_is_demo)."""
    ratio = _check_mix("mix_sequence_demonstrations", "sequence", dataset, demonstration_ratio)
    if int(period) < 1:
        raise ValueError("period must be >= 1")
    if int(sequence_length) < 1:
        raise ValueError("sequence_length must be >= 1")
    if not isinstance(store, SequenceDemonstrationStore):
        raise ValueError("store must be a SequenceDemonstrationStore")
    mixed = SequenceMixedDataset(dataset, store, ratio, period, sequence_length, seed,
                                 record_is_demo)
    if dataset.table.fields is not None:
        mixed.check_layout(dataset.table)
    return mixed
