"""Thin owners of the native objects behind the drop-in API.

`NativeReplay` wraps an acme_replay (GPU table); `NativeDQN` wraps an acme_dqn learner and
owns its flat device buffers (params / target / grads / Adam m, v) as torch tensors so
that torch.distributed (RCCL) can all-reduce the gradient buffer in place.
"""

from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from acme_amd import _lib
from acme_amd._lib import check, lib, ptr, stream_ptr

SAMPLER_UNIFORM = 0
SAMPLER_PRIORITIZED = 1


class NativeReplay:
    """Device-resident FIFO table with a 64-ary sum-tree sampler (see csrc/replay.hip)."""

    def __init__(self, capacity: int, field_bytes: Sequence[int], prioritized: bool,
                 priority_exponent: float = 0.6, seed: int = 1234, device=None):
        _lib.require_gpu()
        if len(field_bytes) > _lib.MAX_FIELDS:
            raise ValueError(f"at most {_lib.MAX_FIELDS} flattened fields per item")
        cfg = _lib.ReplayConfig()
        cfg.capacity = int(capacity)
        cfg.sampler = SAMPLER_PRIORITIZED if prioritized else SAMPLER_UNIFORM
        cfg.num_fields = len(field_bytes)
        cfg.priority_exponent = float(priority_exponent)
        cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        for i, b in enumerate(field_bytes):
            cfg.field_bytes[i] = int(b)
        self.field_bytes = [int(b) for b in field_bytes]
        self.capacity = int(capacity)
        self.prioritized = prioritized
        self.priority_exponent = float(priority_exponent)
        self.seed = cfg.seed
        self.device = torch.device(device or "cuda")
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().acme_replay_create(ctypes.byref(cfg), ctypes.byref(h)), "replay create")
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                lib().acme_replay_destroy(h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None

    @property
    def handle(self):
        return self._h

    def size(self) -> int:
        return int(lib().acme_replay_size(self._h))

    def nstep_writer(self, n_step: int, discount: float, obs_bytes: int, action_bytes: int,
                     rows_per_chunk: int = 64) -> "NativeNStepWriter":
        return NativeNStepWriter(self, n_step, discount, obs_bytes, action_bytes, rows_per_chunk)

    def insert(self, fields: Sequence, priorities: Optional[np.ndarray] = None,
               stream=None) -> np.ndarray:
        """fields: per-field arrays/tensors with leading dim n (host numpy or device tensors)."""
        n = int(fields[0].shape[0])
        keys = np.empty(n, np.uint64)
        on_dev = isinstance(fields[0], torch.Tensor) and fields[0].is_cuda
        keep = []
        ptrs = (ctypes.c_void_p * len(fields))()
        for i, f in enumerate(fields):
            if on_dev:
                t = f.contiguous()
                keep.append(t)
                ptrs[i] = t.data_ptr()
            else:
                a = np.ascontiguousarray(f)
                keep.append(a)
                ptrs[i] = a.ctypes.data
            nbytes = keep[-1].nbytes if not on_dev else keep[-1].numel() * keep[-1].element_size()
            if nbytes != n * self.field_bytes[i]:
                raise ValueError(f"field {i}: expected {n * self.field_bytes[i]} bytes, got {nbytes}")
        pr = None
        if priorities is not None:
            pr = np.ascontiguousarray(priorities, np.float64)
            if pr.shape != (n,):
                raise ValueError("priorities must have shape [n]")
        check(lib().acme_replay_insert(self._h, ptrs, n, None if pr is None else pr.ctypes.data,
                                       1 if on_dev else 0, keys.ctypes.data, stream_ptr(stream)),
              "replay insert")
        return keys

    def stage_capacity(self) -> int:
        """Items per pinned staging chunk (acme_replay_stage_capacity)."""
        n = int(lib().acme_replay_stage_capacity(self._h))
        if n <= 0:
            check(_lib.ACME_ERR_HIP, "replay staging")
        return n

    def stage(self, n: int) -> List[np.ndarray]:
        """Pinned host rows for n items: one writable uint8 [n, field_bytes[f]] array per
        field (valid until the matching commit)."""
        ptrs = (ctypes.c_void_p * len(self.field_bytes))()
        check(lib().acme_replay_stage(self._h, int(n), ptrs), "replay stage")
        return [np.ctypeslib.as_array((ctypes.c_uint8 * (n * b)).from_address(ptrs[i]))
                .reshape(n, b) for i, b in enumerate(self.field_bytes)]

    def commit(self, n: int, priorities: Optional[np.ndarray] = None, stream=None) -> np.ndarray:
        """Issues the first n staged items (side-stream H2D, no host wait); returns keys."""
        keys = np.empty(n, np.uint64)
        pr = None
        if priorities is not None:
            pr = np.ascontiguousarray(priorities, np.float64)
            if pr.shape != (n,):
                raise ValueError("priorities must have shape [n]")
        check(lib().acme_replay_commit(self._h, int(n), None if pr is None else pr.ctypes.data,
                                       keys.ctypes.data, stream_ptr(stream)), "replay commit")
        return keys

    def sync_inserts(self) -> None:
        check(lib().acme_replay_sync_inserts(self._h), "replay sync_inserts")

    def fill_synthetic(self, n: int, layout: int, num_actions: int = 18, seed: int = 0,
                       stream=None) -> None:
        check(lib().acme_replay_fill_synthetic(self._h, int(n), int(layout), int(num_actions),
                                               int(seed), stream_ptr(stream)), "fill_synthetic")

    def sample(self, batch: int, step: int, out: Optional[Dict[str, torch.Tensor]] = None,
               stream=None) -> Dict[str, torch.Tensor]:
        if out is None:
            out = self.alloc_sample_info(batch)
        check(lib().acme_replay_sample(self._h, int(batch), int(step) & 0xFFFFFFFFFFFFFFFF,
                                       ptr(out["slots"]), ptr(out["keys"]),
                                       ptr(out["probabilities"]), ptr(out["table_size"]),
                                       ptr(out["priorities"]), stream_ptr(stream)),
              "replay sample")
        return out

    def alloc_sample_info(self, batch: int) -> Dict[str, torch.Tensor]:
        d = self.device
        return dict(slots=torch.empty(batch, dtype=torch.int64, device=d),
                    keys=torch.empty(batch, dtype=torch.uint64, device=d),
                    probabilities=torch.empty(batch, dtype=torch.float64, device=d),
                    table_size=torch.empty(batch, dtype=torch.int64, device=d),
                    priorities=torch.empty(batch, dtype=torch.float64, device=d))

    def gather(self, slots: torch.Tensor, outs: Sequence[torch.Tensor], stream=None) -> None:
        ptrs = (ctypes.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        check(lib().acme_replay_gather(self._h, ptr(slots), int(slots.numel()), ptrs,
                                       stream_ptr(stream)), "replay gather")

    def update_priorities(self, keys: torch.Tensor, priorities: torch.Tensor, stream=None,
                          skip_word: Optional[int] = None) -> None:
        """skip_word: a learner's device skip word (NativeDQN.skip_word): the update is
        dropped when the step that produced the priorities was skipped."""
        keys = keys.to(self.device, torch.uint64).contiguous()
        priorities = priorities.to(self.device, torch.float64).contiguous()
        if skip_word:
            check(lib().acme_replay_update_priorities_gated(
                self._h, ptr(keys), ptr(priorities), int(keys.numel()), ctypes.c_void_p(skip_word),
                stream_ptr(stream)), "update_priorities")
            return
        check(lib().acme_replay_update_priorities(self._h, ptr(keys), ptr(priorities),
                                                  int(keys.numel()), stream_ptr(stream)),
              "update_priorities")

    def export_state(self) -> Dict[str, np.ndarray]:
        """Host copy of the live table (checkpoints): field rows, keys and raw priorities of
        slots [0, size), the insert counter.  Leaves and tree levels are derived data."""
        L = lib()
        n = self.size()
        torch.cuda.synchronize(self.device)
        out = {"inserted": np.int64(L.acme_replay_inserted(self._h))}
        for f, b in enumerate(self.field_bytes):
            p = ctypes.c_void_p()
            check(L.acme_replay_storage(self._h, f, ctypes.byref(p)))
            out[f"field_{f}"] = _device_array(p.value, n * b, np.uint8, self.device).cpu() \
                .numpy().reshape(n, b).copy()
        lv, rp, ks = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        check(L.acme_replay_debug_leaves(self._h, ctypes.byref(lv), ctypes.byref(rp),
                                         ctypes.byref(ks)))
        out["raw_priorities"] = _device_array(rp.value, n, np.float64, self.device).cpu() \
            .numpy().view(np.float64).copy()
        out["keys"] = _device_array(ks.value, n, np.uint64, self.device).cpu().numpy() \
            .view(np.uint64).copy()
        return out

    def import_state(self, state: Dict[str, np.ndarray]) -> None:
        """Inverse of export_state (same capacity and field layout): writes rows, keys and
        raw priorities, then rebuilds leaves and levels on the device."""
        L = lib()
        keys = np.asarray(state["keys"], np.uint64)
        n = len(keys)
        if n > self.capacity:
            raise ValueError(f"state holds {n} items, table capacity is {self.capacity}")
        torch.cuda.synchronize(self.device)
        for f, b in enumerate(self.field_bytes):
            rows = np.ascontiguousarray(state[f"field_{f}"], np.uint8)
            if rows.shape != (n, b):
                raise ValueError(f"field {f}: state rows {rows.shape}, table expects {(n, b)}")
            p = ctypes.c_void_p()
            check(L.acme_replay_storage(self._h, f, ctypes.byref(p)))
            _memcpy_htod(p.value, rows)
        lv, rp, ks = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        check(L.acme_replay_debug_leaves(self._h, ctypes.byref(lv), ctypes.byref(rp),
                                         ctypes.byref(ks)))
        _memcpy_htod(rp.value, np.asarray(state["raw_priorities"], np.float64))
        _memcpy_htod(ks.value, keys)
        check(L.acme_replay_restore(self._h, int(state["inserted"]), None), "replay restore")
        torch.cuda.synchronize(self.device)

    def debug_state(self) -> Dict[str, np.ndarray]:
        """Host copies of leaf weights / raw priorities / keys (tests)."""
        lv, rp, ks = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        check(lib().acme_replay_debug_leaves(self._h, ctypes.byref(lv), ctypes.byref(rp),
                                             ctypes.byref(ks)))
        torch.cuda.synchronize(self.device)
        n = self.capacity
        out = {}
        for name, p, dt, cnt in (("leaves", lv, np.float64, n), ("raw", rp, np.float64, n),
                                 ("keys", ks, np.uint64, n)):
            out[name] = _device_array(p.value, cnt, dt, self.device).cpu().numpy().view(dt).copy()
        return out

    def debug_levels(self) -> list:
        """Host copies of every stored sum-tree level, leaves first (tests)."""
        n = ctypes.c_int32()
        p, cnt = ctypes.c_void_p(), ctypes.c_int64()
        check(lib().acme_replay_debug_level(self._h, 0, ctypes.byref(p), ctypes.byref(cnt),
                                            ctypes.byref(n)))
        torch.cuda.synchronize(self.device)
        out = []
        for l in range(n.value):
            check(lib().acme_replay_debug_level(self._h, l, ctypes.byref(p), ctypes.byref(cnt),
                                                None))
            out.append(_device_array(p.value, cnt.value, np.float64, self.device)
                       .cpu().numpy().view(np.float64).copy())
        return out



class NativeNStepWriter:
    """acme_nstep_writer: the native side of NStepTransitionAdder (rows formed and packed in
    C, straight into pinned chunks).  `add_raw(act_ptr, reward, discount, obs_ptr, last,
    priority)` is the per-step entry, with the pointers of host arrays the caller keeps alive
    for the call."""

    def __init__(self, table: NativeReplay, n_step: int, discount: float, obs_bytes: int,
                 action_bytes: int, rows_per_chunk: int = 64):
        h = ctypes.c_void_p()
        L = lib()
        check(L.acme_nstep_writer_create(table.handle, int(n_step), float(discount),
                                         int(obs_bytes), int(action_bytes), int(rows_per_chunk),
                                         ctypes.byref(h)), "n-step writer create")
        self._table = table  # the writer commits into it: keep it alive
        self._h = h
        self._add = L.acme_nstep_writer_add
        self._pending = L.acme_nstep_writer_pending

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                lib().acme_nstep_writer_destroy(h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None

    def start(self, obs_ptr: int) -> None:
        check(lib().acme_nstep_writer_start(self._h, obs_ptr), "n-step writer start")

    def add_raw(self, act_ptr: int, reward: float, discount: float, obs_ptr: int, last: bool,
                priority: float = 1.0) -> None:
        rc = self._add(self._h, act_ptr, reward, discount, obs_ptr, 1 if last else 0, priority)
        if rc:
            check(rc, "n-step writer add")

    def flush(self) -> None:
        check(lib().acme_nstep_writer_flush(self._h), "n-step writer flush")

    def reset(self) -> None:
        check(lib().acme_nstep_writer_reset(self._h), "n-step writer reset")

    def pending(self) -> int:
        return int(self._pending(self._h))


DEMO_MAX_FIELDS = 16           # ACME_DEMO_MAX_FIELDS
SEQ_DEMO_MAX_OUT_FIELDS = 32   # ACME_SEQ_DEMO_MAX_OUT_FIELDS


class NativeDemoStore:
    """acme_demo_store: demonstration episodes as K immutable per-step device arrays
    (csrc/demos.hip).  The constructor checks the layout on the host (an episode shorter than
    min_episode_steps is a ValueError, no GPU needed); `upload()` puts the packed fields on
    the device, once; `mix_transitions()` (acme_demo_mix) and `mix_sequences()`
    (acme_seq_demo_mix) overlay the demonstration rows of a drawn batch."""

    def __init__(self, offsets: np.ndarray, step_bytes: Sequence[int],
                 min_episode_steps: int = 1):
        self.offsets = np.ascontiguousarray(offsets, np.int64)
        self.step_bytes = np.ascontiguousarray(step_bytes, np.int64)
        self.device = None
        h = ctypes.c_void_p()
        check(lib().acme_demo_store_create(len(self.offsets) - 1, self.offsets.ctypes.data,
                                           len(self.step_bytes), self.step_bytes.ctypes.data,
                                           int(min_episode_steps), ctypes.byref(h)),
              "demonstration store")
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                lib().acme_demo_store_destroy(h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None

    @property
    def handle(self):
        return self._h

    def upload(self, fields: Sequence[np.ndarray], device=None) -> None:
        """Packed host fields: uint8 [total, step_bytes[f]] each."""
        _lib.require_gpu()
        total = int(self.offsets[-1])
        arrays = [np.ascontiguousarray(a, np.uint8) for a in fields]
        if len(arrays) != len(self.step_bytes):
            raise ValueError(f"{len(arrays)} demonstration fields, expected "
                             f"{len(self.step_bytes)}")
        for a, sb in zip(arrays, self.step_bytes):
            if a.nbytes != total * int(sb):
                raise ValueError(f"demonstration field has {a.nbytes} bytes, expected "
                                 f"{total * int(sb)}")
        self.device = torch.device(device or "cuda")
        ptrs = (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
        with torch.cuda.device(self.device):
            check(lib().acme_demo_store_upload(self._h, ptrs), "demonstration store upload")

    def mix_transitions(self, ratio: float, n_step: int, discount: float, seed: int, step: int,
                        batch: int, out_fields, keys: int, probabilities: int,
                        table_size: int, priorities: int, is_demo: int = 0,
                        stream: Optional[int] = None) -> None:
        """out_fields: a ctypes array of the five transition fields' device pointers; the
        other outputs raw device addresses (0: not written); stream: a raw hipStream_t.  The
        store's fields are observation rows, action rows, f32 rewards, f32 discounts."""
        check(lib().acme_demo_mix(self._h, float(ratio), int(n_step), float(discount),
                                  int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF,
                                  int(batch), out_fields, keys or None, probabilities or None,
                                  table_size or None, priorities or None, is_demo or None,
                                  stream_ptr() if stream is None else stream),
              "demonstration mix")

    def mix_sequences(self, ratio: float, period: int, sequence_length: int, seed: int,
                      step: int, batch: int, out_fields, row_bytes: np.ndarray,
                      logical_bytes: np.ndarray, keys: int, probabilities: int,
                      table_size: int, priorities: int, is_demo: int = 0,
                      stream: Optional[int] = None) -> None:
        """out_fields: a ctypes array of every batch field's device pointer; row_bytes /
        logical_bytes: int64 arrays of the same length; the other outputs raw device
        addresses (0: not written); stream: a raw hipStream_t."""
        check(lib().acme_seq_demo_mix(self._h, float(ratio), int(period), int(sequence_length),
                                      int(seed) & 0xFFFFFFFFFFFFFFFF,
                                      int(step) & 0xFFFFFFFFFFFFFFFF, int(batch), out_fields,
                                      len(out_fields), row_bytes.ctypes.data,
                                      logical_bytes.ctypes.data, keys or None,
                                      probabilities or None, table_size or None,
                                      priorities or None, is_demo or None,
                                      stream_ptr() if stream is None else stream),
              "sequence demonstration mix")


def _device_array(address: int, count: int, dtype, device) -> torch.Tensor:
    """Copies `count` elements at a raw device address into a new tensor (test helper)."""
    nbytes = count * np.dtype(dtype).itemsize
    dst = torch.empty(nbytes, dtype=torch.uint8, device=device)
    torch.cuda.synchronize(device)
    _memcpy_dtod(dst.data_ptr(), address, nbytes)
    return dst


_hip = None


def _hip_memcpy(dst: int, src: int, nbytes: int, kind: int) -> None:
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so.7")
        _hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        _hip.hipMemcpy.restype = ctypes.c_int
    rc = _hip.hipMemcpy(ctypes.c_void_p(dst), ctypes.c_void_p(src), ctypes.c_size_t(nbytes), kind)
    if rc != 0:
        raise RuntimeError(f"hipMemcpy failed ({rc})")


def _memcpy_dtod(dst: int, src: int, nbytes: int) -> None:
    _hip_memcpy(dst, src, nbytes, 3)


def _memcpy_htod(dst: int, host: np.ndarray) -> None:
    """Synchronous host -> device copy of a numpy array to a raw device address."""
    a = np.ascontiguousarray(host)
    if a.nbytes:
        _hip_memcpy(dst, a.ctypes.data, a.nbytes, 1)


def _read_tensor_table(num_fn, info_fn, handle) -> List[Tuple[str, int, Tuple[int, ...]]]:
    """(name, offset, shape) of every tensor of a learner's flat buffer, in buffer order."""
    tensors = []
    for i in range(num_fn(handle)):
        off, numel, nd = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        shape = (ctypes.c_int64 * 4)()
        name = ctypes.c_char_p()
        check(info_fn(handle, i, ctypes.byref(off), ctypes.byref(numel), ctypes.byref(nd), shape,
                      ctypes.byref(name)))
        tensors.append((name.value.decode(), int(off.value),
                        tuple(int(shape[k]) for k in range(nd.value))))
    return tensors


def _debug_buffer(fn, handle, name: str, device) -> np.ndarray:
    """A host copy of the learner workspace buffer `name` (float32 words)."""
    p, n = ctypes.c_void_p(), ctypes.c_int64()
    check(fn(handle, name.encode(), ctypes.byref(p), ctypes.byref(n)))
    return _device_array(p.value, n.value, np.float32, device).cpu().numpy().view(
        np.float32).copy()


NET_NATURE = 0
NET_MLP = 1
OBS_U8 = 0
OBS_F32 = 1


class _NativeLearner:
    """A native learner handle and its flat buffers, shared by every Native* learner class:
    creation and lifetime, the tensor table, the flat params / (target) / grads / Adam m / v
    buffers and their bind, the step count and debug buffers.  Subclasses name the C ABI
    prefix (_prefix, e.g. "acme_dqn") and the error-message tag (_tag)."""

    _prefix = ""
    _tag = ""
    _has_target = True  # a target network's buffer is bound after params

    def _fn(self, name: str):
        return getattr(lib(), f"{self._prefix}_{name}")

    def _create(self, cfg, device, shared_params: Optional[torch.Tensor] = None) -> None:
        """Creates the handle from cfg, allocates the flat buffers (params = shared_params
        when given) and binds them."""
        self.cfg = cfg
        self.device = torch.device(device or "cuda")
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(self._fn("create")(ctypes.byref(cfg), ctypes.byref(h)), f"{self._tag} create")
        self._h = h
        self.flat_size = int(self._fn("flat_size")(h))
        self.tensors = _read_tensor_table(self._fn("num_tensors"), self._fn("tensor_info"), h)
        z = lambda: torch.zeros(self.flat_size, dtype=torch.float32, device=self.device)  # noqa
        if shared_params is not None:
            if shared_params.numel() != self.flat_size or not shared_params.is_cuda:
                raise ValueError("shared_params must be a device buffer of the same layout")
            self.params = shared_params
        else:
            self.params = z()
        bound = [self.params]
        if self._has_target:
            self.target = z()
            bound.append(self.target)
        self.grads, self.m, self.v = z(), z(), z()
        bound += [self.grads, self.m, self.v]
        check(self._fn("bind")(h, *[ptr(b) for b in bound]), f"{self._tag} bind")

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self._fn("destroy")(h)
            except Exception:
                pass
            self._h = None

    # --------------------------------------------------------------- parameters
    def views(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        out = {}
        for name, off, shape in self.tensors:
            n = int(np.prod(shape))
            out[name] = flat[off:off + n].view(shape)
        return out

    def _copy_in(self, flat: torch.Tensor, src: Dict[str, np.ndarray]) -> None:
        for name, t in self.views(flat).items():
            t.copy_(torch.as_tensor(np.asarray(src[name], np.float32)).view(t.shape))

    def set_params(self, params: Dict[str, np.ndarray], target: Optional[Dict] = None) -> None:
        self._copy_in(self.params, params)
        if self._has_target:
            self._copy_in(self.target, target if target is not None else params)
        self.params_changed()

    def get_params(self, which: str = "params") -> Dict[str, np.ndarray]:
        flat = getattr(self, which)
        return {k: v.detach().cpu().numpy().copy() for k, v in self.views(flat).items()}

    @property
    def num_steps(self) -> int:
        return int(self._fn("num_steps")(self._h))

    @num_steps.setter
    def num_steps(self, n: int) -> None:
        check(self._fn("set_num_steps")(self._h, int(n)))

    def debug_buffer(self, name: str) -> np.ndarray:
        return _debug_buffer(self._fn("debug_buffer"), self._h, name, self.device)

    def params_changed(self) -> None:
        """The params / target buffers were written from outside (nothing to do for a learner
        whose step reads the f32 buffers directly)."""

    def _sequence_batch(self, observation, prev_action, prev_reward, action, reward, discount,
                        h0, c0, behaviour_logits=None, core_state=True):
        """Validates a recurrent learner's batch-major [B, T, ...] device tensors and the core
        state at t = 0 (h0 / c0 [B, H] views with unit inner stride, unless not core_state);
        returns the filled _lib.SequenceBatch."""
        B, T = int(action.shape[0]), int(action.shape[1])
        want = torch.uint8 if self.torso == "atari" else torch.float32
        checks = [("observation", observation, want), ("prev_action", prev_action, torch.int32),
                  ("prev_reward", prev_reward, torch.float32), ("action", action, torch.int32),
                  ("reward", reward, torch.float32), ("discount", discount, torch.float32)]
        if behaviour_logits is not None:
            checks.append(("behaviour_logits", behaviour_logits, torch.float32))
        for name, t, dt in checks:
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous()
                    and t.dtype == dt):
                raise ValueError(f"{name} must be a contiguous {dt} device tensor")
            if tuple(t.shape[:2]) != (B, T):
                raise ValueError(f"{name} has shape {tuple(t.shape)}, expected [{B}, {T}, ...]")
        b = _lib.SequenceBatch()
        b.observation, b.prev_action, b.prev_reward = ptr(observation), ptr(prev_action), ptr(prev_reward)
        b.action, b.reward, b.discount = ptr(action), ptr(reward), ptr(discount)
        b.behaviour_logits = ptr(behaviour_logits) if behaviour_logits is not None else None
        if core_state:
            for name, t in (("h0", h0), ("c0", c0)):
                if (t is None or t.dtype != torch.float32 or t.shape != (B, self.lstm_size)
                        or t.stride(1) != 1):
                    raise ValueError(f"{name} must be float32 [{B}, {self.lstm_size}] with unit "
                                     "inner stride")
            if h0.stride(0) != c0.stride(0):
                raise ValueError("h0 and c0 must share a row stride")
            b.h0, b.c0, b.state_stride = ptr(h0), ptr(c0), int(h0.stride(0))
        else:
            b.h0 = b.c0 = None
            b.state_stride = self.lstm_size
        b.batch, b.sequence_length = B, T
        return b

    def _acting_outputs(self, rows: int, second_dtype) -> List[torch.Tensor]:
        """The outputs of a recurrent learner's network step for `rows` actors: [rows, A],
        [rows] of second_dtype (values or actions) and the core state [rows, H] twice."""
        A, H, dev = self.num_actions, self.lstm_size, self.device
        return [torch.empty(rows, A, dtype=torch.float32, device=dev),
                torch.empty(rows, dtype=second_dtype, device=dev),
                torch.empty(rows, H, dtype=torch.float32, device=dev),
                torch.empty(rows, H, dtype=torch.float32, device=dev)]


class _PlaneState:
    """Plane-scale and step-guard state of the learners on the f16 plane engine (NativeDQN,
    NativeIMPALA, NativeR2D2), beside _NativeLearner."""

    # The words <prefix>_guard_state writes, in order.
    _guard_fields = ("applied", "skipped", "last_skipped")

    def params_changed(self) -> None:
        """Tells the learner its params / target buffers were written from outside (its
        derived f16 parameter planes are rebuilt and the plane scales recalibrate before the
        next use)."""
        check(self._fn("params_changed")(self._h), f"{self._tag} params_changed")

    def scale_state(self) -> np.ndarray:
        """The plane scales (learner state for checkpoints; empty without the plane path)."""
        n = ctypes.c_int32(0)
        fn, what = self._fn("scale_state"), f"{self._tag} scale_state"
        check(fn(self._h, None, 0, ctypes.byref(n)), what)
        out = np.zeros(n.value, np.float32)
        if n.value:
            check(fn(self._h, out.ctypes.data, n.value, ctypes.byref(n)), what)
        return out

    def set_scale_state(self, state) -> None:
        """Restores scale_state() (after params_changed): resumed steps are bit-identical."""
        a = np.ascontiguousarray(np.asarray(state, np.float32))
        if a.size:
            check(self._fn("set_scale_state")(self._h, a.ctypes.data, a.size),
                  f"{self._tag} set_scale_state")

    @property
    def skipped_steps(self) -> int:
        """Steps skipped (plane overflow or LSTM timeout) so far among those the device has
        finished (no synchronisation)."""
        return int(self._fn("skipped_steps")(self._h))

    def guard_state(self) -> Dict[str, int]:
        """The step guard's counters under the names in _guard_fields (synchronises the
        device)."""
        a = (ctypes.c_int64 * len(self._guard_fields))()
        check(self._fn("guard_state")(self._h, a), f"{self._tag} guard_state")
        return dict(zip(self._guard_fields, (int(x) for x in a)))

    @property
    def applied_steps(self) -> int:
        """Updates applied (Adam's t after the last step); synchronises."""
        return self.guard_state()["applied"]

    @applied_steps.setter
    def applied_steps(self, n: int) -> None:
        check(self._fn("set_applied_steps")(self._h, int(n)), f"{self._tag} set_applied_steps")

    @property
    def skip_word(self) -> Optional[int]:
        """Device address of the word an after-step priority update is gated on (set while
        the last step was skipped), or None: no plane path, or a learner that writes no
        priorities (IMPALA has no such export)."""
        return None


class _PlaneOverflow:
    """plane_overflow of the learners that export it (NativeDQN, NativeIMPALA)."""

    def plane_overflow(self, reset: bool = False) -> bool:
        """True if a plane tensor exceeded f16's range at its scale since the last reset
        (synchronises the device)."""
        v = ctypes.c_int32(0)
        check(self._fn("plane_overflow")(self._h, ctypes.byref(v), int(reset)),
              f"{self._tag} plane_overflow")
        return bool(v.value)


class NativeDQN(_PlaneOverflow, _PlaneState, _NativeLearner):
    """acme_dqn learner + its flat buffers."""

    _prefix, _tag = "acme_dqn", "dqn"
    _guard_fields = _PlaneState._guard_fields + ("q_values_overflowed",)

    def __init__(self, *, network: str, num_actions: int, max_batch: int, obs_dtype: str,
                 obs_dim: int = 0, hidden: Sequence[int] = (), discount: float = 0.99,
                 importance_sampling_exponent: float = 0.2, learning_rate: float = 1e-3,
                 huber_loss_parameter: float = 1.0, target_update_period: int = 100,
                 max_abs_reward: float = 1.0, adam_beta1: float = 0.9, adam_beta2: float = 0.999,
                 adam_epsilon: float = 1e-8, semantics: str = "tf", device=None):
        """semantics: "tf" restates acme/agents/tf/dqn/learning.py, "jax" the JAX learner
        (acme/agents/jax/dqn/learning.py: f32 IS weights, steps+1 target cadence, optix.adam)."""
        _lib.require_gpu()
        if semantics not in ("tf", "jax"):
            raise ValueError(f"semantics must be 'tf' or 'jax', got {semantics!r}")
        if huber_loss_parameter < 0:
            raise ValueError("quadratic_linear_boundary must be >= 0.")
        cfg = _lib.DQNConfig()
        cfg.network = NET_NATURE if network == "nature" else NET_MLP
        cfg.obs_dtype = OBS_U8 if obs_dtype == "uint8" else OBS_F32
        cfg.num_actions = int(num_actions)
        cfg.max_batch = int(max_batch)
        cfg.obs_dim = int(obs_dim)
        if len(hidden) > _lib.MAX_MLP_LAYERS:
            raise ValueError(f"at most {_lib.MAX_MLP_LAYERS} hidden layers")
        cfg.num_hidden = len(hidden)
        for i, h in enumerate(hidden):
            cfg.hidden[i] = int(h)
        cfg.discount = discount
        cfg.importance_sampling_exponent = importance_sampling_exponent
        cfg.learning_rate = learning_rate
        cfg.huber_loss_parameter = huber_loss_parameter
        cfg.adam_beta1, cfg.adam_beta2, cfg.adam_epsilon = adam_beta1, adam_beta2, adam_epsilon
        cfg.target_update_period = int(target_update_period)
        cfg.max_abs_reward = max_abs_reward
        cfg.semantics = _lib.SEMANTICS_JAX if semantics == "jax" else _lib.SEMANTICS_TF
        self.semantics = semantics
        self.network = network
        self.num_actions = int(num_actions)
        self.max_batch = int(max_batch)
        self._create(cfg, device)
        self.num_params = int(lib().acme_dqn_num_params(self._h))
        d = self.device
        self.loss = torch.zeros(1, dtype=torch.float32, device=d)
        self.td_error = torch.zeros(max_batch, dtype=torch.float32, device=d)
        self.priorities = torch.zeros(max_batch, dtype=torch.float64, device=d)

    # ---- step guard (acme_dqn_guard_state: the skip-on-overflow rule of the plane path)
    def guard_state(self) -> Dict[str, int]:
        """{applied, skipped, last_skipped, q_values_overflowed, verdict_timeouts} (synchronises
        the device)."""
        g = super().guard_state()
        t = ctypes.c_int64()
        check(lib().acme_dqn_verdict_timeouts(self._h, ctypes.byref(t)), "dqn verdict_timeouts")
        g["verdict_timeouts"] = int(t.value)
        return g

    def update_rider_launches(self) -> int:
        """Steps whose priority write-back rode conv1's weight-gradient launch."""
        return int(lib().acme_dqn_update_rider_launches(self._h))

    def fused_x2_launches(self) -> int:
        """Forwards of the step that ran conv3 inside conv2's launch (x2 kept in LDS)."""
        return int(lib().acme_dqn_fused_x2_launches(self._h))

    @property
    def skip_word(self) -> Optional[int]:
        p = ctypes.c_void_p()
        check(lib().acme_dqn_skip_word(self._h, ctypes.byref(p)), "dqn skip_word")
        return p.value

    # ---- re-issue of skipped steps (acme_dqn_set_reissue / _verdicts_issued / _step_verdict)
    def set_reissue(self, enable: bool) -> None:
        """A skipped step holds every later step skipped until the next calibration, so the
        caller can re-issue the held batches in order (DQNLearner)."""
        check(lib().acme_dqn_set_reissue(self._h, 1 if enable else 0), "dqn set_reissue")

    @property
    def verdicts_issued(self) -> int:
        """Step verdicts issued so far (the next step's verdict has this sequence number)."""
        return int(lib().acme_dqn_verdicts_issued(self._h))

    def step_verdict(self, seq: int) -> Optional[bool]:
        """None while verdict `seq` is undecided, else whether that step was skipped (no
        synchronisation: a pinned ring the device writes)."""
        v = ctypes.c_int32(-1)
        check(lib().acme_dqn_step_verdict(self._h, int(seq), ctypes.byref(v)), "dqn step_verdict")
        return None if v.value < 0 else bool(v.value)

    def set_data_parallel_gate(self, enable: bool) -> None:
        check(lib().acme_dqn_set_data_parallel_gate(self._h, 1 if enable else 0), "dqn dp gate")

    # --------------------------------------------------------------- step
    def _batch(self, o_tm1, a_tm1, r_t, d_t, o_t, probabilities, global_min_probability=None,
               mean_over=None, obs_f16=None):
        B = int(a_tm1.shape[0])
        if B < 1 or B > self.max_batch:
            raise ValueError(f"batch of {B} rows: the learner takes 1..{self.max_batch}")
        for name, t in (("o_tm1", o_tm1), ("a_tm1", a_tm1), ("r_t", r_t), ("d_t", d_t),
                        ("o_t", o_t), ("probabilities", probabilities)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous device tensor")
            if t.shape[0] != B:
                raise ValueError(f"{name} has leading dim {t.shape[0]}, expected {B}")
        if a_tm1.dtype != torch.int32 or r_t.dtype != torch.float32 or d_t.dtype != torch.float32:
            raise ValueError("a_tm1 must be int32, r_t and d_t float32")
        if probabilities.dtype != torch.float64:
            raise ValueError("probabilities must be float64")
        want = torch.uint8 if self.cfg.obs_dtype == OBS_U8 else torch.float32
        if o_tm1.dtype != want or o_t.dtype != want:
            raise ValueError(f"observations must be {want}")
        tb = _lib.TransitionBatch()
        tb.o_tm1, tb.a_tm1, tb.r_t, tb.d_t, tb.o_t = (ptr(o_tm1), ptr(a_tm1), ptr(r_t), ptr(d_t),
                                                      ptr(o_t))
        tb.probabilities = ptr(probabilities)
        tb.batch = B
        tb.global_min_probability = ptr(global_min_probability)
        tb.mean_over = int(mean_over or 0)
        if obs_f16 is not None:  # [2B, obs] f16 bits of [o_tm1; o_t] (the dataset's copy)
            if not (isinstance(obs_f16, torch.Tensor) and obs_f16.is_cuda and
                    obs_f16.dtype in (torch.int16, torch.uint16, torch.float16) and
                    obs_f16.is_contiguous() and obs_f16.shape[0] >= 2 * B and
                    obs_f16[0].numel() == o_tm1[0].numel()):
                raise ValueError("obs_f16 must be a contiguous [2B, obs] 16-bit device tensor")
            tb.obs_f16 = ptr(obs_f16)
        return tb

    @staticmethod
    def _event_handle(ev) -> Optional[int]:
        if ev is None:
            return None
        return ev.handle if hasattr(ev, "handle") else int(ev.cuda_event)

    def _outputs(self, q_tm1=None):
        o = _lib.DQNOutputs()
        o.loss, o.td_error, o.priorities = ptr(self.loss), ptr(self.td_error), ptr(self.priorities)
        o.q_tm1 = ptr(q_tm1)
        return o

    def forward_backward(self, *batch, global_min_probability=None, q_tm1=None, stream=None):
        tb = self._batch(*batch, global_min_probability=global_min_probability)
        out = self._outputs(q_tm1)
        check(lib().acme_dqn_forward_backward(self._h, ctypes.byref(tb), ctypes.byref(out),
                                              stream_ptr(stream)), "dqn forward_backward")

    def forward_backward_stage(self, stage: int, *batch, global_min_probability=None,
                               q_tm1=None, stream=None, mean_over=None, obs_f16=None,
                               inputs_event=None):
        """Stage 0: forwards, loss, head/dense backward (grads[grad_split:]); stage 1: torso
        backward (grads[:grad_split]).  Stage 0 may be issued as stage 2 (forwards) then
        stage 3 (loss and dense backward; global_min_probability is read from here on) or
        stage 4 (stage 3 without ordering the stream after the dense gradients: see
        dense_grads_ready).  mean_over: the batch mean's denominator (default the batch; a
        data-parallel share passes the nominal per-rank batch).  inputs_event: as for
        step()."""
        tb = self._batch(*batch, global_min_probability=global_min_probability,
                         mean_over=mean_over, obs_f16=obs_f16)
        tb.inputs_event = self._event_handle(inputs_event)
        out = self._outputs(q_tm1)
        check(lib().acme_dqn_forward_backward_stage(self._h, ctypes.byref(tb), ctypes.byref(out),
                                                    int(stage), stream_ptr(stream)),
              f"dqn forward_backward stage {stage}")

    def dense_grads_ready(self, stream=None) -> None:
        """Orders `stream` (default: the current one) after the dense gradients
        grads[grad_split:] of the last stage 3 / 4."""
        check(lib().acme_dqn_dense_grads_ready(self._h, stream_ptr(stream)), "dense grads ready")

    def dp_init(self, comm, world_size: int) -> None:
        """Binds a caller-owned RCCL communicator (ncclComm_t) for dp_step."""
        check(lib().acme_dqn_dp_init(self._h, ctypes.c_void_p(comm), int(world_size)), "dp init")

    def dp_step(self, *batch, mean_over=None, q_tm1=None, stream=None, obs_f16=None):
        """One data-parallel step over the bound communicator (acme_dqn_dp_step)."""
        tb = self._batch(*batch, mean_over=mean_over, obs_f16=obs_f16)
        out = self._outputs(q_tm1)
        check(lib().acme_dqn_dp_step(self._h, ctypes.byref(tb), ctypes.byref(out),
                                     stream_ptr(stream)), "dqn dp step")

    @property
    def grad_split(self) -> int:
        s = ctypes.c_int64()
        check(lib().acme_dqn_grad_split(self._h, ctypes.byref(s)))
        return int(s.value)

    def batch_min_probability(self, probabilities: torch.Tensor, out: torch.Tensor, stream=None):
        """out[0] = min(probabilities) on the device (data-parallel IS normaliser)."""
        check(lib().acme_min_f64(ptr(probabilities), int(probabilities.numel()), ptr(out),
                                 stream_ptr(stream)), "min_f64")

    def apply(self, stream=None):
        check(lib().acme_dqn_apply(self._h, stream_ptr(stream)), "dqn apply")

    def step(self, *batch, q_tm1=None, stream=None, obs_f16=None, priority_update=None,
             inputs_event=None):
        """One SGD step.  priority_update = (native replay handle, uint64 keys tensor[, raw
        hipEvent_t of the table's last device read or None]): the batch's priorities are
        written back to that table as part of the step (acme_dqn_step_update: beside the
        backward on the plane path, after that read).  inputs_event: an event at which the
        batch's inputs are complete (acme_transition_batch.inputs_event)."""
        tb = self._batch(*batch, obs_f16=obs_f16)
        tb.inputs_event = self._event_handle(inputs_event)
        out = self._outputs(q_tm1)
        if priority_update is None:
            check(lib().acme_dqn_step(self._h, ctypes.byref(tb), ctypes.byref(out),
                                      stream_ptr(stream)), "dqn step")
            return
        handle, keys, after = (tuple(priority_update) + (None,))[:3]
        if keys.dtype not in (torch.uint64, torch.int64) or not keys.is_contiguous():
            raise ValueError("priority_update keys must be a contiguous 64-bit tensor")
        if keys.numel() != int(tb.batch) or not keys.is_cuda:
            raise ValueError("priority_update keys must hold one key per batch row, on the "
                             "learner's device")
        check(lib().acme_dqn_step_update(self._h, ctypes.byref(tb), ctypes.byref(out), handle,
                                         ptr(keys), after, stream_ptr(stream)), "dqn step")

    def q_values(self, obs: torch.Tensor, use_target: bool = False, stream=None) -> torch.Tensor:
        B = int(obs.shape[0])
        q = torch.empty(B, self.num_actions, dtype=torch.float32, device=self.device)
        check(lib().acme_dqn_q_values(self._h, ptr(obs.contiguous()), B, 1 if use_target else 0,
                                      ptr(q), stream_ptr(stream)), "dqn q_values")
        return q


def nccl_unique_id() -> bytes:
    """A fresh RCCL unique id (128 bytes) for nccl_comm_init on every rank."""
    buf = (ctypes.c_uint8 * 128)()
    check(lib().acme_nccl_get_unique_id(buf), "nccl unique id")
    return bytes(buf)


def nccl_comm_init(uid: bytes, world_size: int, rank: int) -> int:
    """An RCCL communicator handle (ncclComm_t as an int) for rank of world_size."""
    buf = (ctypes.c_uint8 * 128).from_buffer_copy(uid)
    comm = ctypes.c_void_p()
    check(lib().acme_nccl_comm_init(buf, int(world_size), int(rank), ctypes.byref(comm)),
          "nccl comm init")
    return int(comm.value)


def nccl_comm_destroy(comm: int) -> None:
    check(lib().acme_nccl_comm_destroy(ctypes.c_void_p(comm)), "nccl comm destroy")


class _NativeActorCritic(_NativeLearner):
    """The actor-critic learner handle shared by NativeD4PG, NativeDDPG and NativeMPO: flat
    buffers (policy tensors first, then critic tensors), batch validation, step, policy.
    Subclasses name the C ABI prefix ("acme_d4pg" / "acme_ddpg" / "acme_mpo") and the config
    struct, and fill the fields only they have; NativeMPO has a step and a policy of its own."""

    _config = None   # ctypes config struct

    def _setup(self, *, obs_dim, act_dim, max_batch, policy_sizes, critic_sizes, action_min,
               action_max, discount, target_update_period, policy_learning_rate,
               critic_learning_rate, clipping, adam_beta1, adam_beta2, adam_epsilon,
               layer_norm_epsilon, device, **extra):
        _lib.require_gpu()
        cfg = self._config()
        cfg.obs_dim, cfg.act_dim, cfg.max_batch = int(obs_dim), int(act_dim), int(max_batch)
        for n, sizes in (("policy", policy_sizes), ("critic", critic_sizes)):
            if not 1 <= len(sizes) <= _lib.D4PG_MAX_LAYERS:
                raise ValueError(f"{n} needs 1..{_lib.D4PG_MAX_LAYERS} layer sizes")
        cfg.num_policy_layers = len(policy_sizes)
        cfg.num_critic_layers = len(critic_sizes)
        for i, s in enumerate(policy_sizes):
            cfg.policy_sizes[i] = int(s)
        for i, s in enumerate(critic_sizes):
            cfg.critic_sizes[i] = int(s)
        if act_dim > _lib.D4PG_MAX_ACT:
            raise ValueError(f"act_dim must be <= {_lib.D4PG_MAX_ACT}")
        lo = np.broadcast_to(np.asarray(-1.0 if action_min is None else action_min, np.float32),
                             (act_dim,))
        hi = np.broadcast_to(np.asarray(1.0 if action_max is None else action_max, np.float32),
                             (act_dim,))
        if hasattr(cfg, "action_min"):  # acme_crr_config has no action range
            for j in range(act_dim):
                cfg.action_min[j], cfg.action_max[j] = float(lo[j]), float(hi[j])
        for k, v in extra.items():  # the fields only this learner has
            setattr(cfg, k, v)
        cfg.discount = discount
        if target_update_period is not None:  # MPO has two periods of its own
            cfg.target_update_period = int(target_update_period)
        cfg.policy_learning_rate, cfg.critic_learning_rate = policy_learning_rate, critic_learning_rate
        cfg.adam_beta1, cfg.adam_beta2, cfg.adam_epsilon = adam_beta1, adam_beta2, adam_epsilon
        cfg.clipping = 1 if clipping else 0
        cfg.layer_norm_epsilon = layer_norm_epsilon
        self.obs_dim, self.act_dim, self.max_batch = int(obs_dim), int(act_dim), int(max_batch)
        self._create(cfg, device)
        self.policy_size = int(self._fn("policy_size")(self._h))
        d = self.device
        self.critic_loss = torch.zeros(1, dtype=torch.float32, device=d)
        self.policy_loss = torch.zeros(1, dtype=torch.float32, device=d)

    def _check_batch(self, o_tm1, a_tm1, r_t, d_t, o_t) -> int:
        """Validates the transition tensors every step takes; returns the batch size."""
        B = int(r_t.shape[0])
        for name, t, cols in (("o_tm1", o_tm1, self.obs_dim), ("a_tm1", a_tm1, self.act_dim),
                              ("r_t", r_t, None), ("d_t", d_t, None), ("o_t", o_t, self.obs_dim)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous()
                    and t.dtype == torch.float32):
                raise ValueError(f"{name} must be a contiguous float32 device tensor")
            if t.shape[0] != B or (cols is not None and t.numel() != B * cols):
                raise ValueError(f"{name} has shape {tuple(t.shape)}, expected [{B}, {cols}]")
        return B

    def step(self, o_tm1, a_tm1, r_t, d_t, o_t, stream=None):
        B = self._check_batch(o_tm1, a_tm1, r_t, d_t, o_t)
        b = _lib.D4PGBatch()
        b.o_tm1, b.a_tm1, b.r_t, b.d_t, b.o_t = (ptr(o_tm1), ptr(a_tm1), ptr(r_t), ptr(d_t),
                                                 ptr(o_t))
        b.batch = B
        out = _lib.D4PGOutputs()
        out.critic_loss, out.policy_loss = ptr(self.critic_loss), ptr(self.policy_loss)
        check(self._fn("step")(self._h, ctypes.byref(b), ctypes.byref(out),
                                   stream_ptr(stream)), f"{self._tag} step")

    def policy(self, obs: torch.Tensor, use_target: bool = False, stream=None) -> torch.Tensor:
        rows = int(obs.shape[0])
        obs = obs.reshape(rows, -1).to(self.device, torch.float32).contiguous()
        if obs.shape[1] != self.obs_dim:
            raise ValueError(f"observations must have {self.obs_dim} features")
        a = torch.empty(rows, self.act_dim, dtype=torch.float32, device=self.device)
        check(self._fn("policy")(self._h, ptr(obs), rows, 1 if use_target else 0, ptr(a),
                                     stream_ptr(stream)), f"{self._tag} policy")
        return a


class NativeD4PG(_NativeActorCritic):
    """acme_d4pg learner + its flat buffers (policy tensors first, then critic tensors)."""

    _prefix, _tag, _config = "acme_d4pg", "d4pg", _lib.D4PGConfig

    def __init__(self, *, obs_dim: int, act_dim: int, max_batch: int,
                 policy_sizes: Sequence[int] = (256, 256, 256),
                 critic_sizes: Sequence[int] = (512, 512, 256), num_atoms: int = 51,
                 vmin: float = -150.0, vmax: float = 150.0, action_min=None, action_max=None,
                 discount: float = 0.99, target_update_period: int = 100,
                 policy_learning_rate: float = 1e-4, critic_learning_rate: float = 1e-4,
                 clipping: bool = True, adam_beta1: float = 0.9, adam_beta2: float = 0.999,
                 adam_epsilon: float = 1e-8, layer_norm_epsilon: float = 1e-5, device=None):
        self._setup(obs_dim=obs_dim, act_dim=act_dim, max_batch=max_batch,
                    policy_sizes=policy_sizes, critic_sizes=critic_sizes,
                    action_min=action_min, action_max=action_max, discount=discount,
                    target_update_period=target_update_period,
                    policy_learning_rate=policy_learning_rate,
                    critic_learning_rate=critic_learning_rate, clipping=clipping,
                    adam_beta1=adam_beta1, adam_beta2=adam_beta2, adam_epsilon=adam_epsilon,
                    layer_norm_epsilon=layer_norm_epsilon, device=device,
                    num_atoms=int(num_atoms), vmin=vmin, vmax=vmax)


class NativeDDPG(_NativeActorCritic):
    """acme_ddpg learner (scalar critic LayerNormMLP(critic_sizes + (1,)), TD loss) + its
    flat buffers; the surface of NativeD4PG."""

    _prefix, _tag, _config = "acme_ddpg", "ddpg", _lib.DDPGConfig

    def __init__(self, *, obs_dim: int, act_dim: int, max_batch: int,
                 policy_sizes: Sequence[int] = (256, 256, 256),
                 critic_sizes: Sequence[int] = (512, 512, 256), action_min=None,
                 action_max=None, discount: float = 0.99, target_update_period: int = 100,
                 policy_learning_rate: float = 1e-4, critic_learning_rate: float = 1e-4,
                 clipping: bool = True, adam_beta1: float = 0.9, adam_beta2: float = 0.999,
                 adam_epsilon: float = 1e-8, layer_norm_epsilon: float = 1e-5, device=None):
        self._setup(obs_dim=obs_dim, act_dim=act_dim, max_batch=max_batch,
                    policy_sizes=policy_sizes, critic_sizes=critic_sizes,
                    action_min=action_min, action_max=action_max, discount=discount,
                    target_update_period=target_update_period,
                    policy_learning_rate=policy_learning_rate,
                    critic_learning_rate=critic_learning_rate, clipping=clipping,
                    adam_beta1=adam_beta1, adam_beta2=adam_beta2, adam_epsilon=adam_epsilon,
                    layer_norm_epsilon=layer_norm_epsilon, device=device)


class NativeMPO(_NativeActorCritic):
    """acme_mpo learner (Gaussian policy head, N sampled actions per state, scalar critic,
    decoupled MPO loss) + its flat buffers: policy tensors, critic tensors, then the dual
    variables `mpo/log_*`, which so share `views`, `get_params` and the Adam moment buffers.
    The step's stats are device tensors: `stats` (in `stat_names` order), `kl_mean_rel` and
    `kl_stddev_rel` ([act_dim] with per_dim_constraining, else [1])."""

    _prefix, _tag, _config = "acme_mpo", "mpo", _lib.MPOConfig
    stat_names = _lib.MPO_STATS
    _more_config: Dict = {}  # config fields a derived learner adds (NativeDMPO)

    def __init__(self, *, obs_dim: int, act_dim: int, max_batch: int,
                 policy_sizes: Sequence[int] = (256, 256, 256),
                 critic_sizes: Sequence[int] = (512, 512, 256), num_samples: int = 20,
                 discount: float = 0.99, target_policy_update_period: int = 100,
                 target_critic_update_period: int = 100, policy_learning_rate: float = 1e-4,
                 critic_learning_rate: float = 1e-4, dual_learning_rate: float = 1e-2,
                 clipping: bool = True, epsilon: float = 1e-1, epsilon_mean: float = 1e-3,
                 epsilon_stddev: float = 1e-6, epsilon_penalty: float = 1e-3,
                 init_log_temperature: float = 1.0, init_log_alpha_mean: float = 1.0,
                 init_log_alpha_stddev: float = 10.0, per_dim_constraining: bool = True,
                 action_penalization: bool = True, init_scale: float = 0.3,
                 min_scale: float = 1e-6, seed: int = 0, adam_beta1: float = 0.9,
                 adam_beta2: float = 0.999, adam_epsilon: float = 1e-8,
                 layer_norm_epsilon: float = 1e-5, device=None):
        if not 1 <= num_samples <= _lib.MPO_MAX_SAMPLES:
            raise ValueError(f"num_samples must be in [1, {_lib.MPO_MAX_SAMPLES}]")
        self.num_samples = int(num_samples)
        self._setup(obs_dim=obs_dim, act_dim=act_dim, max_batch=max_batch,
                    policy_sizes=policy_sizes, critic_sizes=critic_sizes, action_min=None,
                    action_max=None, discount=discount, target_update_period=None,
                    policy_learning_rate=policy_learning_rate,
                    critic_learning_rate=critic_learning_rate, clipping=clipping,
                    adam_beta1=adam_beta1, adam_beta2=adam_beta2, adam_epsilon=adam_epsilon,
                    layer_norm_epsilon=layer_norm_epsilon, device=device,
                    num_samples=int(num_samples),
                    target_policy_update_period=int(target_policy_update_period),
                    target_critic_update_period=int(target_critic_update_period),
                    dual_learning_rate=dual_learning_rate, epsilon=epsilon,
                    epsilon_mean=epsilon_mean, epsilon_stddev=epsilon_stddev,
                    epsilon_penalty=epsilon_penalty, init_log_temperature=init_log_temperature,
                    init_log_alpha_mean=init_log_alpha_mean,
                    init_log_alpha_stddev=init_log_alpha_stddev,
                    per_dim_constraining=1 if per_dim_constraining else 0,
                    action_penalization=1 if action_penalization else 0,
                    init_scale=init_scale, min_scale=min_scale,
                    seed=int(seed) & 0xFFFFFFFFFFFFFFFF, **self._more_config)
        self.dual_offset = int(self._fn("dual_offset")(self._h))
        self.dual_dim = self.act_dim if per_dim_constraining else 1
        check(self._fn("init_duals")(self._h), "mpo init_duals")
        d = self.device
        self.stats = torch.zeros(len(self.stat_names), dtype=torch.float32, device=d)
        self.kl_mean_rel = torch.zeros(self.dual_dim, dtype=torch.float32, device=d)
        self.kl_stddev_rel = torch.zeros(self.dual_dim, dtype=torch.float32, device=d)

    def set_params(self, params: Dict[str, np.ndarray], target: Optional[Dict] = None) -> None:
        """As the other learners'; dual variables absent from `params` keep their values (the
        initial ones after construction), and the target buffer's dual slots are never used."""
        for flat, src in ((self.params, params), (self.target, target if target is not None else params)):
            for name, t in self.views(flat).items():
                if name in src:
                    t.copy_(torch.as_tensor(np.asarray(src[name], np.float32)).view(t.shape))
                elif not name.startswith("mpo/"):
                    raise KeyError(name)

    def stat(self, name: str) -> torch.Tensor:
        """One entry of the reference's stats dict as a device scalar (a view of `stats`)."""
        if name in ("kl_mean_rel", "kl_stddev_rel"):
            return getattr(self, name)
        return self.stats[self.stat_names.index(name)]

    def step(self, o_tm1, a_tm1, r_t, d_t, o_t, noise=None, stream=None):
        """One learner step.  `noise`: eps [num_samples, B, act_dim] to sample the target
        policy's actions with (tests); None: generated on the device from (seed, step)."""
        B = self._check_batch(o_tm1, a_tm1, r_t, d_t, o_t)
        b = _lib.MPOBatch()
        b.o_tm1, b.a_tm1, b.r_t, b.d_t, b.o_t = (ptr(o_tm1), ptr(a_tm1), ptr(r_t), ptr(d_t),
                                                 ptr(o_t))
        b.batch = B
        if noise is not None:
            if not (isinstance(noise, torch.Tensor) and noise.is_cuda and noise.is_contiguous()
                    and noise.dtype == torch.float32
                    and noise.numel() == self.num_samples * B * self.act_dim):
                raise ValueError(f"noise must be a contiguous float32 device tensor of shape "
                                 f"[{self.num_samples}, {B}, {self.act_dim}]")
            b.noise = ptr(noise)
        out = _lib.MPOOutputs()
        out.critic_loss, out.policy_loss = ptr(self.critic_loss), ptr(self.policy_loss)
        out.stats, out.kl_mean_rel = ptr(self.stats), ptr(self.kl_mean_rel)
        out.kl_stddev_rel = ptr(self.kl_stddev_rel)
        check(self._fn("step")(self._h, ctypes.byref(b), ctypes.byref(out), stream_ptr(stream)),
              f"{self._tag} step")

    def policy_distribution(self, obs: torch.Tensor, use_target: bool = False, stream=None):
        """(mean, stddev) [rows, act_dim] of the policy's diagonal Gaussian."""
        rows = int(obs.shape[0])
        obs = obs.reshape(rows, -1).to(self.device, torch.float32).contiguous()
        if obs.shape[1] != self.obs_dim:
            raise ValueError(f"observations must have {self.obs_dim} features")
        mean = torch.empty(rows, self.act_dim, dtype=torch.float32, device=self.device)
        stddev = torch.empty_like(mean)
        check(self._fn("policy")(self._h, ptr(obs), rows, 1 if use_target else 0, ptr(mean),
                                 ptr(stddev), stream_ptr(stream)), "mpo policy")
        return mean, stddev

    def policy(self, obs: torch.Tensor, use_target: bool = False, stream=None) -> torch.Tensor:
        """The distribution's mean (the greedy action)."""
        return self.policy_distribution(obs, use_target, stream)[0]


class NativeDMPO(NativeMPO):
    """acme_dmpo learner: NativeMPO's policy side, duals, step and stats with D4PG's categorical
    critic (DiscreteValuedHead over `num_atoms` atoms on [vmin, vmax]); the surface of
    NativeMPO plus `values`, the support."""

    _prefix, _tag, _config = "acme_dmpo", "dmpo", _lib.DMPOConfig

    def __init__(self, *, num_atoms: int = 51, vmin: float = -150.0, vmax: float = 150.0,
                 **mpo_args):
        self.num_atoms, self.vmin, self.vmax = int(num_atoms), float(vmin), float(vmax)
        self._more_config = dict(num_atoms=self.num_atoms, vmin=self.vmin, vmax=self.vmax)
        super().__init__(**mpo_args)

    @property
    def values(self) -> np.ndarray:
        """The support: tf.linspace(vmin, vmax, num_atoms), as the learner computes it."""
        step = (np.float64(self.vmax) - np.float64(self.vmin)) / (self.num_atoms - 1)
        return (np.float64(self.vmin) + np.arange(self.num_atoms) * step).astype(np.float32)


class NativeCRR(_NativeActorCritic):
    """acme_crr learner (offline actor-critic: NativeMPO's Gaussian policy, NativeDMPO's
    categorical critic, the advantage-weighted behaviour-cloning loss, no duals) + its flat
    buffers: policy tensors, then critic tensors.  A step takes R = B (T - 1) transitions
    (`flatten_sequences`); `sequence_length` T is the reference's loss divisor.  The step's
    outputs are the device scalars `critic_loss`, `policy_loss` and `policy_loss_coef`."""

    _prefix, _tag, _config = "acme_crr", "crr", _lib.CRRConfig

    def __init__(self, *, obs_dim: int, act_dim: int, max_batch: int, sequence_length: int,
                 policy_sizes: Sequence[int] = (256, 256, 256),
                 critic_sizes: Sequence[int] = (512, 512, 256), num_atoms: int = 51,
                 vmin: float = -150.0, vmax: float = 150.0, discount: float = 0.99,
                 target_update_period: int = 100, num_action_samples_td_learning: int = 1,
                 num_action_samples_policy_weight: int = 4,
                 baseline_reduce_function: str = "mean", policy_improvement_modes: str = "exp",
                 ratio_upper_bound: float = 20.0, beta: float = 1.0,
                 policy_learning_rate: float = 1e-4, critic_learning_rate: float = 1e-4,
                 clipping: bool = True, init_scale: float = 0.3, min_scale: float = 1e-6,
                 seed: int = 0, adam_beta1: float = 0.9, adam_beta2: float = 0.999,
                 adam_epsilon: float = 1e-8, layer_norm_epsilon: float = 1e-5, device=None):
        for name, n in (("num_action_samples_td_learning", num_action_samples_td_learning),
                        ("num_action_samples_policy_weight", num_action_samples_policy_weight)):
            if not 1 <= n <= _lib.MPO_MAX_SAMPLES:
                raise ValueError(f"{name} must be in [1, {_lib.MPO_MAX_SAMPLES}]")
        if baseline_reduce_function not in _lib.CRR_REDUCE:
            raise ValueError(f"baseline_reduce_function must be one of {_lib.CRR_REDUCE}")
        if policy_improvement_modes not in _lib.CRR_MODES:
            raise ValueError(f"policy_improvement_modes must be one of {_lib.CRR_MODES}")
        if sequence_length < 2:
            raise ValueError("sequence_length must be >= 2")
        self.num_samples_td = int(num_action_samples_td_learning)
        self.num_samples_pw = int(num_action_samples_policy_weight)
        self.sequence_length = int(sequence_length)
        self.num_atoms, self.vmin, self.vmax = int(num_atoms), float(vmin), float(vmax)
        self._setup(obs_dim=obs_dim, act_dim=act_dim, max_batch=max_batch,
                    policy_sizes=policy_sizes, critic_sizes=critic_sizes, action_min=None,
                    action_max=None, discount=discount,
                    target_update_period=target_update_period,
                    policy_learning_rate=policy_learning_rate,
                    critic_learning_rate=critic_learning_rate, clipping=clipping,
                    adam_beta1=adam_beta1, adam_beta2=adam_beta2, adam_epsilon=adam_epsilon,
                    layer_norm_epsilon=layer_norm_epsilon, device=device,
                    num_atoms=self.num_atoms, vmin=self.vmin, vmax=self.vmax,
                    init_scale=init_scale, min_scale=min_scale,
                    num_action_samples_td_learning=self.num_samples_td,
                    num_action_samples_policy_weight=self.num_samples_pw,
                    baseline_reduce_function=_lib.CRR_REDUCE.index(baseline_reduce_function),
                    policy_improvement_modes=_lib.CRR_MODES.index(policy_improvement_modes),
                    ratio_upper_bound=ratio_upper_bound, beta=beta,
                    sequence_length=self.sequence_length,
                    seed=int(seed) & 0xFFFFFFFFFFFFFFFF)
        self.policy_loss_coef = torch.zeros(1, dtype=torch.float32, device=self.device)

    values = NativeDMPO.values

    @staticmethod
    def flatten_sequences(observation, action, reward, discount):
        """[B, T, ...] sequences as the R = B (T - 1) transitions of the reference's loop over
        t (recurrent_learning.py:229-234), row b (T - 1) + (t - 1): (o_tm1, a_tm1, r_t, d_t,
        o_t) = (o[:, :-1], a[:, :-1], r[:, :-1], d[:, :-1], o[:, 1:])."""
        B, T = int(action.shape[0]), int(action.shape[1])
        R = B * (T - 1)
        o = observation.reshape(B, T, -1)
        flat = lambda x: x.reshape(R, -1).to(torch.float32).contiguous()  # noqa: E731
        return (flat(o[:, :-1]), flat(action.reshape(B, T, -1)[:, :-1]),
                flat(reward.reshape(B, T)[:, :-1]).reshape(R),
                flat(discount.reshape(B, T)[:, :-1]).reshape(R), flat(o[:, 1:]))

    def step(self, o_tm1, a_tm1, r_t, d_t, o_t, noise=None, stream=None):
        """One learner step over R transitions (a multiple of sequence_length - 1).  `noise`:
        eps [N_td + N_pw, R, act_dim] for the two action sets (tests); None: generated on the
        device from (seed, step)."""
        R = self._check_batch(o_tm1, a_tm1, r_t, d_t, o_t)
        b = _lib.MPOBatch()
        b.o_tm1, b.a_tm1, b.r_t, b.d_t, b.o_t = (ptr(o_tm1), ptr(a_tm1), ptr(r_t), ptr(d_t),
                                                 ptr(o_t))
        b.batch = R
        n = self.num_samples_td + self.num_samples_pw
        if noise is not None:
            if not (isinstance(noise, torch.Tensor) and noise.is_cuda and noise.is_contiguous()
                    and noise.dtype == torch.float32 and noise.numel() == n * R * self.act_dim):
                raise ValueError(f"noise must be a contiguous float32 device tensor of shape "
                                 f"[{n}, {R}, {self.act_dim}]")
            b.noise = ptr(noise)
        out = _lib.CRROutputs()
        out.critic_loss, out.policy_loss = ptr(self.critic_loss), ptr(self.policy_loss)
        out.policy_loss_coef = ptr(self.policy_loss_coef)
        check(self._fn("step")(self._h, ctypes.byref(b), ctypes.byref(out), stream_ptr(stream)),
              "crr step")

    policy_distribution = NativeMPO.policy_distribution
    policy = NativeMPO.policy


class NativeAZ(_NativeLearner):
    """acme_az learner (policy-value MLP, soft-label cross-entropy + TD value loss, Adam) + its
    flat buffers, and the network evaluation the MCTS actor calls once per tree node.  The
    step's losses are the device scalars `loss`, `value_loss`, `policy_loss`."""

    _prefix, _tag = "acme_az", "az"
    _has_target = False

    def __init__(self, *, obs_dim: int, hidden: Sequence[int], num_actions: int, max_batch: int,
                 max_eval_rows: int = 1, activate_final: bool = False, discount: float = 1.0,
                 learning_rate: float = 1e-3, adam_beta1: float = 0.9,
                 adam_beta2: float = 0.999, adam_epsilon: float = 1e-8, device=None):
        cfg = _lib.AZConfig()
        if not 1 <= len(hidden) <= _lib.MAX_MLP_LAYERS:
            raise ValueError(f"hidden needs 1..{_lib.MAX_MLP_LAYERS} layer sizes")
        cfg.obs_dim, cfg.num_actions = int(obs_dim), int(num_actions)
        cfg.max_batch, cfg.max_eval_rows = int(max_batch), int(max_eval_rows)
        cfg.num_hidden = len(hidden)
        for i, s in enumerate(hidden):
            cfg.hidden[i] = int(s)
        cfg.activate_final = 1 if activate_final else 0
        cfg.discount, cfg.learning_rate = float(discount), float(learning_rate)
        cfg.adam_beta1, cfg.adam_beta2, cfg.adam_epsilon = adam_beta1, adam_beta2, adam_epsilon
        self.obs_dim, self.num_actions = int(obs_dim), int(num_actions)
        self.max_batch, self.max_eval_rows = int(max_batch), int(max_eval_rows)
        self.learning_rate = float(learning_rate)
        _lib.require_gpu()
        self._create(cfg, device)
        d = self.device
        self._losses = torch.zeros(3, dtype=torch.float32, device=d)
        self.loss, self.value_loss, self.policy_loss = (self._losses[i:i + 1] for i in range(3))
        self._out = _lib.AZOutputs()
        self._out.loss, self._out.value_loss, self._out.policy_loss = (
            ptr(self.loss), ptr(self.value_loss), ptr(self.policy_loss))

    def _check_batch(self, o_t, r_t, d_t, o_tp1, pi) -> int:
        B = int(r_t.shape[0])
        for name, t, cols in (("o_t", o_t, self.obs_dim), ("r_t", r_t, 1), ("d_t", d_t, 1),
                              ("o_tp1", o_tp1, self.obs_dim), ("pi", pi, self.num_actions)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous()
                    and t.dtype == torch.float32):
                raise ValueError(f"{name} must be a contiguous float32 device tensor")
            if t.shape[0] != B or t.numel() != B * cols:
                raise ValueError(f"{name} has shape {tuple(t.shape)}, expected [{B}, {cols}]")
        return B

    def step(self, o_t, r_t, d_t, o_tp1, pi, stream=None):
        b = _lib.AZBatch()
        b.batch = self._check_batch(o_t, r_t, d_t, o_tp1, pi)
        b.o_t, b.r_t, b.d_t, b.o_tp1, b.pi = ptr(o_t), ptr(r_t), ptr(d_t), ptr(o_tp1), ptr(pi)
        check(self._fn("step")(self._h, ctypes.byref(b), ctypes.byref(self._out),
                               stream_ptr(stream)), "az step")

    def evaluate_packed(self, obs: torch.Tensor, stream=None) -> torch.Tensor:
        """probs [rows, A] then value [rows] of device observations [rows, obs_dim], packed in
        one device buffer of rows (A + 1) floats (one copy brings both to the host)."""
        rows, A = int(obs.shape[0]), self.num_actions
        if not (obs.is_cuda and obs.dtype == torch.float32 and obs.is_contiguous()
                and obs.numel() == rows * self.obs_dim):
            raise ValueError(f"observations must be contiguous float32 [rows, {self.obs_dim}] "
                             "on the device")
        out = torch.empty(rows * (A + 1), dtype=torch.float32, device=self.device)
        check(self._fn("evaluate")(self._h, ptr(obs), rows, ptr(out),
                                   out.data_ptr() + 4 * rows * A, stream_ptr(stream)),
              "az evaluate")
        return out

    def evaluate(self, obs: torch.Tensor, stream=None):
        """(probs [rows, A], value [rows]) as device tensors (views of one buffer)."""
        rows, A = int(obs.shape[0]), self.num_actions
        out = self.evaluate_packed(obs, stream)
        return out[:rows * A].view(rows, A), out[rows * A:]


class NativeIMPALA(_PlaneOverflow, _PlaneState, _NativeLearner):
    """acme_impala learner + its flat buffers (no target network)."""

    _prefix, _tag, _has_target = "acme_impala", "impala", False
    _guard_fields = _PlaneState._guard_fields + ("lstm_timeouts",)

    def __init__(self, *, num_actions: int, max_batch: int, max_sequence_length: int,
                 torso: str = "atari", obs_dim: int = 0, lstm_size: int = 256,
                 head_size: int = 256, discount: float = 0.99, entropy_cost: float = 0.0,
                 baseline_cost: float = 1.0, max_abs_reward: Optional[float] = None,
                 max_gradient_norm: Optional[float] = None, learning_rate: float = 1e-3,
                 adam_beta1: float = 0.9, adam_beta2: float = 0.999, adam_epsilon: float = 1e-8,
                 semantics: str = "tf", device=None, shared_params: Optional[torch.Tensor] = None):
        """semantics: "tf" (acme/agents/tf/impala) or "jax" (acme/agents/jax/impala: the
        optix.chain(clip_by_global_norm, adam) update; max_gradient_norm None = inf).
        shared_params: bind another instance's parameter buffer (an actor-side network with
        its own workspace, reading the learner's current parameters)."""
        _lib.require_gpu()
        if semantics not in ("tf", "jax"):
            raise ValueError(f"semantics must be 'tf' or 'jax', got {semantics!r}")
        cfg = _lib.IMPALAConfig()
        cfg.torso = _lib.IMPALA_TORSO_ATARI if torso == "atari" else _lib.IMPALA_TORSO_FLAT
        cfg.obs_dim, cfg.num_actions = int(obs_dim), int(num_actions)
        cfg.max_batch, cfg.max_sequence_length = int(max_batch), int(max_sequence_length)
        cfg.lstm_size, cfg.head_size = int(lstm_size), int(head_size)
        cfg.discount, cfg.entropy_cost, cfg.baseline_cost = discount, entropy_cost, baseline_cost
        # learning.py:67-71: None -> no reward clipping, gradient norm 1e10.
        cfg.max_abs_reward = float("inf") if max_abs_reward is None else max_abs_reward
        cfg.max_gradient_norm = ((float("inf") if semantics == "jax" else 1e10)
                                 if max_gradient_norm is None else max_gradient_norm)
        cfg.semantics = _lib.SEMANTICS_JAX if semantics == "jax" else _lib.SEMANTICS_TF
        cfg.learning_rate = learning_rate
        cfg.adam_beta1, cfg.adam_beta2, cfg.adam_epsilon = adam_beta1, adam_beta2, adam_epsilon
        self.torso, self.obs_dim = torso, int(obs_dim)
        self.num_actions, self.lstm_size = int(num_actions), int(lstm_size)
        self.max_batch, self.max_sequence_length = int(max_batch), int(max_sequence_length)
        self._create(cfg, device, shared_params)
        self.metrics = torch.zeros(4, dtype=torch.float32, device=self.device)

    def set_params(self, params: Dict[str, np.ndarray]) -> None:
        super().set_params(params)

    def set_policy_planes(self, on: bool = True) -> None:
        """Policy steps (>= 64 rows, Atari torso) on the plane engine: for actor-side networks
        that only run policy steps (acme_impala_set_policy_planes)."""
        check(lib().acme_impala_set_policy_planes(self._h, 1 if on else 0), "policy planes")

    def set_lstm_unroll(self, per_step: bool) -> None:
        """Per-step LSTM launches instead of the one-launch unroll (tests compare the two)."""
        check(lib().acme_impala_set_lstm_unroll(self._h, 1 if per_step else 0), "lstm unroll")

    def step(self, observation, prev_action, prev_reward, action, reward, discount,
             behaviour_logits, h0, c0, stream=None):
        """Batch-major [B, T, ...] device tensors; h0 / c0 are [B, H] views (any row stride
        that is a multiple of 4 floats, e.g. core_state[:, 0] of a [B, T, H] tensor)."""
        b = self._sequence_batch(observation, prev_action, prev_reward, action, reward, discount,
                                 h0, c0, behaviour_logits=behaviour_logits)
        check(lib().acme_impala_step(self._h, ctypes.byref(b), ptr(self.metrics),
                                     stream_ptr(stream)), "impala step")

    def policy_step(self, obs, prev_action, prev_reward, h, c, stream=None, out=None):
        """One network step for `rows` actors; returns (logits, values, h, c) (into `out`,
        four contiguous device tensors of those shapes, when given)."""
        rows = int(prev_action.shape[0])
        if out is None:
            out = self._acting_outputs(rows, torch.float32)
        check(lib().acme_impala_policy_step(
            self._h, ptr(obs.contiguous()), ptr(prev_action.contiguous()),
            ptr(prev_reward.contiguous()), ptr(h.contiguous()), ptr(c.contiguous()), rows,
            *[ptr(o) for o in out], stream_ptr(stream)), "impala policy_step")
        return tuple(out)


class NativeR2D2(_PlaneState, _NativeLearner):
    """acme_r2d2 learner + its flat buffers (params, target, grads, Adam m / v):
    R2D2Learner._step (acme/agents/tf/r2d2/learning.py:112-200) on R2D2AtariNetwork."""

    _prefix, _tag = "acme_r2d2", "r2d2"

    def __init__(self, *, num_actions: int, max_batch: int, max_sequence_length: int,
                 burn_in_length: int, torso: str = "atari", obs_dim: int = 0,
                 lstm_size: int = 512, head_size: int = 512, n_step: int = 5,
                 discount: float = 0.99, importance_sampling_exponent: float = 0.2,
                 max_replay_size: int = 1_000_000, max_priority_weight: float = 0.9,
                 target_update_period: int = 100, learning_rate: float = 1e-3,
                 adam_beta1: float = 0.9, adam_beta2: float = 0.999, adam_epsilon: float = 1e-3,
                 store_lstm_state: bool = True, device=None):
        """Defaults are R2D2Learner's (learning.py:47-66; snt.Adam epsilon 1e-3, :78)."""
        _lib.require_gpu()
        cfg = _lib.R2D2Config()
        cfg.torso = _lib.IMPALA_TORSO_ATARI if torso == "atari" else _lib.IMPALA_TORSO_FLAT
        cfg.obs_dim, cfg.num_actions = int(obs_dim), int(num_actions)
        cfg.max_batch, cfg.max_sequence_length = int(max_batch), int(max_sequence_length)
        cfg.burn_in_length = int(burn_in_length)
        cfg.lstm_size, cfg.head_size, cfg.n_step = int(lstm_size), int(head_size), int(n_step)
        cfg.store_lstm_state = 1 if store_lstm_state else 0
        cfg.target_update_period = int(target_update_period)
        cfg.max_replay_size = int(max_replay_size)
        cfg.discount = discount
        cfg.importance_sampling_exponent = importance_sampling_exponent
        cfg.max_priority_weight = max_priority_weight
        cfg.learning_rate = learning_rate
        cfg.adam_beta1, cfg.adam_beta2, cfg.adam_epsilon = adam_beta1, adam_beta2, adam_epsilon
        self.torso, self.obs_dim = torso, int(obs_dim)
        self.num_actions, self.lstm_size = int(num_actions), int(lstm_size)
        self.max_batch, self.max_sequence_length = int(max_batch), int(max_sequence_length)
        self.burn_in_length = int(burn_in_length)
        self.store_lstm_state = bool(store_lstm_state)
        self._create(cfg, device)
        T, B = self.max_sequence_length, self.max_batch
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._errors = torch.zeros(max(T - self.burn_in_length - 1, 1) * B, dtype=torch.float32,
                                   device=self.device)
        self._last = (1, B)
        self.priorities = torch.zeros(B, dtype=torch.float64, device=self.device)

    @property
    def errors(self) -> torch.Tensor:
        """The last step's errors [T - burn_in - 1, B] (time-major, extra.errors)."""
        tm, b = self._last
        return self._errors[:tm * b].view(tm, b)

    def set_params(self, params: Dict[str, np.ndarray], target: Dict[str, np.ndarray]) -> None:
        super().set_params(params, target)

    @property
    def skip_word(self) -> Optional[int]:
        return lib().acme_r2d2_skip_word(self._h) or None

    def set_lstm_unroll(self, per_step: bool) -> None:
        """per_step=True: one LSTM launch per time step instead of the one-launch unroll."""
        check(lib().acme_r2d2_set_lstm_unroll(self._h, 1 if per_step else 0), "r2d2 lstm unroll")

    def step(self, observation, prev_action, prev_reward, action, reward, discount,
             probabilities, h0=None, c0=None, stream=None):
        """Batch-major [B, T, ...] device tensors (the sequence dataset's layout: the OAR
        observation's frames, previous action and reward; action, reward, discount), the
        sample's probabilities [B] (f64) and the core state at t = 0 (h0 / c0 [B, H] views
        with unit inner stride; ignored with store_lstm_state=False).  Loss, errors
        [T - burn_in - 1, B] and priorities [B] land in .loss / .errors / .priorities."""
        b = self._sequence_batch(observation, prev_action, prev_reward, action, reward, discount,
                                 h0, c0, core_state=self.store_lstm_state)
        B, T = int(b.batch), int(b.sequence_length)
        if not (probabilities.is_cuda and probabilities.dtype == torch.float64
                and probabilities.is_contiguous() and probabilities.numel() == B):
            raise ValueError(f"probabilities must be a contiguous float64 [{B}] device tensor")
        o = _lib.R2D2Outputs()
        o.loss, o.errors, o.priorities = ptr(self.loss), ptr(self._errors), ptr(self.priorities)
        self._last = (T - self.burn_in_length - 1, B)
        check(lib().acme_r2d2_step(self._h, ctypes.byref(b), ptr(probabilities), ctypes.byref(o),
                                   stream_ptr(stream)), "r2d2 step")

    def q_step(self, obs, prev_action, prev_reward, h, c, *, epsilon: float, seed: int,
               step: int, use_target: bool = False, stream=None, out=None):
        """One network step for `rows` actors (acme_r2d2_q_step): device tensors obs
        [rows, ...], prev_action int32 / prev_reward float32 [rows], core state h / c
        [rows, H] float32 views with unit inner stride and one row stride.  Returns (q
        [rows, A], actions int32 [rows], h, c), the epsilon-greedy actions drawn from (seed,
        step, row).  out: four device tensors (or None to skip an output) to write into; the
        state outputs may be h and c themselves."""
        rows = int(prev_action.shape[0])
        H = self.lstm_size
        for name, t in (("h", h), ("c", c)):
            if (t.dtype != torch.float32 or tuple(t.shape) != (rows, H) or t.stride(1) != 1
                    or not t.is_cuda):
                raise ValueError(f"{name} must be a float32 [{rows}, {H}] device tensor with "
                                 "unit inner stride")
        if h.stride(0) != c.stride(0):
            raise ValueError("h and c must share a row stride")
        if out is None:
            out = self._acting_outputs(rows, torch.int32)
        for o in out[2:]:
            if o is not None and not o.is_contiguous():
                raise ValueError("the state outputs must be contiguous [rows, H] tensors")
        check(lib().acme_r2d2_q_step(
            self._h, ptr(obs.contiguous()), ptr(prev_action.contiguous()),
            ptr(prev_reward.contiguous()), ptr(h), ptr(c), int(h.stride(0)), rows,
            1 if use_target else 0, float(epsilon), int(seed) & (2 ** 64 - 1),
            int(step) & (2 ** 64 - 1), *[ptr(o) for o in out], stream_ptr(stream)), "r2d2 q_step")
        return tuple(out)


def epsilon_greedy(q: torch.Tensor, epsilon: float, seed: int, step: int,
                   stream=None) -> torch.Tensor:
    """Epsilon-greedy actions (int32 [rows]) of a contiguous float32 [rows, A] device tensor:
    acme_epsilon_greedy, trfl's epsilon_greedy(q, epsilon).sample() drawn from (seed, step,
    row)."""
    if not (isinstance(q, torch.Tensor) and q.is_cuda and q.dtype == torch.float32
            and q.dim() == 2 and q.is_contiguous()):
        raise ValueError("q must be a contiguous float32 [rows, A] device tensor")
    rows, A = int(q.shape[0]), int(q.shape[1])
    out = torch.empty(rows, dtype=torch.int32, device=q.device)
    with torch.cuda.device(q.device):
        check(lib().acme_epsilon_greedy(ptr(q), rows, A, float(epsilon),
                                        int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1),
                                        ptr(out), stream_ptr(stream)), "epsilon_greedy")
    return out
