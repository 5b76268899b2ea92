"""Numpy oracle of the sequence demonstration mix (acme_seq_demo_mix,
acme_amd/csrc/demos.hip) — test infrastructure, no GPU.

- draw(): the per-row mapping of one Philox4x32-10 call (tests/_oracle.philox) to
  (demonstration?, episode, first, to), as _sequence_from_episode draws them
  (acme/agents/tf/r2d3/agent.py:193-196);
- mix(): the draws of a whole batch;
- window(): the zero-padded [T, ...] slice of one per-step array and the row's flag.
"""

import numpy as np

from tests import _oracle
from tests.dqfd_oracle import DEMO_KEY, u01_53  # noqa: F401

SEQ_DEMO_TAG = 0x53455144  # "SEQD"
assert SEQ_DEMO_TAG != 0x44454D4F  # not the transition mix's "DEMO"


def draw(seed, step, j, ratio, lengths, period, sequence_length=None):
    """(is_demo, episode, first, to) of row j of draw `step`; `to` is None without a
    sequence_length.  Episode and window are reported for replay rows too (the kernel does
    not compute them there)."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    r = _oracle.philox([j, step & 0xFFFFFFFF, step >> 32, SEQ_DEMO_TAG],
                       [seed & 0xFFFFFFFF, seed >> 32])
    is_demo = u01_53(r[0], r[1]) < ratio
    e = (int(r[2]) * len(lengths)) >> 32
    L = int(lengths[e])
    pos = (int(r[3]) * L) >> 32
    first = pos // int(period) * int(period)
    to = None if sequence_length is None else min(first + int(sequence_length), L)
    return is_demo, e, first, to


def mix(lengths, seed, step, ratio, period, sequence_length, batch):
    """(is_demo bool [B], {j: (e, first, to)} of the demonstration rows) of one batch."""
    is_demo = np.zeros(batch, bool)
    rows = {}
    for j in range(batch):
        demo, e, first, to = draw(seed, step, j, ratio, lengths, period, sequence_length)
        is_demo[j] = demo
        if demo:
            rows[j] = (e, first, to)
    return is_demo, rows


def window(x, first, to, sequence_length):
    """x[first:to] zero-padded to sequence_length steps (_slice_and_pad)."""
    x = np.asarray(x)
    out = np.zeros((sequence_length,) + x.shape[1:], x.dtype)
    out[:to - first] = x[first:to]
    return out
