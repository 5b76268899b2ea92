"""Numpy oracle of the epsilon-greedy selection (acme_epsilon_greedy and the acting step's
head finish, acme_amd/csrc/kernels.hip) — test infrastructure, no GPU.

select(): the mapping of one Philox4x32-10 call per row (tests/_oracle.philox, the C
restatement of the published generator) to an action, as include/acme_hip.h states it:
counter (row, step lo, step hi, "R2AC"), key = seed; the row explores iff
u01_53(r.x, r.y) < epsilon, then a = (r.z * A) >> 32; otherwise a is the
((r.w * n) >> 32)-th of the n actions equal to the row's maximum (NaNs ignored), ascending;
a row of NaNs gives 0.
"""

import numpy as np

from tests import _oracle
from tests.dqfd_oracle import u01_53

ACT_TAG = 0x52324143  # "R2AC"


def draw(seed, step, row):
    """The four Philox words of (seed, step, row)."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    return _oracle.philox([int(row) & 0xFFFFFFFF, step & 0xFFFFFFFF, step >> 32, ACT_TAG],
                          [seed & 0xFFFFFFFF, seed >> 32])


def greedy_set(q_row):
    """Ascending indices equal to the row's maximum with NaNs ignored (empty: all NaN)."""
    q_row = np.asarray(q_row, np.float32)
    ok = ~np.isnan(q_row)
    if not ok.any():
        return np.zeros(0, np.int64)
    return np.flatnonzero(ok & (q_row == q_row[ok].max()))


def select_row(q_row, epsilon, seed, step, row):
    """(action, explored) of one row."""
    r = draw(seed, step, row)
    A = len(q_row)
    if u01_53(r[0], r[1]) < epsilon:
        return (int(r[2]) * A) >> 32, True
    g = greedy_set(q_row)
    if len(g) == 0:
        return 0, False
    return int(g[(int(r[3]) * len(g)) >> 32]), False


def select(q, epsilon, seed, step, first_row=0):
    """Actions int32 [rows] of q [rows, A]; row i draws as row first_row + i."""
    q = np.asarray(q, np.float32)
    return np.array([select_row(q[i], epsilon, seed, step, first_row + i)[0]
                     for i in range(q.shape[0])], np.int32)
