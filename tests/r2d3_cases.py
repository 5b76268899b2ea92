"""The cases of tests/test_r2d3_gpu.py::test_mixed_sequences_equal_oracle, kept apart from
the GPU test so that tests/test_r2d3_cpu.py can assert on the oracle alone that they cover
what they are meant to (no GPU, no package import)."""

import numpy as np

MIX_SEED = 4321
DRAWS = 3  # batches drawn per case: draw counters 0, 1, 2
LENGTHS = [1, 2, 9, 40, 4, 17]

# Observation leaf per step: (shape, dtype); the key is its step bytes.
OBS = {3: ((3,), np.uint8),            # the byte path (a window starts at first * 3)
       12: ((3,), np.float32),         # the 4-byte path
       16: ((4,), np.float32),         # the 16-byte path
       28224: ((84, 84, 4), np.uint8)}  # rows of T * 28,224 bytes span several chunks

# (observation step bytes, OAR-nested, T, B, episode lengths, period, ratio)
CASES = [
    (3, False, 9, 33, LENGTHS, 4, 0.5),
    (3, False, 2, 5, LENGTHS, 1, 0.5),
    (3, False, 9, 33, [1], 64, 0.25),
    (12, True, 9, 33, LENGTHS, 1, 0.25),
    (12, False, 2, 33, LENGTHS, 64, 0.5),
    (12, True, 9, 1, LENGTHS, 4, 0.5),
    (16, False, 9, 5, LENGTHS, 4, 1.0),
    (16, False, 2, 33, [1], 1, 1.0),
    (16, False, 9, 33, LENGTHS, 4, 0.0),
    (16, True, 2, 5, LENGTHS, 4, 0.25),
    (28224, True, 5, 5, LENGTHS, 4, 0.5),
    (28224, False, 5, 1, [1], 64, 1.0),
]


def case_id(case) -> str:
    nb, oar, T, B, lengths, period, ratio = case
    return f"{nb}B{'-oar' if oar else ''}-T{T}-B{B}-E{len(lengths)}-p{period}-r{ratio}"
