"""The LDS image geometries of the image-resident convolutions, checked on the host.

tests/p3i_geom_check.cc includes acme_amd/csrc/gemm_p3i_geom.h (no HIP dependency) and, for
every geometry torso.hip instantiates (the sub-pixel input gradient's included) with that
instantiation's frames per block and wave counts, checks the placement of every unit, every
read of every GEMM row against the im2col definition (TF SAME padding), and models the bank
conflicts of the A-fragment
ds_read_b128s with the lane groups of the MI355X LDS: {0-3, 12-15, 20-27}, {4-11, 16-19,
28-31} and the same + 32; bank of byte address a = (a / 4) mod 64; every extra distinct
address on a busy bank costs the lane group one extra cycle.  The program exits non-zero on
a placement or read error and prints "name mean worst" per geometry: the mean extra cycles
per lane-group cycle and the worst lane group's.
"""

import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "acme_amd", "csrc")

# The same program built against the geometry of commit 24393eb (the parent of the banked
# zero units and the class-major strided layouts): mean, worst.
PARENT_24393EB = {
    "conv1_fwd": (1.2667, 3),
    "conv2_fwd": (1.0029, 3),
    "conv3_fwd": (0.4861, 1),
    "conv3_dgrad": (0.4731, 1),
    "conv12_fwd.conv1": (1.1084, 3),
    "conv12_fwd.conv2": (0.9785, 3),
    "conv2_dgrad": (0.5991, 2),
}


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("p3i_geom") / "p3i_geom_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", exe,
                           os.path.join(HERE, "p3i_geom_check.cc")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stderr  # placement and reads
    out = {}
    for line in r.stdout.split("\n"):
        if line.strip():
            name, mean, worst = line.split()
            out[name] = (float(mean), int(worst))
    return out


def test_placement_and_reads_cover_every_instantiation(figures):
    assert set(figures) == set(PARENT_24393EB)


@pytest.mark.parametrize("name", ["conv3_fwd", "conv3_dgrad"])
def test_stride1_reads_are_conflict_free(figures, name):
    assert figures[name] == (0.0, 0)


def test_conv2_fwd_conflicts(figures):
    mean, worst = figures["conv2_fwd"]
    assert mean <= 0.25 and worst <= 1, (mean, worst)


@pytest.mark.parametrize("name", ["conv1_fwd", "conv12_fwd.conv1", "conv12_fwd.conv2",
                                  "conv2_dgrad"])
def test_no_geometry_worse_than_parent(figures, name):
    mean, worst = figures[name]
    pmean, pworst = PARENT_24393EB[name]
    assert mean <= pmean and worst <= pworst, (mean, worst, pmean, pworst)
