"""The LDS placement of the forwards that keep x2 in LDS, checked on the host.

tests/fused_x2_geom_check.cc includes acme_amd/csrc/gemm_p3i_geom.h (no HIP dependency) and,
for conv123_fwd (conv1 -> conv2 -> conv3, one frame per block) and conv23_fwd (conv2 -> conv3,
two frames per block) at every stage depth torso.hip launches them with, checks that conv2's
epilogue sink writes every (frame, oh, ow, chunk) where ImgGeom<G3, false>::fill would place
that unit of x2, that no two live LDS regions overlap in any phase of either kernel, and that
each kernel's LDS is at most 160 KiB.  The kernels static_assert that the placement structs
checked here are the offsets they use.
"""

import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "acme_amd", "csrc")

NAMES = ("conv123_fwd", "conv123_fwd.bk32", "conv23_fwd", "conv23_fwd.bk32")


@pytest.fixture(scope="module")
def budgets(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fused_x2_geom") / "fused_x2_geom_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", exe,
                           os.path.join(HERE, "fused_x2_geom_check.cc")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stderr  # sink offsets, region overlaps, budgets
    return {line.split()[0]: int(line.split()[1]) for line in r.stdout.split("\n") if line.strip()}


def test_every_instantiation_is_checked(budgets):
    assert set(budgets) == set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_lds_budget(budgets, name):
    assert 0 < budgets[name] <= 160 * 1024, budgets[name]


def test_fusing_conv3_adds_no_lds(budgets):
    # x2 lies over the dead x1 planes: the fused kernels need what their conv2 halves need
    # (conv12_fwd 117.5 KB, conv2_fwd 158,720 B at a 64-k stage).
    assert budgets["conv123_fwd"] == 120320
    assert budgets["conv23_fwd"] == 158720
