"""The launch-shape rules (img_env_amd/csrc/launch_plan.h: which kernel variant runs at which grid, block and LDS size) on the
CPU: tests/host/launch_plan_check.cpp compiles the very header the library's launch functions call and feeds it the shapes
the project's documents make claims about -- the table of DESIGN.md §5, the measurement comments beside each threshold, the
docstrings of tests/test_gpu_large_launches.py ("`k_raster<.., true, 1>`, split", "32 tiles per `k_crop_big` wavefront", ...) --
and every threshold with its two neighbours.  A threshold that moves fails here; without this it would pass the GPU suite and
silently stop covering the variant a shape was chosen for."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "launch_plan_check")
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "launch_plan_check.cpp"), "-o", exe])
    return exe


def test_launch_plans_match_the_documented_shapes_and_thresholds(checker):
    out = subprocess.run([checker], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
