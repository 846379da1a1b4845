"""plan_raster_pack (img_env_amd/csrc/launch_plan.h: which chains draw their robots several to a wavefront, k_raster_pack) on the
CPU: tests/host/raster_pack_plan_check.cpp compiles the header the library's launch_rasters calls and pins the rule for the
headline handle, cfg-5's, a 1024- and a 4096-robot handle, every reason it refuses for, the size threshold with its two
neighbours, and plan_rasters' unchanged answer for the headline (8192 x 64, one wavefront per block, no split)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pack_plan") / "raster_pack_plan_check")
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "raster_pack_plan_check.cpp"), "-o", exe])
    return exe


def test_raster_pack_plan_rule_refusals_and_threshold(checker):
    out = subprocess.run([checker], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
