"""plan_obs_lds and plan_obs (img_env_amd/csrc/launch_plan.h) on the CPU: the LDS size an early k_obs asks for so that a compute
unit keeps room for the packed raster launch behind it.  tests/host/obs_room_check.cpp compiles the very header the library's
launch functions call: the size stays lds_obs where packing is refused or the step is not early, a padded size leaves the asked
number of workgroups per compute unit (wavefront slots and the rasters' LDS) and stays within the per-workgroup limit, and the
steps between sizes hold with their neighbours."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("obs_room") / "obs_room_check")
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "obs_room_check.cpp"), "-o", exe])
    return exe


def test_obs_room_sizes_thresholds_and_refusals(checker):
    out = subprocess.run([checker], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
