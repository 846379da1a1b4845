"""The launch shape of k_tracks_install (img_env_amd/csrc/launch_plan.h: plan_tracks_install) on the CPU, beside
tests/test_launch_plan_actions.py: tests/host/launch_plan_tracks_check.cpp compiles the header the library's launch functions call
and asserts the shape for zero worlds, one world, more finished worlds than the hinted grid (the stride path) and an odd
Pw * stride."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tracks_install_launch_shapes(tmp_path):
    exe = str(tmp_path / "launch_plan_tracks_check")
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "launch_plan_tracks_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
