"""The launch shapes of k_actions and k_obs_post (img_env_amd/csrc/launch_plan.h: plan_actions_launch, plan_tail_launch) on
the CPU, beside tests/test_launch_plan.py: tests/host/launch_plan_actions_check.cpp compiles the header the library's launch
functions call and asserts the shapes at 1, 256 and 257 local robots, at a listed reset chain of 2 worlds x 3 robots, at a
device-side chain and at the block cap."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_action_and_obs_post_launch_shapes(tmp_path):
    exe = str(tmp_path / "launch_plan_actions_check")
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "launch_plan_actions_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
