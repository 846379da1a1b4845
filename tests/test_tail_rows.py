"""The row walk of the chain-tail kernels k_stack, k_episodes and k_obs_post (img_env_amd/csrc/tail_rows.h) on the CPU, beside
tests/test_launch_plan_actions.py: tests/host/tail_rows_check.cpp compiles the header the three kernels call and compares the
walk with a literal loop over (world in list, robot in world) -- not listed at 1, 5 and 257 rows, a list of 2 of 4 worlds with
its count on the host and in device memory, an empty count, one robot per world in reverse -- and the kernels' item mapping over
a simulated grid of 2 blocks x 256 lanes: every (row, element) pair exactly once."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tail_row_walk_and_item_mapping(tmp_path):
    exe = str(tmp_path / "tail_rows_check")
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "host", "tail_rows_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
