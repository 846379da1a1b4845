"""k_final_obs (img_env_amd/csrc/final_obs.h) on the CPU, beside tests/test_tail_rows.py: tests/host/final_obs_check.cpp compiles
the field-table planning of launch_plan.h and the kernel's loop body for the host and runs the body over a simulated grid -- row
sizes of 12, 20, 60, 88, 1448, 2880, 4608 and 27648 bytes, a one-byte field, a stack row of depth 3 and a 6-byte row; worlds 0
and 2 of 3 listed with two robots each, every local row, and a device-side count below (and above) the grid's guess.  Every byte
of a covered row is copied exactly once, no byte of another row is touched, final_count rises by one on covered rows only.
The same program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own."""
import os
import subprocess

from img_env_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "final_obs_check.cpp")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-Wall", "-Werror"] + flags + [SOURCE, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    return out.stdout.split()


def test_final_obs_plan_and_chunk_walk(tmp_path):
    words = _build_and_run(tmp_path, "final_obs_check", [])
    # the launch constants Python mirrors (tests/test_gpu_final_obs.py sizes its grid-stride case by them)
    consts = dict(zip(words[3::2], (int(w) for w in words[4::2])))
    assert consts["FINAL_BLOCK"] == _cabi.FINAL_BLOCK and consts["FINAL_MAX_BLOCKS"] == _cabi.FINAL_MAX_BLOCKS
    assert consts["FINAL_MAX_FIELDS"] >= len(_cabi.FINAL_ARRAYS) - 1  # every pointer of the out struct but final_count is a field


def test_final_obs_chunk_walk_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "final_obs_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
