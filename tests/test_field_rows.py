"""What the row-copy features share (observation stacks, final observations, rollout storage, rollout minibatches, running
normalisation), on the CPU, beside tests/test_final_obs_plan.py: tests/host/field_rows_check.cpp compiles field_rows.h,
obs_fields.h and the block layouts of launch_plan.h for the host.

The walk: tables filled to their last entry (18 fields of k_final_obs, 11 of k_rollout) and tables of 1 and 2 fields, over row sizes
of 27648, 4608, 2880, 1448, 724, 20, 12, 6 and 1 bytes in every rotation; every chunk number of a row lands in the right field with
the right relative chunk, and the first one past the row stays in the last field.  The catalogue: the row sizes of the 17 fields
for a handle with every optional array and for one with none, against literals; the silent skip and the refusal of the selection.

The layouts: every offset and the total of the five blocks at RL = 4 / state_dim 3 and RL = 5 / state_dim 5 (181 beams, 48 x 48
images, stacks of depth (3, 3, 2), T = 3, F = 4, batch 4 with 2 buffers) equal literals, are multiples of 256 and leave no two
arrays overlapping.  The literals are the layout of the commit before the plans existed, DERIVED BY HAND from the arithmetic its
enable functions spelled out (each array rounded up to 256 bytes, in the order written there) -- not read back from a device.

The same program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "field_rows_check.cpp")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-Wall", "-Werror"] + flags + [SOURCE, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    return out.stdout.split()


def test_field_rows_walk_catalogue_and_layouts(tmp_path):
    words = _build_and_run(tmp_path, "field_rows_check", [])
    assert int(words[1]) > 500  # (the checks ran: the layouts alone make several hundred)


def test_field_rows_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "field_rows_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
