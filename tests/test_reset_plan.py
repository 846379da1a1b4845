"""What a host-side reset decides and computes without a device, on the CPU: tests/host/reset_plan_check.cpp compiles reset_plan.h
(and through it host_tables.h, sfm.h and tfm.h) for the host.

Every refusal of the reset path for a bad batch at list position 1, text for text, the three that used to fire in the middle of
staging included (footprint, pedscene obstacle count, RVO capacity after the device-side reset); obstacle instances (lattice bounds of
circles and rectangles, reversed and oversized footprints), the polygon's vertex order from the one shared function, robot rows with
the 3-4-5 rotation and a shard, pedestrian rows re-strided and zero-padded, traj_v's atan2, bank-fed worlds, the waypoint deque cut
at SFM_MAX_WP, the growth decided once per call with pairwise disjoint slice destinations, and the placement pool's sizes and
refusals -- against literals DERIVED BY HAND, not printed from the code.

The same program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "reset_plan_check.cpp")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    # (host_tables.h keeps its table builders static, this program calls only a few; fp_rows.h carries a device-side unroll pragma)
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas", "-ffp-contract=off"] + flags + [SOURCE, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    return out.stdout.split()


def test_reset_plan_refusals_rows_growth(tmp_path):
    words = _build_and_run(tmp_path, "reset_plan_check", [])
    assert int(words[1]) > 100  # (the checks ran: the refusals alone make over 40)


def test_reset_plan_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "reset_plan_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
