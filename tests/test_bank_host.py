"""The host plumbing the map, track and scenario banks share (img_env_amd/csrc/bank_host.h) without a device: the (world, id) list
check and its messages, the draws a host-placed reset carries to its launches, the search for a placement's scenario epoch, and
the all-or-nothing allocation of device blocks -- whose failure paths no GPU test can reach -- over a fake device that fails at a
chosen call."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bank_host_under_the_sanitizers(tmp_path):
    """a stand-alone program with its own main (tests/host/bank_host_check.cpp): a leaked or twice-freed block of a failed
    transaction, or a read past a list, fails the run"""
    exe = str(tmp_path / "bank_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "bank_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
