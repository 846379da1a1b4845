"""The per-row rules of the episode log (img_env_amd/csrc/episode_log.h) on the CPU, beside tests/test_tail_rows.py:
tests/host/episode_log_check.cpp compiles the header k_episode_log calls, under AddressSanitizer and UBSan, and walks the covered rows
as the kernel does -- 16 wavefronts of 64 lanes, a counting pass, then chunks of 1024 rows with a ballot per wavefront and a running
base -- over 1, 63, 65, 1024, 1025 and 2500 covered rows with random open flags, listed and not, the count on the host and in device
memory, into rings of capacity 1, 7 and 4096 that are in mid-turn; against a sequential append that keeps a chain's last
``capacity`` records.  The logged figures must be what ep_fold then adds to the robot's figure sums, and every covered
row must carry the tags of the episode that starts."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunked_append_equals_the_sequential_one(tmp_path):
    exe = str(tmp_path / "episode_log_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "host", "episode_log_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
