"""k_view's first hits over live beams only, checked on the CPU (no GPU, no oracle): tests/host/k_view_live_beams_check.cpp
restates the one-wavefront walk of phase 3 -- chunk 0 of every beam, then later chunks only of the beams still alive, taken from
a queue compacted in place -- with the library's own tables (img_env_amd/csrc/host_tables.h) and checks that every beam gets the
key of its first occupied cell, on random crops with and without axis-parallel walls and with hits on chunk boundaries."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("klb") / "k_view_live_beams_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "k_view_live_beams_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("view_w,view_h,res,beams,a0,a1", [
    (12, 12, 0.25, 360, -1.5708, 1.5708),      # the headline geometry: 48 x 48 cells, 360 beams
    (11.25, 12.5, 0.25, 200, -3.14159, 3.14159),  # 50 x 45 cells (rows not a multiple of 4), full circle
    (6, 6, 0.125, 720, -1.5708, 1.5708),       # 48 x 48 at half the cell size, 720 beams: the queue does not fit, old walk
    (5, 7, 0.25, 33, -0.7, 2.1),               # a small odd view, few beams
    (12, 12, 0.125, 720, -1.5708, 1.5708),     # cfg-5's 96 x 96 cells, 720 beams
])
def test_live_beam_walk_finds_every_first_hit(checker, view_w, view_h, res, beams, a0, a1):
    out = subprocess.run([checker, str(view_w), str(view_h), str(res), str(beams), str(a0), str(a1), "7"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
