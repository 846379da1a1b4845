"""The room of k_view's step (5) -- skip list, cap_d chunk descriptors, cap_r result slots (launch_plan.h: plan_resolve_room) --
and what the step does when it runs out, on the CPU (no GPU): tests/host/k_view_resolve_room_check.cpp replays the step's
bookkeeping with the kernel's own packing for the product caps, the tiny build's (5, 2), (0, 0) and each area short on its
own, against the reference's
sequential beam-after-beam laser_map, and counts what a view wants of either area.

  * the usual geometries stay inside both caps on idealised scenes around the sensor cell (rings, walls a row / a column either
    side of it, random, checkerboard, everything occupied); small views with many beams, tall narrow views and LDS-bound views
    with thousands of beams do not -- through the public ABI, in the product build;
  * the replay holds on those scenes and on random occupancies with walls next to the sensor, for every geometry of
    tests/test_gpu_k_view_resolve_room.py;
  * the scenarios of that file overflow the cap they are meant to, by the oracle and this model alone (resolve_room_cases.py)."""
import functools

import pytest

import resolve_room_cases as rr

H, F = rr.HALF, rr.FULL
D, R = 3, 5  # columns of a row: need_d (cap_d follows), need_r (cap_r follows)


@functools.lru_cache(maxsize=None)
def scenes(view_w, view_h, res, beams, fov):
    return rr.run_checker([str(view_w), str(view_h), str(res), str(beams), repr(fov[0]), repr(fov[1]), "-100.0", "100.0", "0.17", "64",
                           "scenes", "7"])


@pytest.mark.parametrize("view_w,view_h,res,beams,fov", [
    (12, 12, 0.25, 360, H),   # 48 x 48 cells: the headline view
    (24, 24, 0.25, 960, H),   # 96 x 96 cells
    (10, 10, 0.25, 400, H),   # 40 x 40 cells
    (6, 6, 0.25, 360, H),     # 24 x 24 cells
])
def test_usual_views_stay_inside_both_caps(view_w, view_h, res, beams, fov):
    geom, rows = scenes(view_w, view_h, res, beams, fov)
    assert len(rows) == 9
    for name, r in rows.items():
        assert r[D] <= r[D + 1] and r[R] <= r[R + 1], (name, r)


@pytest.mark.parametrize("view_w,view_h,res,beams,fov,scene,over_d,over_r,pinned", [
    (6, 6, 0.25, 719, H, "row_walls", True, False, None),                   # the smallest fuzz view with the most fuzz beams
    (4, 4, 0.25, 720, F, "row_walls", True, False, (108, 23, 28, 64)),      # 16 x 16 cells
    (4, 4, 0.25, 720, F, "random30", True, False, None),
    (2, 12, 0.25, 1440, F, "col_walls", True, True, (342, 9, 84, 32)),      # 48 cells along the heading, 8 across
    (24, 24, 0.25, 4000, F, "row_walls", True, False, (1356, 1084, 207, 384)),  # LDS-bound: four wavefronts per view
])
def test_views_that_run_out_of_room(view_w, view_h, res, beams, fov, scene, over_d, over_r, pinned):
    geom, rows = scenes(view_w, view_h, res, beams, fov)
    r = rows[scene]
    assert (r[D] > r[D + 1]) == over_d and (r[R] > r[R + 1]) == over_r, r
    if pinned:
        assert tuple(r[D:D + 4]) == pinned, r


def test_lds_bound_view_takes_four_wavefronts():
    geom, _ = scenes(24, 24, 0.25, 4000, F)
    assert geom["lds_bound"] == 1 and geom["nw"] == 4
    geom, _ = scenes(12, 12, 0.25, 360, H)
    assert geom["lds_bound"] == 0 and geom["nw"] == 8


@pytest.mark.parametrize("case", sorted(rr.CASES))
def test_replay_at_the_gpu_geometries(case):
    k = rr.CASES[case]
    geom, rows = rr.run_checker(rr.geometry_args(case) + ["scenes", "3"])
    assert (geom["Hv"], geom["Wv"], geom["B"]) == (k["hv"], k["wv"], k["beams"])
    assert geom["nw"] == k["nw"], geom


@pytest.mark.parametrize("case", sorted(rr.CASES))
def test_gpu_scenarios_run_out_of_room(case):
    """the conditions under which tests/test_gpu_k_view_resolve_room.py means something, from the oracle and the model alone"""
    ev = rr.evidence(case)
    print(case, ev)
    assert ev["over"][0] >= 8 and max(ev["over"][1:]) >= 8, ev
