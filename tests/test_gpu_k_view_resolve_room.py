"""k_view's step (5) where its room runs out, in the product build: World against OracleWorld, every field at the reset and at
each of a few steps, at parity.compare's bars.

The step resolves the cells their top beam leaves alone in scratch carved out of dead LDS -- cap_d chunk descriptors, cap_r result
slots (launch_plan.h: plan_resolve_room) -- and a cell that finds no room walks its list alone.  No other test's geometry
overflows either cap; these do, once per kernel variant (8, 2, 1 and -- LDS-bound -- 4 wavefronts per view, which allocate through
LDS atomics or, alone, through scalar cursors), once through the slots, once with cells that are no power of two and once
with rows that are no multiple of four cells.  The scenarios (resolve_room_cases.py) are robots in one-cell corridors.

That a case overflows is not taken from the GPU: a second oracle world without a laser gives every robot's crop, and the CPU
model of the step (tests/host/k_view_resolve_room_check.cpp) counts what each view wants against its caps.  Each test asserts
at least 8 such robots at the reset and at least 8, not frozen, in a compared step; which variant runs comes from the launch
planner itself (plan_lds_bound, plan_views) through the same program."""
import os
import sys

import pytest

import resolve_room_cases as rr
from parity import CLOSE, EXACT, compare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(rr.CASES))
def test_views_out_of_room_match_oracle(case):
    import torch
    assert torch.cuda.is_available()
    from img_env_amd.world import World
    from oracle_binding import OracleWorld
    k = rr.CASES[case]
    ev = rr.evidence(case)
    print(case, ev)
    geom = ev["geom"]
    assert (geom["Hv"], geom["Wv"], geom["B"]) == (k["hv"], k["wv"], k["beams"])
    assert geom["nw"] == k["nw"], geom                      # the variant the launch planner picks for this many robots
    assert geom["lds_bound"] == (1 if case == "nw4_lds_bound" else 0), geom
    assert geom["a4"] == (0 if case == "rows_of_15" else 1), geom
    if case == "nw1":  # one wavefront and more beams than the live-beam queue holds: phase (3)'s plain chunk loop
        assert k["beams"] > 8 * k["wv"]
    assert ev["over"][0] >= 8 and max(ev["over"][1:]) >= 8, ev
    grid, params, layout, actions = rr.scenario(case)
    gpu, cpu = World(params, grid), OracleWorld(params, grid)
    try:
        gpu.reset(layout)
        cpu.reset(layout)
        bad = compare(gpu.snapshot(), cpu.snapshot(), EXACT + CLOSE)
        assert not bad, ("reset", bad)
        for s, a in enumerate(actions):
            gpu.step(a)
            cpu.step(a)
            bad = compare(gpu.snapshot(), cpu.snapshot(), EXACT + CLOSE)
            assert not bad, ("step %d" % s, bad)
    finally:
        gpu.close()
        cpu.close()
