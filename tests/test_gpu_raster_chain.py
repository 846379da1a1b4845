"""The packed raster launch as it runs beside an early k_obs (img_env_amd/csrc/kernels.h: k_raster_pack; launch_plan.h:
plan_obs_lds) at the smallest shapes where what changed in it can go wrong: every wavefront asks at its entry for
the old cell list's first entries and the first lattice rows before it knows whether its robot has moved at all -- a robot's
list shorter than a segment, a standing robot beside moving ones, a last wavefront with empty segments, the pedestrians' blocks
behind the robots'.  IMGENV_RASTER_PACK=4 is set while each handle is created
(these handles are far below the size rule); steps go through step_begin / step_end, as in tests/test_gpu_raster_pack.py, so the
packed kernel and not k_move_raster draws them, and from the second step on the observation is the early one.

Each case: a 64 x 64 grid, an ORCA scene, the SUM layer, 12 steps.  Robot 0 never gets a velocity (its cached cell list must
survive every step), robots 1 and 2 drive into each other and freeze, the others move with v > 0.  Every output is compared
with the oracle after the reset and after every step at the parity suite's bars.  A second test runs the first shape on
handles created with IMGENV_OBS_ROOM at 0, unset (the plan's own value) and 4 (ten LDS granules per k_obs workgroup at this
shape): padding k_obs' LDS changes where its wavefronts run and nothing else, so all outputs and the robot records agree bit
for bit."""
import os
import sys

import numpy as np
import pytest

from parity import CLOSE, EXACT, compare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

RES, CELLS, STEPS = 0.25, 64, 12


def _world(params, grid, **env):
    """a handle created with these variables in the environment (the library reads its measurement switches per handle)"""
    from img_env_amd.world import World
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        w = World(params, grid)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert w.layer_mode()["layer"] == "counting"
    return w


def _scenario(n, n_peds, ped_shape, seed):
    from img_env_amd import _cabi, worldgen
    grid = worldgen.make_grid(CELLS, 0)
    params = worldgen.make_params(n, n_peds, res=RES, view_cells=48, beams=360, scene="rvoscene", ped_shape=ped_shape,
                                  flags=_cabi.FLAG_LAYER_SUM)
    layout = worldgen.make_layout(grid, RES, n, n_peds, seed=seed, clearance=0.7)
    # robots 1 and 2 face to face, half a metre apart: they collide and freeze within a step or two
    xy = layout.robot_pose[1, :2]
    layout.robot_pose[1] = worldgen.yaw_to_pose(xy[None], np.array([0.0]))[0]
    layout.robot_pose[2] = worldgen.yaw_to_pose((xy + np.array([0.5, 0.0]))[None], np.array([np.pi]))[0]
    rng = np.random.default_rng(seed + 100)
    actions = []
    for _ in range(STEPS):
        a = np.stack([rng.uniform(0.2, 0.6, n), rng.uniform(-0.9, 0.9, n), np.zeros(n)], 1).astype(np.float32)
        a[0] = 0.0  # robot 0 stands where it is
        a[1:3, 1] = 0.0  # the pair drives straight
        actions.append(a)
    return grid, params, layout, actions


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _records(w):
    import torch
    torch.cuda.synchronize(w.device)
    return w.records.cpu().numpy().copy()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("n,n_peds,ped_shape", [(9, 3, "circle"), (5, 2, "leg"), (4, 0, "circle")])
def test_packed_chain_matches_the_oracle(n, n_peds, ped_shape):
    """9 + 3 discs: the last robot wavefront has three empty segments.  5 + 2 leg-shaped pedestrians: a robot wavefront with one
    robot, both legs drawn by the blocks behind.  4 + 0: one full wavefront, no pedestrian block at all."""
    from oracle_binding import OracleWorld, build_oracle
    build_oracle()
    grid, params, layout, actions = _scenario(n, n_peds, ped_shape, seed=41)
    gpu, cpu = _world(params, grid, IMGENV_RASTER_PACK=4, IMGENV_OBS_ROOM=None), OracleWorld(params, grid)
    try:
        gpu.reset(layout)
        cpu.reset(layout)
        c = cpu.snapshot()
        bad = compare(gpu.snapshot(), c, EXACT + CLOSE)
        assert not bad, ("reset", bad)
        poses = [c["robot_pose"].copy()]
        for s, a in enumerate(actions):
            gpu.step_begin(a)
            gpu.step_end()
            cpu.step(a)
            c = cpu.snapshot()
            bad = compare(gpu.snapshot(), c, EXACT + CLOSE)
            assert not bad, ("step %d" % s, bad)
            poses.append(c["robot_pose"].copy())
    finally:
        gpu.close()
        cpu.close()
    moved = np.array([np.any(poses[s + 1] != poses[s], axis=-1) for s in range(STEPS)])
    assert not moved[:, 0].any(), "robot 0 was to stand still"
    assert moved[0, 1] and not moved[-1, 1], "robot 1 was to move, collide and freeze"
    assert moved[:, 3:].all(axis=0).any(), "no robot moved in every step"


@pytest.mark.timeout(120)
def test_obs_room_changes_no_output():
    """the first shape on three handles: IMGENV_OBS_ROOM 0, unset and 4"""
    grid, params, layout, actions = _scenario(9, 3, "circle", seed=41)
    rooms = (0, None, 4)
    ws = []
    try:
        for room in rooms:
            ws.append(_world(params, grid, IMGENV_RASTER_PACK=4, IMGENV_OBS_ROOM=room))
        for w in ws:
            w.reset(layout)
        for s, a in enumerate(actions):
            for w in ws:
                w.step_begin(a)
                w.step_end()
            base, base_rec = ws[0].snapshot(), _records(ws[0])
            for room, w in zip(rooms[1:], ws[1:]):
                snap = w.snapshot()
                diff = [k for k in base if not _same_bits(base[k], snap[k])]
                assert not diff, ("step %d" % s, "IMGENV_OBS_ROOM %s against 0" % room, diff)
                assert _same_bits(base_rec, _records(w)), ("step %d" % s, "IMGENV_OBS_ROOM %s: robot records differ" % room)
                assert w.launches() == ws[0].launches()
    finally:
        for w in ws:
            w.close()
