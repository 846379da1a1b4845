"""Scenarios in which k_view's step (5) runs out of room, and the CPU-only proof that they do.

Shared by tests/test_k_view_resolve_room.py (no GPU) and tests/test_gpu_k_view_resolve_room.py.  A case is a view geometry, a
number of robots (which picks the kernel variant: launch_plan.h plan_views) and the cap it is to overflow.  The world is a drawn
map of one-cell corridors -- every second column of the grid is a wall -- with a robot every few cells of every corridor, at the
centre of its cell, headed along the corridor, across it or anywhere; the footprints are a fifth of a cell, so standing between
two walls is no collision.  Robots headed along their corridor creep forward in the steps, a third of the others turn on the
spot, the rest stand still: nobody ever collides or arrives, so nobody is frozen.

Why a case is not vacuous is established without the GPU: a second ORACLE world on the same scenario with use_laser = 0 gives
each robot's crop as its view_maps (0 = occupied), and tests/host/k_view_resolve_room_check.cpp -- the CPU model of step (5),
built on the library's own host tables -- counts per view the chunk descriptors and result slots the step wants against
cap_d / cap_r, and replays the step with the product caps and with smaller ones against the sequential reference."""
import functools
import os
import struct
import subprocess
import tempfile

import numpy as np

from img_env_amd import worldgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STEPS = 3
FULL, HALF = (-3.14159, 3.14159), (-1.570795, 1.570795)

#: name -> view cells along / across the heading, cell size, beams, field of view, robots, the cap to overflow ("d": chunk
#: descriptors, "r": result slots), the variant plan_views picks (wavefronts per view); pitch: cells between two robots of a
#: corridor (4), margin: cells of corridor between the map's border and the first robot (2) -- the long views overflow only
#: where the shallow beams get far along the corridor before another robot or the border stops them
CASES = {
    "nw8_descriptors": dict(hv=16, wv=16, res=0.25, beams=720, fov=FULL, n=48, cap="d", nw=8),
    "nw8_slots": dict(hv=48, wv=8, res=0.25, beams=1440, fov=FULL, n=48, cap="r", nw=8, pitch=26, margin=24),
    "nw2": dict(hv=16, wv=16, res=0.25, beams=720, fov=FULL, n=1025, cap="d", nw=2),
    "nw1": dict(hv=16, wv=16, res=0.25, beams=720, fov=FULL, n=4097, cap="d", nw=1),
    "nw4_lds_bound": dict(hv=96, wv=96, res=0.25, beams=4000, fov=FULL, n=32, cap="d", nw=4, pitch=100, margin=48),
    "cells_of_0.1": dict(hv=16, wv=16, res=0.1, beams=720, fov=FULL, n=48, cap="d", nw=8),
    "rows_of_15": dict(hv=17, wv=15, res=0.25, beams=720, fov=FULL, n=48, cap="d", nw=8),
}


def geometry_args(case):
    """the checker's leading arguments: view_w view_h res beams angle_begin angle_end min_dist max_dist radius n_robots"""
    k = CASES[case]
    return [repr(k["wv"] * k["res"]), repr(k["hv"] * k["res"]), repr(k["res"]), str(k["beams"]), repr(k["fov"][0]),
            repr(k["fov"][1]), "-100.0", "100.0", repr(radius(case)), str(k["n"])]


def radius(case):
    return float(np.float32(0.2 * CASES[case]["res"]))


@functools.lru_cache(maxsize=None)
def checker():
    exe = os.path.join(tempfile.mkdtemp(prefix="kvrr"), "k_view_resolve_room_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "k_view_resolve_room_check.cpp"), "-o", exe])
    return exe


def run_checker(args):
    """(GEOM dict, rows of the S / V lines as {key: [n_skip, flagged, passing, need_d, cap_d, need_r, cap_r, alone_r]})"""
    out = subprocess.run([checker()] + list(args), capture_output=True, text=True, timeout=600)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines and lines[-1].startswith("OK"), out.stdout[-2000:] + out.stderr[-2000:]
    geom, rows = None, {}
    for ln in lines:
        f = ln.split()
        if f[0] == "GEOM":
            geom = dict(zip(("Hv", "Wv", "B", "NC", "lds_view", "lds_bound", "nw", "a4"), map(int, f[1:])))
        elif f[0] in ("S", "V"):
            rows[f[1]] = [int(x) for x in f[2:]]
    return geom, rows


def scenario(case):
    """(grid, params, layout, [actions of step 0, 1, ...]) -- deterministic"""
    k = CASES[case]
    n, res = k["n"], k["res"]
    rng = np.random.default_rng(11)
    pitch, margin = k.get("pitch", 4), k.get("margin", 2)
    size = 20
    while True:  # the smallest square map whose corridors hold the robots
        per_col, cols = (size - 18 - 2 * margin) // pitch + 1 if size - 18 - 2 * margin >= 0 else 0, (size - 18) // 2
        if per_col * cols >= n * 1.1:
            break
        size += 2
    grid = np.full((size, size), 255, np.uint8)
    grid[:8] = 0
    grid[-8:] = 0
    grid[:, :8] = 0
    grid[:, -8:] = 0
    grid[:, 8::2] = 0                            # corridors along x in the odd columns
    spots = [(8 + margin + pitch * j, 9 + 2 * c) for c in range(cols) for j in range(per_col)]
    assert len(spots) >= n, (len(spots), n)
    pick = rng.permutation(len(spots))[:n]
    cells = np.array([spots[q] for q in sorted(pick)], np.float64)
    # a quarter each: along the corridor forwards / backwards, across it, anywhere
    kind = np.arange(n) % 4
    yaw = np.where(kind == 0, 0.0, np.where(kind == 1, np.pi, np.where(kind == 2, np.pi / 2, rng.uniform(-3.1, 3.1, n))))
    pose = worldgen.yaw_to_pose(cells * res, yaw)
    layout = worldgen.ResetLayout(robot_pose=pose, robot_goal=cells * res + 1000.0, ped_pose=np.zeros((0, 4)), ped_goal=np.zeros((0, 2)),
                                  ped_traj=np.zeros((0, 2, 3)), ped_traj_len=np.zeros(0, np.int32))
    r = radius(case)
    params = worldgen.make_params(
        n, 0, res=res, beams=k["beams"], scene="", view_width=k["wv"] * res, view_height=k["hv"] * res,
        view_angle_begin=k["fov"][0], view_angle_end=k["fov"][1], view_min_dist=-100.0, view_max_dist=100.0,
        image_size=(k["wv"], k["hv"]), robot_size=np.tile(np.array([0, 0, r, 0], np.float32), (n, 1)),
        robot_size_last=np.full(n, r))
    actions = []
    for s in range(N_STEPS):
        a = np.zeros((n, 3), np.float32)
        a[kind == 0, 0] = 0.3 * res / 0.25       # (the robots headed backwards have another robot's back closer in front of them)
        turn = (kind >= 2) & (np.arange(n) % 3 == 0)
        a[turn, 1] = rng.uniform(-0.9, 0.9, int(turn.sum()))
        actions.append(a)
    return grid, params, layout, actions


@functools.lru_cache(maxsize=None)
def evidence(case):
    """What the oracle and the CPU model say about the case, pass by pass (pass 0: the reset, then the steps):
    {"geom": ..., "over": [robots over the targeted cap and not frozen, per pass], "worst": [(need, cap) per pass],
     "frozen": [robots frozen, per pass]}.
    Runs the oracle twice: with the laser (the flags that freeze a robot) and without (the crops)."""
    from oracle_binding import OracleWorld
    k = CASES[case]
    grid, params, layout, actions = scenario(case)
    n, nc = k["n"], k["hv"] * k["wv"]
    blind = dict(params, use_laser=0)
    seeing, crops = OracleWorld(params, grid), OracleWorld(blind, grid)
    occ, frozen = [], []
    try:
        for s in range(N_STEPS + 1):
            # a robot that has collided or arrived keeps its view from then on: k_view returns before it looks
            before = seeing.snapshot() if s else None
            frozen.append(np.zeros(n, bool) if s == 0 else (before["is_collisions"].reshape(n) != 0) | (before["is_arrives"].reshape(n) != 0))
            for w in (seeing, crops):
                w.reset(layout) if s == 0 else w.step(actions[s - 1])
            a, b = seeing.snapshot(), crops.snapshot()
            assert np.array_equal(a["robot_pose"], b["robot_pose"]) and np.array_equal(a["is_collisions"], b["is_collisions"])
            occ.append((b["view_maps"].reshape(n, nc) == 0).astype(np.uint8))
    finally:
        seeing.close()
        crops.close()
    with tempfile.NamedTemporaryFile(suffix=".views", delete=False) as fh:
        fh.write(struct.pack("<ii", n * (N_STEPS + 1), nc))
        fh.write(np.concatenate([np.full(n, 1 if s == 0 else 0, np.uint8) for s in range(N_STEPS + 1)]).tobytes())
        for o in occ:
            fh.write(o.tobytes())
        path = fh.name
    try:
        geom, rows = run_checker(geometry_args(case) + ["file", path])
    finally:
        os.unlink(path)
    col = (3, 4) if k["cap"] == "d" else (5, 6)
    over, worst = [], []
    for s in range(N_STEPS + 1):
        need = np.array([rows[str(s * n + i)][col[0]] for i in range(n)])
        cap = np.array([rows[str(s * n + i)][col[1]] for i in range(n)])
        live = ~frozen[s]
        over.append(int(((need > cap) & live).sum()))
        q = int(np.argmax(np.where(live, need - cap, -10 ** 9)))
        worst.append((int(need[q]), int(cap[q])))
    return dict(geom=geom, over=over, worst=worst, frozen=[int(f.sum()) for f in frozen])
