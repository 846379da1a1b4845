"""k_raster_pack (several robots per wavefront in the SUM layer's step, img_env_amd/csrc/kernels.h) against the oracle and against
k_raster itself: three handles of one library per case -- IMGENV_RASTER_PACK=0, 2 and 4 in the environment while each is created --
take the same resets and steps.  The packed ones must match the oracle at the parity suite's bars after the reset and after every
step, and the pack-0 handle bit for bit on every output array and on the robot records (their eighth double is the footprint
bitmap).

Steps go through step_begin / step_end: imgenv_step on a handle this small leaves the move to the raster launch (k_move_raster),
which the packed kernel never replaces.  At 0.1 m cells the footprint bitmap (5 x 5) does not fit a segment of 16 lanes: the
pack-4 handle is then refused by the plan and runs k_raster, with the same results.

Uncertified poses: a disc's lattice has a pitch of 0.01 m, so a robot on multiples of `res` with heading 0 puts no sample on a
rounding boundary (0.125 m is no multiple of the pitch, and 0.1 arrives as a float32) -- tests/host/raster_pack_pose_check.cpp says
so.  The case keeps such robots and adds ones whose y puts the sample 0.05 m off the centre exactly onto a boundary; heading 0 and
no turn rate keep them there while they move."""
import os
import subprocess
import sys

import numpy as np
import pytest

from parity import CLOSE, EXACT, compare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

SWITCH = "IMGENV_RASTER_PACK"
RADIUS = 0.17


def _world(params, grid, pack):
    from img_env_amd.world import World
    old = os.environ.get(SWITCH)
    os.environ[SWITCH] = str(pack)
    try:
        w = World(params, grid)
    finally:
        if old is None:
            del os.environ[SWITCH]
        else:
            os.environ[SWITCH] = old
    assert w.layer_mode()["layer"] == "counting"
    return w


def _sum_params(n, n_peds, res, **over):
    from img_env_amd import _cabi, worldgen
    return worldgen.make_params(n, n_peds, res=res, view_cells=48, beams=360, scene="rvoscene", flags=_cabi.FLAG_LAYER_SUM, **over)


def _records(w):
    import torch
    torch.cuda.synchronize(w.device)
    return w.records.cpu().numpy().copy()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Trio:
    """pack-0, pack-2 and pack-4 handles of one parameter set"""

    def __init__(self, params, grid):
        self.w = {}
        try:
            for pack in (0, 2, 4):
                self.w[pack] = _world(params, grid, pack)
        except Exception:
            self.close()
            raise

    def reset(self, layout):
        for w in self.w.values():
            w.reset(layout)

    def step(self, a):
        for w in self.w.values():
            w.step_begin(a)
            w.step_end()

    def check(self, what, oracle_snapshot=None, fields=EXACT + CLOSE):
        """the packed handles against the oracle's snapshot and against the pack-0 handle; returns pack 0's snapshot and records"""
        base, base_rec = self.w[0].snapshot(), _records(self.w[0])
        for pack in (2, 4):
            snap, rec = self.w[pack].snapshot(), _records(self.w[pack])
            if oracle_snapshot is not None:
                bad = compare(snap, oracle_snapshot, fields)
                assert not bad, (what, "pack %d against the oracle" % pack, bad)
            diff = [k for k in base if not _same_bits(base[k], snap[k])]
            assert not diff, (what, "pack %d against pack 0" % pack, diff)
            assert _same_bits(base_rec, rec), (what, "pack %d: robot records differ from pack 0's" % pack,
                                               np.argwhere(base_rec.view(np.uint64) != rec.view(np.uint64))[:8].tolist())
            assert self.w[pack].launches() == self.w[0].launches(), (what, "imgenv_step_launches")
        if oracle_snapshot is not None:
            bad = compare(base, oracle_snapshot, fields)
            assert not bad, (what, "pack 0 against the oracle", bad)
        return base, base_rec

    def close(self):
        for w in self.w.values():
            w.close()


@pytest.fixture(scope="module")
def pose_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pack") / "raster_pack_pose_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "raster_pack_pose_check.cpp"), "-o", exe])

    def run(records, res):
        """per robot: (certified by the lattice rows, hash of the covered cells) at the pose its record holds"""
        text = "".join("%s %s %s %s\n" % (float(r[0]).hex(), float(r[1]).hex(), float(r[5]).hex(), float(r[6]).hex()) for r in records)
        out = subprocess.run([exe, repr(RADIUS), repr(res)], input=text, capture_output=True, text=True, timeout=60, check=True)
        rows = [ln.split() for ln in out.stdout.splitlines()]
        assert len(rows) == len(records)
        return np.array([r[0] == "1" for r in rows]), np.array([int(r[1]) for r in rows], np.uint64)

    return run


def _face_to_face(layout, a, b, gap=0.5):
    """robot b right in front of robot a, the two heading for each other: they collide and freeze within a step or two"""
    from img_env_amd import worldgen
    xy = layout.robot_pose[a, :2]
    layout.robot_pose[a] = worldgen.yaw_to_pose(xy[None], np.array([0.0]))[0]
    layout.robot_pose[b] = worldgen.yaw_to_pose((xy + np.array([gap, 0.0]))[None], np.array([np.pi]))[0]


def _run(params, grid, layout, actions, res, on_step=None):
    """reset + steps on the three handles and the oracle; returns the oracle's robot poses and pack 0's records per snapshot"""
    from oracle_binding import OracleWorld, build_oracle
    build_oracle()
    trio, cpu = Trio(params, grid), OracleWorld(params, grid)
    poses, recs = [], []
    try:
        trio.reset(layout)
        cpu.reset(layout)
        c = cpu.snapshot()
        _, rec = trio.check("reset", c)
        poses.append(c["robot_pose"].copy())
        recs.append(rec)
        for s, a in enumerate(actions):
            trio.step(a)
            cpu.step(a)
            c = cpu.snapshot()
            _, rec = trio.check("step %d" % s, c)
            poses.append(c["robot_pose"].copy())
            recs.append(rec)
    finally:
        trio.close()
        cpu.close()
    return poses, recs


def _moved(poses):
    """[steps, R]: the robot's pose of this snapshot differs from the one before"""
    return np.array([np.any(poses[s + 1] != poses[s], axis=-1) for s in range(len(poses) - 1)])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [7, 70])
def test_robots_that_move_freeze_and_enter_cells(n, pose_check):
    """7 and 70 robots + 5 pedestrians: the last wavefront holds 3 robots (RPW 4) and 1 (RPW 2), or 2 of 4; robots 1 and 2 run into
    each other, so a pair and a quad of neighbouring indices hold a frozen robot beside moving ones"""
    from img_env_amd import worldgen
    res, steps = 0.25, 10
    grid = worldgen.make_grid(100, 0)
    layout = worldgen.make_layout(grid, res, n, 5, seed=11, clearance=0.7)
    _face_to_face(layout, 1, 2)
    rng = np.random.default_rng(5)
    actions = [np.stack([rng.uniform(0.0, 0.6, n), rng.uniform(-0.9, 0.9, n), np.zeros(n)], 1).astype(np.float32) for _ in range(steps)]
    poses, recs = _run(_sum_params(n, 5, res), grid, layout, actions, res)
    moved = _moved(poses)
    for rpw in (2, 4):  # a wavefront-sized group of neighbouring indices with a frozen and a moving robot in one step
        mixed = [(s, g) for s in range(steps) for g in range(0, n, rpw) if moved[s, g:g + rpw].any() and not moved[s, g:g + rpw].all()]
        assert mixed, "no group of %d neighbouring robots held a frozen and a moving robot" % rpw
    cells = np.array([pose_check(r, res)[1] for r in recs])
    assert (cells[1:] != cells[:-1]).any(), "no robot changed its covered cells"
    assert (cells[1:] == cells[:-1])[moved].any(), "no robot moved within its cells"


@pytest.mark.timeout(300)
def test_turning_in_place_changes_last_samples_only(pose_check):
    """v = 0: the pose changes, the cells do not, the list's last-sample values do (the collision test of k_view reads them)"""
    from img_env_amd import worldgen
    res, n, steps = 0.25, 10, 8
    grid = worldgen.make_grid(100, 0)
    layout = worldgen.make_layout(grid, res, n, 5, seed=12, clearance=0.7)
    rng = np.random.default_rng(6)
    actions = [np.stack([np.zeros(n), rng.uniform(-0.9, 0.9, n), np.zeros(n)], 1).astype(np.float32) for _ in range(steps)]
    poses, recs = _run(_sum_params(n, 5, res), grid, layout, actions, res)
    assert _moved(poses).any()
    for s in range(steps):
        assert np.array_equal(poses[s + 1][:, :2], poses[0][:, :2])  # nobody leaves its spot
    cells = np.array([pose_check(r, res)[1] for r in recs])
    assert (cells == cells[0]).mean() > 0.5  # (a disc turning about its centre mostly keeps its cells)


def _boundary_y(y, res):
    """the y nearest to `y` that puts the lattice sample 0.05 m off the robot's centre exactly onto a rounding boundary of the cells"""
    res32 = float(np.float32(res))
    return (np.round(y / res32) + 0.5) * res32 - 0.05


@pytest.mark.timeout(300)
@pytest.mark.parametrize("res,cells", [(0.25, 100), (0.1, 200)])
def test_uncertified_poses_fall_back_inside_a_packed_wavefront(res, cells, pose_check):
    """odd robots sit on a rounding boundary (heading 0, no turn rate: they stay on it while they move) next to ordinary ones;
    robots 2, 6, ... on multiples of res with heading 0.  res = 0.1 is the non-power-of-two variant as well."""
    from img_env_amd import worldgen
    n, steps = 16, 8
    grid = worldgen.make_grid(cells, 0)
    layout = worldgen.make_layout(grid, res, n, 5, seed=13, clearance=1.0)
    res32 = float(np.float32(res))
    for i in range(n):
        x, y = layout.robot_pose[i, :2]
        if i % 2 == 1:
            layout.robot_pose[i] = (x, _boundary_y(y, res), 0.0, 1.0)
        elif i % 4 == 2:
            layout.robot_pose[i] = (np.round(x / res32) * res32, np.round(y / res32) * res32, 0.0, 1.0)
    rng = np.random.default_rng(7)
    straight = np.arange(n) % 2 == 1
    actions = [np.stack([np.full(n, 0.3), np.where(straight, 0.0, rng.uniform(-0.9, 0.9, n)), np.zeros(n)], 1).astype(np.float32)
               for _ in range(steps)]
    poses, recs = _run(_sum_params(n, 5, res), grid, layout, actions, res)
    moved = _moved(poses)
    cert = np.array([pose_check(r, res)[0] for r in recs])[1:]  # at the poses the steps' rasters saw
    assert not cert[:, straight][moved[:, straight]].any(), "a robot on a rounding boundary was certified"
    pairs = moved[:, 1::2] & ~cert[:, 1::2] & moved[:, 0::2] & cert[:, 0::2]
    assert pairs.any(), "no step drew an uncertified robot and a certified neighbour in one wavefront"
    assert cert[:, ~straight][moved[:, ~straight]].mean() > 0.9  # the neighbours are ordinary: certified


@pytest.mark.timeout(300)
def test_non_power_of_two_resolution():
    """res = 0.1: a box of 9 x 9 cells, three rounds of a 32-lane segment over it, more rows than a segment has lanes"""
    from img_env_amd import worldgen
    res, n, steps = 0.1, 9, 8
    grid = worldgen.make_grid(200, 0)
    layout = worldgen.make_layout(grid, res, n, 5, seed=14, clearance=0.7)
    _face_to_face(layout, 1, 2)
    rng = np.random.default_rng(8)
    actions = [np.stack([rng.uniform(0.0, 0.6, n), rng.uniform(-0.9, 0.9, n), np.zeros(n)], 1).astype(np.float32) for _ in range(steps)]
    poses, _ = _run(_sum_params(n, 5, res), grid, layout, actions, res)
    assert _moved(poses).any()


@pytest.mark.timeout(300)
def test_three_worlds_in_one_handle():
    """3 worlds x (3 robots + 2 pedestrians): 9 robots, so a wavefront spans two worlds' layers"""
    from img_env_amd import worldgen
    from img_env_amd.vec_env import stack_params
    from oracle_binding import OracleWorld, build_oracle
    build_oracle()
    res, W, Rw, Pw, steps = 0.25, 3, 3, 2, 8
    grid = worldgen.make_grid(100, 0)
    params = _sum_params(Rw, Pw, res)
    layouts = [worldgen.make_layout(grid, res, Rw, Pw, seed=20 + q, clearance=0.7) for q in range(W)]
    trio, cpus = Trio(stack_params(params, W), grid), [OracleWorld(params, grid) for _ in range(W)]
    rng = np.random.default_rng(9)

    def against_oracles(what):
        base, _ = trio.check(what)
        for pack, w in trio.w.items():
            snap = base if pack == 0 else w.snapshot()
            for q, cpu in enumerate(cpus):
                c = cpu.snapshot()
                rows = {k: snap[k][q * len(c[k]):(q + 1) * len(c[k])] for k in EXACT + CLOSE if k != "counters"}
                bad = compare(rows, c, tuple(rows))
                assert not bad, (what, "pack %d, world %d against its oracle" % (pack, q), bad)

    try:
        trio.reset(layouts)
        for cpu, lay in zip(cpus, layouts):
            cpu.reset(lay)
        against_oracles("reset")
        for s in range(steps):
            a = np.stack([rng.uniform(0.0, 0.6, W * Rw), rng.uniform(-0.9, 0.9, W * Rw), np.zeros(W * Rw)], 1).astype(np.float32)
            trio.step(a)
            for q, cpu in enumerate(cpus):
                cpu.step(a[q * Rw:(q + 1) * Rw])
            against_oracles("step %d" % s)
    finally:
        trio.close()
        for cpu in cpus:
            cpu.close()


@pytest.mark.timeout(300)
def test_two_robot_classes_keep_k_raster():
    """an ineligible handle (the packed kernel reads ONE class record): the switch is set, k_raster runs, nothing changes"""
    from img_env_amd import worldgen
    res, n, steps = 0.25, 8, 6
    grid = worldgen.make_grid(100, 0)
    layout = worldgen.make_layout(grid, res, n, 5, seed=15, clearance=0.9)
    radius = np.where(np.arange(n) % 2 == 0, RADIUS, 0.2)
    params = _sum_params(n, 5, res, robot_size=np.stack([np.zeros(n), np.zeros(n), radius, np.zeros(n)], 1).astype(np.float32),
                         robot_size_last=radius.copy())
    rng = np.random.default_rng(10)
    actions = [np.stack([rng.uniform(0.0, 0.6, n), rng.uniform(-0.9, 0.9, n), np.zeros(n)], 1).astype(np.float32) for _ in range(steps)]
    poses, _ = _run(params, grid, layout, actions, res)
    assert _moved(poses).any()


@pytest.mark.timeout(300)
def test_reset_steps_reset_steps_on_one_handle():
    """the reset chain's k_raster and the packed steps hand fp_n / fp_cells / the cached poses to each other, twice"""
    from img_env_amd import worldgen
    from oracle_binding import OracleWorld, build_oracle
    build_oracle()
    res, n, steps = 0.25, 11, 4
    grid = worldgen.make_grid(100, 0)
    params = _sum_params(n, 5, res)
    trio, cpu = Trio(params, grid), OracleWorld(params, grid)
    rng = np.random.default_rng(11)
    try:
        for episode in range(2):
            layout = worldgen.make_layout(grid, res, n, 5, seed=30 + episode, clearance=0.7)
            trio.reset(layout)
            cpu.reset(layout)
            trio.check("reset %d" % episode, cpu.snapshot())
            for s in range(steps):
                a = np.stack([rng.uniform(0.0, 0.6, n), rng.uniform(-0.9, 0.9, n), np.zeros(n)], 1).astype(np.float32)
                trio.step(a)
                cpu.step(a)
                trio.check("episode %d step %d" % (episode, s), cpu.snapshot())
    finally:
        trio.close()
        cpu.close()
