"""The map bank (include/imgenv.h, "map bank"): several static maps in ONE handle, one of them per world and episode, chosen by
the host (imgenv_world_maps_set) or drawn with the placement inside the device-side reset chain (IMGENV_MAPS_BY_PLACEMENT).

The checker is the one of tests/test_gpu_multiworld.py -- one oracle per world, its fields and bars (PER_ROBOT, EXACT / CLOSE of
tests/parity.py), compared after the reset and after EVERY step -- with every oracle built on ITS world's map
(``worldgen.make_grid(size, seed)``, one seed per map).

A world that changes map gets a fresh oracle on the new grid at that reset.  What a reset does not restart lives on in the
library as it does in a node of the reference -- the crowd's velocities (rvoscene.h:32-34 sets positions only; ``ped_state``
shows them right after the reset) -- so the fresh oracle is first fed the world's own history (its resets and actions) on the
new grid and then the reset.  The cases that change maps run crowds that ignore the robots (relation_ped_robo 0) or no crowd at
all: the crowd's motion then depends on the placements alone, not on the map, and the replay leaves the fresh oracle's crowd
exactly where the library's is.  The beep lottery stays out of these cases (a fresh oracle restarts its rand() stream).

The issue also asks for the curriculum case once under IMGENV_GRAPH=1 "at a robot count that really takes the captured path":
this tree has no captured path any more (the hipGraph replay of the reset chain was removed, docs/HISTORY.md), so there is nothing
such a case could exercise and none is written."""
import copy
import json
import os

import numpy as np
import pytest

from parity import compare
from scenarios import random_actions
from stack_model import StackModel, bits, depths
from test_gpu_multiworld import PER_ROBOT, _stack_params, _world_slice

pytestmark = pytest.mark.gpu

VEC_FIELDS = ("is_collisions", "is_arrives", "view_maps", "sensor_maps", "vector_states", "lasers", "ped_maps",
              "ped_vector_states", "rewards", "dones", "dones_info", "robot_pose")  # the checker of tests/test_gpu_envs.py's vec envs


@pytest.fixture(scope="module")
def worlds():
    import torch
    assert torch.cuda.is_available()
    from img_env_amd.world import World
    from oracle_binding import OracleWorld, build_oracle
    build_oracle()
    return World, OracleWorld


class MovingOracle:
    """one world's oracle, which can move to another map: a fresh OracleWorld on the new grid, fed the world's history"""

    def __init__(self, OracleWorld, params, grid):
        self.make, self.params, self.history = OracleWorld, params, []
        self.cpu = OracleWorld(params, grid)

    def reset(self, layout):
        self.history.append(("reset", layout))
        self.cpu.reset(layout)

    def step(self, actions):
        self.history.append(("step", np.array(actions, np.float32)))
        self.cpu.step(actions)

    def move_to(self, grid, replay=True):
        self.cpu.close()
        self.cpu = self.make(self.params, grid)
        for what, arg in (self.history if replay else ()):
            (self.cpu.reset if what == "reset" else self.cpu.step)(arg)

    def snapshot(self):
        return self.cpu.snapshot()

    def close(self):
        self.cpu.close()


def _grids(n_maps, size, seed):
    from img_env_amd import worldgen
    grids = [worldgen.make_grid(size, seed + 17 * m) for m in range(n_maps)]
    for a in range(n_maps):
        for b in range(a):
            assert (grids[a] != grids[b]).sum() > size  # different maps, really
    return grids


def _compare_all(gpu, cpus, Rw, Pw, where, fails):
    snap = gpu.snapshot()
    for k, cpu in enumerate(cpus):
        bad = compare(_world_slice(snap, k, Rw, Pw), cpu.snapshot(), PER_ROBOT + (("ped_state",) if Pw else ()))
        if bad:
            fails.append((where, k, bad))


def _run(World, OracleWorld, W, Rw, Pw, steps, resets, seed, n_maps, start, moves=None, whole=(), replay=True, grid_size=200,
         res=0.125, n_obstacles=2, clearance=1.0, **kw):
    """``start[k]``: the map world k is put on before the first reset; ``moves``: {step: [(world, map)]} told to the library after
    that step; ``resets``: {step: [worlds reset after that step]} (one world: imgenv_reset_world, several: imgenv_reset_worlds);
    ``whole``: steps after which the whole handle is reset by one imgenv_reset (world 0's obstacles everywhere).  Returns the
    failures and how many resets changed a world's map."""
    from img_env_amd import worldgen
    grids = _grids(n_maps, grid_size, seed)
    params = worldgen.make_params(Rw, Pw, res=res, **kw)
    n_lay = [0]

    def layout(k, m):  # a placement for world k on map m: clear of that map's walls
        n_lay[0] += 1
        return worldgen.make_layout(grids[m], res, Rw, Pw, seed=seed + 1000 * n_lay[0] + k, n_obstacles=n_obstacles, clearance=clearance)

    gpu = World(_stack_params(params, W), grids)
    cur, nxt = list(start), list(start)
    cpus = [MovingOracle(OracleWorld, params, grids[start[k]]) for k in range(W)]
    fails, changed = [], 0

    def apply_reset(ks, lays):
        nonlocal changed
        for k, lay in zip(ks, lays):
            if nxt[k] != cur[k]:
                cpus[k].move_to(grids[nxt[k]], replay)
                cur[k] = nxt[k]
                changed += 1
            cpus[k].reset(lay)

    try:
        assert gpu.n_maps == n_maps and gpu.world_maps().tolist() == [0] * W  # every world starts on map 0
        gpu.set_world_maps(range(W), start)
        assert gpu.world_maps().tolist() == [0] * W  # ... and stays there until it is reset
        lays = [layout(k, start[k]) for k in range(W)]
        gpu.reset(lays)
        for k in range(W):
            cpus[k].reset(lays[k])
        assert gpu.world_maps().tolist() == cur
        _compare_all(gpu, cpus, Rw, Pw, -1, fails)
        rng = np.random.default_rng(seed + 7)
        for s in range(steps):
            a = random_actions(rng, W * Rw)
            gpu.step(a)
            for k, cpu in enumerate(cpus):
                cpu.step(a[k * Rw:(k + 1) * Rw])
            _compare_all(gpu, cpus, Rw, Pw, s, fails)
            for k, m in (moves or {}).get(s, ()):
                gpu.set_world_maps([k], [m])
                nxt[k] = m
            assert gpu.world_maps().tolist() == cur, s  # a selection does not touch the running episode
            ks = list(resets.get(s, ()))
            if ks:
                lays = [layout(k, nxt[k]) for k in ks]
                if len(ks) == 1:
                    gpu.reset_world(ks[0], lays[0])
                else:
                    gpu.reset_worlds(ks, lays)
                apply_reset(ks, lays)
                assert gpu.world_maps().tolist() == cur, s
                _compare_all(gpu, cpus, Rw, Pw, (s, "reset", tuple(ks)), fails)
            if s in whole:  # one batch of every robot / pedestrian, world 0's obstacles in every world
                lays = [layout(k, nxt[k]) for k in range(W)]
                for lay in lays[1:]:
                    lay.obs_shape, lay.obs_size, lay.obs_pose = lays[0].obs_shape, lays[0].obs_size, lays[0].obs_pose
                b = [lay.as_batch() for lay in lays]
                big = dict(b[0])
                for f in ("robot_pose", "robot_goal", "ped_pose", "ped_goal", "ped_traj", "ped_traj_len"):
                    big[f] = np.concatenate([x[f] for x in b], axis=0)
                gpu.reset(big)
                apply_reset(range(W), lays)
                assert gpu.world_maps().tolist() == cur, s
                _compare_all(gpu, cpus, Rw, Pw, (s, "whole reset"), fails)
            if len(fails) > 4:
                break
        return fails, changed
    finally:
        gpu.close()
        for c in cpus:
            c.close()


# ---- 1. different maps side by side ----
@pytest.mark.parametrize("flags", [0, 2, 4, 512], ids=["default_layer", "composed_layer", "stamped_layer", "counting_layer"])
def test_worlds_on_different_maps_match_one_oracle_each(worlds, flags):
    """4 worlds x (5 robots, 6 ORCA pedestrians, own obstacles) on 4 different maps, selected before the first reset; per-world
    resets in mid-flight (alone, in pairs, all at once) and per-world time limits, in every mode of the class layer"""
    World, OracleWorld = worlds
    fails, _ = _run(World, OracleWorld, 4, 5, 6, 24, {6: [1], 9: [1, 3], 14: [0, 2], 18: [0, 1, 2, 3]}, seed=31, n_maps=4,
                    start=[0, 1, 2, 3], n_obstacles=3, time_max=12, flags=flags)
    assert not fails, fails[:3]


def test_the_maps_of_the_bank_really_differ_in_what_the_robots_see(worlds):
    """the yardstick of the cases above: the same placement on map 0 gives other views than on the world's own map, so a library
    that ignored the selection would not pass them"""
    World, OracleWorld = worlds
    from img_env_amd import worldgen
    grids = _grids(4, 200, 31)
    params = worldgen.make_params(5, 6)
    differ = 0
    for m in range(1, 4):
        lay = worldgen.make_layout(grids[m], 0.125, 5, 6, seed=31 + m, n_obstacles=3)
        a, b = OracleWorld(params, grids[m]), OracleWorld(params, grids[0])
        try:
            a.reset(lay)
            b.reset(lay)
            differ += int(not np.array_equal(a.snapshot()["view_maps"], b.snapshot()["view_maps"]))
        finally:
            a.close()
            b.close()
    assert differ >= 2


def test_pedestrian_free_worlds_on_different_maps(worlds):
    """12 worlds x 7 robots, no pedestrians, 3 maps spread k % 3: the move inside the raster launch (k_move_raster)"""
    World, OracleWorld = worlds
    W = 12
    fails, _ = _run(World, OracleWorld, W, 7, 0, 10, {3: [11, 0, 5], 4: [5], 6: list(range(W))}, seed=33, n_maps=3,
                    start=[k % 3 for k in range(W)], n_obstacles=2, grid_size=120)
    assert not fails, fails[:3]


@pytest.mark.parametrize("relation", [1, 0])
def test_pedscene_worlds_on_different_maps(worlds, relation):
    """a social-force crowd per world, 3 worlds on 3 maps, per-world resets in mid-flight"""
    World, OracleWorld = worlds
    fails, _ = _run(World, OracleWorld, 3, 2, 7, 14, {4: [1], 9: [0, 2], 10: [1]}, seed=71, n_maps=3, start=[2, 0, 1],
                    scene="pedscene", grid_size=88, n_obstacles=3, relation_ped_robo=relation)
    assert not fails, fails[:3]


# ---- 2. a world changes its map at a reset ----
@pytest.mark.parametrize("how,flags", [("reset_world", 0), ("reset_worlds", 0), ("reset_worlds", 2), ("reset_worlds", 4),
                                       ("reset_worlds", 512), ("reset", 0), ("reset", 512)])
def test_a_world_moves_to_another_map_at_its_next_reset(worlds, how, flags):
    """world 1 is told at step 3 to move to map 2; it keeps matching the oracle of its old map until its reset after step 8 and
    the oracle of the new map from that reset on (and moves back to map 0 later); worlds 0 and 2 never deviate.  Through
    imgenv_reset_world, imgenv_reset_worlds with a second world that keeps its map, and a whole-handle imgenv_reset."""
    World, OracleWorld = worlds
    resets = {"reset_world": {8: [1], 15: [1]}, "reset_worlds": {8: [1, 2], 15: [0, 1]}, "reset": {}}[how]
    whole = (8, 15) if how == "reset" else ()
    fails, changed = _run(World, OracleWorld, 3, 4, 5, 22, resets, seed=41, n_maps=3, start=[0, 1, 0], moves={3: [(1, 2)], 11: [(1, 0)]},
                          whole=whole, n_obstacles=3, time_max=30, relation_ped_robo=0, flags=flags)
    assert not fails, fails[:3]
    assert changed == 2


def test_a_world_without_a_crowd_moves_between_maps(worlds):
    """no pedestrians: nothing of a world outlives its reset, the fresh oracle on the new map needs no history (robots are crowd
    members by configuration, relation_ped_robo 1, the k_move_raster path)"""
    World, OracleWorld = worlds
    fails, changed = _run(World, OracleWorld, 5, 6, 0, 16, {5: [1, 4], 9: [3], 12: [0, 1, 2, 3, 4]}, seed=43, n_maps=4, start=[0, 1, 2, 3, 0],
                          moves={1: [(1, 3), (4, 2)], 7: [(3, 0)], 10: [(0, 1), (2, 1)]}, replay=False, n_obstacles=2, grid_size=120)
    assert not fails, fails[:3]
    assert changed == 5


# ---- 3. the map curriculum: maps drawn with the placements ----
def _pick_seed(E, n_maps, rounds, device):
    """a seed for which resets that keep the map AND resets that change it are expected -- the draw evaluated on the CPU
    beforehand, with every env running into the time limit (the k-th reset of the run takes the k-th placement)"""
    from img_env_amd import _cabi
    for seed in range(9, 40):
        host0 = (0x9E3779B97F4A7C15 * (1 + seed)) & 0xFFFFFFFFFFFFFFFF  # VecImageEnv._spawn_seed
        base = (host0 + (1 << 63)) & 0xFFFFFFFFFFFFFFFF if device else host0 + E
        cur = [_cabi.map_for_placement(host0 + k, n_maps) for k in range(E)]
        kept = changed = 0
        for q in range(rounds * E):
            m = _cabi.map_for_placement(base + q, n_maps)
            kept += m == cur[q % E]
            changed += m != cur[q % E]
            cur[q % E] = m
        if kept >= 2 and changed >= 2:
            return seed
    raise AssertionError("no seed")


def _curriculum(cfg, grids, E, R, P, n_obs, seed, device, steps, fields=VEC_FIELDS, host_reset_at=2):
    """VecImageEnv(map_policy="placement") over ``grids``: one oracle per env, fed the placement the env really received and moved
    to the map the draw names for that placement; after every step ``world_maps`` must say the same.  Returns (resets that kept
    the map, resets that changed it)."""
    import torch
    from img_env_amd import _cabi, spawn
    from img_env_amd.vec_env import VecImageEnv
    from oracle_binding import OracleWorld
    n_maps = len(grids)
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=seed, native_spawn=True, device_reset=device, map_policy="placement")
    assert vec.n_maps == n_maps and vec.grid.shape[0] == n_maps
    cpus = [MovingOracle(OracleWorld, vec.params, vec.grid[0]) for _ in range(E)]
    cur = [0] * E
    count = {"kept": 0, "changed": 0}

    def start(k, lay, placement_seed, first=False):
        m = _cabi.map_for_placement(placement_seed, n_maps)
        if m != cur[k]:
            cpus[k].move_to(vec.grid[m])
            cur[k] = m
        if not first:
            count["kept" if m == maps_before[k] else "changed"] += 1
        cpus[k].reset(lay)

    def check(where):
        assert vec.world_maps().tolist() == cur, where
        snap = vec.world.snapshot()
        for k, c in enumerate(cpus):
            mine = {f: snap[f][k * R:(k + 1) * R] for f in fields}
            bad = compare(mine, c.snapshot(), fields)
            assert not bad, (where, k, cur[k], bad)

    try:
        seed0, dev0 = vec._spawn_seed, vec._device_seed0
        maps_before = list(cur)
        vec.reset()  # the first episodes: imgenv_reset_worlds_spawn, world k from seed0 + k -- which draws its map too
        for k in range(E):
            start(k, spawn.native_spawn(cfg, seed0 + k), seed0 + k, first=True)
        n_eps = E
        assert len(set(cur)) > 1
        check("reset")
        rng = np.random.default_rng(2)
        expect_serial = 0
        for s in range(steps):
            a = np.zeros((E * R, 3), np.float32)
            a[:, 0], a[:, 1] = rng.uniform(0, 0.6, E * R), rng.uniform(-0.9, 0.9, E * R)
            maps_before = list(cur)
            _, rew, done, info = vec.step(torch.as_tensor(a, device="cuda"))
            if device:
                finished, first = vec.world.autoreset_last()
                assert first == expect_serial, s
            else:
                finished = list(info["reset_envs"])
            rew, done = rew.cpu().numpy(), done.cpu().numpy()
            for k, c in enumerate(cpus):
                c.step(a[k * R:(k + 1) * R])
                ref = c.snapshot()  # what the step itself returned, also for the envs the library has already reset
                assert np.array_equal(rew[k * R:(k + 1) * R], ref["rewards"]), (s, k)
                assert np.array_equal(done[k * R:(k + 1) * R], ref["dones"]), (s, k)
            for q, k in enumerate(finished):
                if device:  # the placement the device drew, and its number: the map is the draw for seed0 + number
                    lay, serial = vec.world.world_placement(k, n_obs)
                    assert serial == first + q, (s, k)
                    lay.ignore_obstacle = bool(cfg["ped_sim"].get("ignore_obstacle", False))
                    start(k, lay, dev0 + serial)
                else:
                    start(k, spawn.native_spawn(cfg, seed0 + n_eps + q), seed0 + n_eps + q)
            if device:
                expect_serial += len(finished)
            else:
                n_eps += len(finished)
            check(s)
            if s == host_reset_at:  # a reset by the host in between (imgenv_reset_worlds_spawn draws the map from its seed as well)
                ep = vec._episodes
                maps_before = list(cur)
                vec.reset_envs([1])
                start(1, spawn.native_spawn(cfg, seed0 + ep), seed0 + ep)
                if not device:
                    n_eps += 1
                check("host reset")
        return count["kept"], count["changed"]
    finally:
        vec.close()
        for c in cpus:
            c.close()


@pytest.mark.parametrize("E,R,P", [(5, 3, 4), (6, 1, 0), (70, 2, 3)])
@pytest.mark.parametrize("device", [True, False], ids=["device_side_reset", "host_placed_reset"])
def test_vec_env_draws_the_map_with_the_placement(E, R, P, device):
    """``VecImageEnv(device_reset=True, map_policy="placement")`` over 3 maps, time_max 5: the finished envs are placed, given their
    map and reset by kernels alone -- the map is the draw for the placement's seed, made inside k_respawn; an env whose draw names
    the map it is on takes the sparse map restore (its old obstacles' cells), one that changes the full one: both must occur.
    The same through the host-placed imgenv_step_autoreset."""
    from img_env_amd import worldgen
    from oracle_binding import build_oracle
    build_oracle()
    grids = _grids(3, 200, 3)
    n_obs = 3
    seed = _pick_seed(E, 3, 3, device)
    cfg = worldgen.make_yaml_cfg(R, P, grids[0], time_max=5, n_obstacles=n_obs, seed=seed, relation_ped_robo=0)
    cfg["global_map"]["map_array"] = np.stack(grids)
    kept, changed = _curriculum(cfg, grids, E, R, P, n_obs, seed, device, steps=16)
    assert kept > 0 and changed > 0, (kept, changed)
    assert kept + changed >= 2 * E


# ---- 4. the shipped geometry: load-time resize, tiled big-view kernels, crop images ----
def test_two_maps_at_the_shipped_geometry_with_device_side_map_changes(tmp_path):
    """the shipped test.yaml cast and geometry (110 x 110 pixel PNGs at 0.1 m resized to 733 x 733 cells of 0.015 m, 400 x 400 cell
    views shrunk to 48 x 48, IMGENV_FLAG_NO_VIEW_MAPS) over two map FILES: both go through the load-time resize, each has its own
    image for the tiled crop kernel, and the device-side reset swaps a world's grid, class layer and crop image when the draw
    moves it.  One oracle per env; the crowd ignores the robots (see the module's docstring)."""
    from PIL import Image
    from img_env_amd import worldgen
    from oracle_binding import build_oracle
    build_oracle()
    names = []
    for k in range(2):
        m = np.full((110, 110), 255, np.uint8)
        m[:5] = m[-5:] = 0
        m[:, :5] = m[:, -5:] = 0
        if k:  # the second room has pillars and a wall stub
            m[30:36, 30:36] = m[70:78, 60:66] = m[50:53, 20:45] = 0
            m[20:24, 70:90] = 0
        names.append("room%d.png" % k)
        Image.fromarray(m).save(str(tmp_path / names[-1]))
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "spawn_ref.npz"))
    cfg = worldgen.shipped_test_yaml_cfg(names, json.loads(str(z["test@1/cfg"])))
    cfg.update(map_dir=str(tmp_path), time_max=4, relation_ped_robo=0)
    E, R, P = 7, 1, int(cfg["ped_sim"]["total"])
    seed = _pick_seed(E, 2, 3, True)
    cfg["seed"] = seed
    from img_env_amd import config
    grids = list(config.load_map(cfg))
    assert len(grids) == 2 and grids[0].shape == (110, 110)
    fields = tuple(f for f in VEC_FIELDS if f != "view_maps")
    kept, changed = _curriculum(cfg, grids, E, R, P, int(cfg["object"]["total"]), seed, True, steps=14, fields=fields, host_reset_at=5)
    assert kept > 0 and changed > 0, (kept, changed)


# ---- 5. an unused bank is invisible ----
def _bytes_equal(a, b, where):
    assert a.keys() == b.keys()
    for f in a:
        assert a[f].tobytes() == b[f].tobytes(), (where, f)


@pytest.mark.parametrize("flags", [0, 2, 4, 512], ids=["default_layer", "composed_layer", "stamped_layer", "counting_layer"])
def test_an_unused_bank_changes_no_byte_and_no_launch(worlds, flags):
    """3 maps added, policy KEEP, every world on map 0: every output byte after every reset and step, and the launch count of
    every step, are those of a handle without a bank"""
    World, _ = worlds
    from img_env_amd import worldgen
    W, Rw, Pw = 3, 5, 6
    grids = _grids(4, 200, 51)
    params = worldgen.make_params(Rw, Pw, flags=flags, time_max=12)
    lays = [worldgen.make_layout(grids[0], 0.125, Rw, Pw, seed=51 + k, n_obstacles=3) for k in range(W + 2)]
    plain, bank = World(_stack_params(params, W), grids[0]), World(_stack_params(params, W), grids)
    try:
        assert (plain.n_maps, bank.n_maps) == (1, 4)
        bank.set_maps_policy("keep")
        for w in (plain, bank):
            w.reset(lays[:W])
        _bytes_equal(plain.snapshot(), bank.snapshot(), "reset")
        rng = np.random.default_rng(5)
        for s in range(20):
            a = random_actions(rng, W * Rw)
            for w in (plain, bank):
                w.step(a)
            assert plain.launches() == bank.launches(), s
            _bytes_equal(plain.snapshot(), bank.snapshot(), s)
            if s in (6, 11):
                for w in (plain, bank):
                    w.reset_world(1, lays[W]) if s == 6 else w.reset_worlds([0, 2], lays[W:W + 2])
                _bytes_equal(plain.snapshot(), bank.snapshot(), (s, "reset"))
        assert bank.world_maps().tolist() == [0] * W and plain.world_maps().tolist() == [0] * W
    finally:
        plain.close()
        bank.close()


def test_an_unused_bank_is_invisible_to_the_device_side_reset():
    """the same through VecImageEnv(device_reset=True): 3 maps, every env on map 0, policy keep"""
    import torch
    from img_env_amd import worldgen
    from img_env_amd.vec_env import VecImageEnv
    E, R, P = 6, 2, 3
    grids = _grids(3, 200, 3)
    cfg = worldgen.make_yaml_cfg(R, P, grids[0], time_max=5, n_obstacles=3, seed=9)
    cfg_bank = copy.deepcopy(cfg)
    cfg_bank["global_map"]["map_array"] = np.stack(grids)
    plain = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True)
    bank = VecImageEnv(cfg_bank, env_num=E, seed=9, device_reset=True, world_maps=[0] * E)
    try:
        for v in (plain, bank):
            v.reset()
        _bytes_equal(plain.world.snapshot(), bank.world.snapshot(), "reset")
        rng = np.random.default_rng(2)
        resets = 0
        for s in range(14):
            a = np.zeros((E * R, 3), np.float32)
            a[:, 0], a[:, 1] = rng.uniform(0, 0.6, E * R), rng.uniform(-0.9, 0.9, E * R)
            for v in (plain, bank):
                v.step(torch.as_tensor(a, device="cuda"))
            assert plain.world.launches() == bank.world.launches(), s
            resets += len(bank.world.autoreset_last()[0])
            _bytes_equal(plain.world.snapshot(), bank.world.snapshot(), s)
        assert resets >= 2 * E and bank.world_maps().tolist() == [0] * E
    finally:
        plain.close()
        bank.close()


def test_vec_env_spreads_its_envs_over_the_maps_by_default():
    """several maps and ``world_maps=None``: env k starts on map k % n_maps and, policy keep, stays there through its device-side
    resets; one oracle per env on its map"""
    import torch
    from img_env_amd import spawn, worldgen
    from img_env_amd.vec_env import VecImageEnv
    from oracle_binding import OracleWorld, build_oracle
    build_oracle()
    E, R, P, n_obs = 7, 2, 3, 3
    grids = _grids(3, 200, 3)
    cfg = worldgen.make_yaml_cfg(R, P, grids[0], time_max=5, n_obstacles=n_obs, seed=9)
    cfg["global_map"]["map_array"] = np.stack(grids)
    with pytest.raises(ValueError, match="native_spawn"):
        VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, map_policy="placement")
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True)
    cpus = [OracleWorld(vec.params, grids[k % 3]) for k in range(E)]
    try:
        vec.reset()
        for k in range(E):
            cpus[k].reset(spawn.native_spawn(cfg, vec._spawn_seed + k))
        rng = np.random.default_rng(2)
        resets = 0
        for s in range(12):
            a = np.zeros((E * R, 3), np.float32)
            a[:, 0], a[:, 1] = rng.uniform(0, 0.6, E * R), rng.uniform(-0.9, 0.9, E * R)
            vec.step(torch.as_tensor(a, device="cuda"))
            finished, _ = vec.world.autoreset_last()
            for k, c in enumerate(cpus):
                c.step(a[k * R:(k + 1) * R])
            for k in finished:
                lay, _ = vec.world.world_placement(k, n_obs)
                cpus[k].reset(lay)
            resets += len(finished)
            assert vec.world_maps().tolist() == [k % 3 for k in range(E)], s
            snap = vec.world.snapshot()
            for k, c in enumerate(cpus):
                bad = compare({f: snap[f][k * R:(k + 1) * R] for f in VEC_FIELDS}, c.snapshot(), VEC_FIELDS)
                assert not bad, (s, k, bad)
        assert resets >= E
    finally:
        vec.close()
        for c in cpus:
            c.close()


def test_single_env_set_map_applies_at_the_next_reset():
    """``make_env`` with a list of maps: the one world runs on map 0, ``env.set_map(i)`` applies at the next ``reset()``"""
    from img_env_amd import worldgen
    from img_env_amd.envs import ImageEnv
    grids = _grids(2, 200, 3)
    cfg = worldgen.make_yaml_cfg(2, 3, grids[0], time_max=20, n_obstacles=2, seed=4)
    cfg["global_map"]["map_array"] = list(grids)
    env = ImageEnv(cfg)
    try:
        env.reset()
        assert env.world.world_maps().tolist() == [0]
        env.set_map(1)
        env.step(np.zeros((2, 3), np.float32))
        assert env.world.world_maps().tolist() == [0]
        env.reset()
        assert env.world.world_maps().tolist() == [1]
        with pytest.raises(ValueError, match="out of range"):
            env.set_map(2)
    finally:
        env.close()


# ---- 6. stacks ----
def test_stacks_are_zero_padded_after_a_map_changing_reset():
    """``stack=True`` with the device-side curriculum: a world's stacks restart ([0, ..., 0, F], tests/stack_model.py) at a reset
    that changes its map exactly as at any reset"""
    import torch
    from img_env_amd import _cabi, worldgen
    from img_env_amd.vec_env import VecImageEnv
    E, R, P = 5, 3, 4
    grids = _grids(3, 200, 3)
    seed = _pick_seed(E, 3, 3, True)
    cfg = worldgen.make_yaml_cfg(R, P, grids[0], time_max=5, n_obstacles=3, seed=seed, image_batch=3, state_batch=2, laser_batch=2)
    cfg["global_map"]["map_array"] = np.stack(grids)
    kd = dict(zip(("sensor_maps", "vector_states", "lasers"), depths(3, 2, 2)))
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=seed, device_reset=True, stack=True, map_policy="placement")
    try:
        models = {f: StackModel(kd[f]) for f in vec.world.stack}
        assert set(models) == set(kd)

        def check(where):
            torch.cuda.synchronize()
            for f, m in models.items():
                got = vec.world.stack[f].cpu().numpy()
                assert np.array_equal(bits(got), bits(m.value.reshape(got.shape))), (where, f)

        vec.reset()
        snap = vec.world.snapshot()
        for f, m in models.items():
            m.reset(snap[f], np.ones(E * R, bool))
        check("reset")
        maps = vec.world_maps().tolist()
        rng = np.random.default_rng(2)
        changed = 0
        for s in range(16):
            a = np.zeros((E * R, 3), np.float32)
            a[:, 0], a[:, 1] = rng.uniform(0, 0.6, E * R), rng.uniform(-0.9, 0.9, E * R)
            vec.step(torch.as_tensor(a, device="cuda"))
            finished, first = vec.world.autoreset_last()
            now = vec.world_maps().tolist()
            for q, k in enumerate(finished):
                assert now[k] == _cabi.map_for_placement(vec._device_seed0 + first + q, 3), (s, k)
                changed += now[k] != maps[k]
            assert all(now[k] == maps[k] for k in range(E) if k not in finished), s
            maps = now
            rows = np.zeros(E * R, bool)
            for k in finished:
                rows[k * R:(k + 1) * R] = True
            snap = vec.world.snapshot()
            for f, m in models.items():
                m.update(snap[f], rows)
            check(s)
        assert changed > 0
    finally:
        vec.close()


# ---- 7. refusals ----
def test_refusals(worlds):
    World, _ = worlds
    import ctypes as C
    from img_env_amd import _cabi, worldgen
    W, Rw, Pw = 2, 3, 2
    grids = _grids(3, 200, 61)
    params = worldgen.make_params(Rw, Pw)
    lays = [worldgen.make_layout(grids[0], 0.125, Rw, Pw, seed=61 + k, n_obstacles=2) for k in range(W)]
    more = np.ascontiguousarray(np.stack(grids[1:]))

    def add(w, maps, h=None, wd=None):
        return w.lib.imgenv_maps_add(w.h, len(maps), maps.ctypes.data, maps.shape[1] if h is None else h, maps.shape[2] if wd is None else wd)

    def select(w, ks, ms):
        n = len(ks)
        return w.lib.imgenv_world_maps_set(w.h, n, (C.c_int32 * n)(*ks), (C.c_int32 * n)(*ms), None)

    w = World(_stack_params(params, W), grids[0])
    try:
        assert add(w, more[:, :150], 150, 200) == _cabi.EINVAL and b"one size" in w.lib.imgenv_last_error()  # another map size
        assert add(w, more, 100, 400) == _cabi.EINVAL                                                        # (the same cell count)
        assert w.lib.imgenv_maps_policy(w.h, _cabi.MAPS_BY_PLACEMENT) == 0  # one map: accepted, a no-op
        assert w.lib.imgenv_maps_policy(w.h, 7) == _cabi.EINVAL
        assert select(w, [0], [1]) == _cabi.EINVAL and select(w, [0, 1], [0, 0]) == 0  # one map: only id 0 exists
        assert add(w, more) == 0
        assert add(w, more) == _cabi.ESTATE                                  # a second call
        assert w.world_maps().tolist() == [0, 0]
        # a bad map id, a bad world, a world listed twice: refused, and NOTHING of the call is applied
        assert select(w, [0, 1], [1, 3]) == _cabi.EINVAL and b"map 3" in w.lib.imgenv_last_error()
        assert select(w, [0, 1], [1, -1]) == _cabi.EINVAL
        assert select(w, [0, 2], [1, 1]) == _cabi.EINVAL and b"world 2" in w.lib.imgenv_last_error()
        assert select(w, [0, -1], [1, 1]) == _cabi.EINVAL
        assert select(w, [1, 1], [1, 2]) == _cabi.EINVAL and b"twice" in w.lib.imgenv_last_error()
        with pytest.raises(ValueError, match="listed twice"):
            w.set_world_maps([1, 1], [1, 2])
        w.reset(lays)
        assert w.world_maps().tolist() == [0, 0]  # no refused selection left a trace
        assert select(w, [1], [2]) == 0
        w.reset_world(1, lays[1])
        assert w.world_maps().tolist() == [0, 2]
        w.step(np.zeros((W * Rw, 3), np.float32))
    finally:
        w.close()
    w = World(_stack_params(params, W), grids[0])
    try:
        w.reset(lays)
        assert add(w, more) == _cabi.ESTATE and b"after the first reset" in w.lib.imgenv_last_error()
    finally:
        w.close()
    w = World(_stack_params(params, W), grids[0])
    try:
        w.reset_world(1, lays[1])  # one world of the handle has been reset: too late as well
        assert add(w, more) == _cabi.ESTATE
    finally:
        w.close()
    # a robot shard
    shard = dict(worldgen.make_params(4, 2), robot_begin=0, robot_end=2)
    w = World(shard, grids[0])
    try:
        assert add(w, more) == _cabi.EINVAL and b"shard" in w.lib.imgenv_last_error()
    finally:
        w.close()
    with pytest.raises(ValueError, match="imgenv_maps_add"):
        World(shard, grids)
    with pytest.raises(ValueError, match="equal-shaped"):
        World(_stack_params(params, W), [grids[0], grids[1][:150]])
    # one map and IMGENV_MAPS_BY_PLACEMENT: the handle resets and steps as ever, on map 0
    w = World(_stack_params(params, W), grids[0])
    try:
        w.set_maps_policy("placement")
        w.reset(lays)
        w.step(np.zeros((W * Rw, 3), np.float32))
        assert w.world_maps().tolist() == [0, 0]
    finally:
        w.close()
