"""The variant matrix: one small world per kernel instantiation the launch plan (csrc/launch_plan.h) can pick.

`CASES` is the table tests/test_gpu_variant_matrix.py runs against the oracle; `census_line` turns a case into the input of
tests/host/variant_census.cpp, which says -- out of the committed headers -- which instantiations the case's chains of launches
run; `EXPECT` is what it said when the table was written, and is part of each GPU test's id.  tests/test_variant_census.py holds
`EXPECT` to the census, and the union of the table to the census's lattice of handle facts: a threshold that moves fails there,
on the CPU, instead of silently emptying a GPU case.

A case is parameters for `scenarios.small_world` plus
    flags     names of `_cabi.FLAG_*` bits (COMPOSE_DENSE, COMPOSE_SPARSE, LAYER_SUM, VIEW_TILED)
    kind      "whole": one handle that owns its world; "shards": ranks 0 / 1 of a robot-sharded world on one GPU, each held to its
              slice of the oracle's whole world; "worlds": `worlds` worlds in one handle, one oracle each, `listed` of them reset in
              mid-episode
    spatial   (shards) contiguous index ranges are vertical strips of the map, not interleaved robots
    image     (big views) the sensor_map's size where the view is shrunk to it
    one_class no mixed footprints (the packed rasters take one robot class, a SUM shard's bitmaps a small box)
    seed      the layout's seed, where seed 0 does not give the episode its collisions (`Exercise`, below)
dt, state_dim, robot_ktype, ped_shape and the footprint classes are drawn from np.random.default_rng(the case's index), the way
tests/test_gpu_parity.py::_fuzz_case draws them -- so a new case goes at the END of the table: the index also seeds the layouts.
"""
import numpy as np

from img_env_amd import _cabi
from scenarios import random_actions, small_world

STEPS_A, STEPS_B = 6, 3  # steps in front of the listed reset (or of nothing) and behind it

# res 0.1 / 0.2: not a power of two.  view 50 / 37 cells: not a multiple of four (37: 3.75 m at 0.1).  96 cells and 720 beams:
# a view whose LDS leaves a compute unit 16 workgroups or fewer (plan_lds_bound); 98 cells: the same, not a multiple of four.
_V37 = dict(view_cells=37, view_width=3.75, view_height=3.75)
CASES = {
    # ---- k_view<pow2, a4, stamp, 8>: at most 1024 robots; the rasters of a small handle: k_raster<.., 4> in the reset, k_move_raster<.., 4>
    "nw8_p1_a1_stamp": dict(n_robots=24, n_peds=8, res=0.125, view_cells=48, beams=400, grid_size=96, clearance=0.5),
    "nw8_p1_a0_stamp": dict(n_robots=24, n_peds=8, res=0.25, view_cells=50, beams=719, grid_size=60, clearance=0.55),
    "nw8_p0_a1_stamp": dict(n_robots=24, n_peds=8, res=0.2, view_cells=48, beams=719, grid_size=64, clearance=0.5),
    "nw8_p0_a0_stamp": dict(n_robots=24, n_peds=8, res=0.1, beams=400, grid_size=120, clearance=0.5, **_V37),
    "nw8_p1_a1_sum": dict(n_robots=24, n_peds=8, res=0.125, view_cells=48, beams=719, grid_size=96, clearance=0.5, flags=["LAYER_SUM"]),
    "nw8_p1_a0_composed": dict(n_robots=24, n_peds=8, res=0.25, view_cells=50, beams=400, grid_size=60, clearance=0.55, flags=["COMPOSE_DENSE"]),
    "nw8_p0_a1_composed": dict(n_robots=24, n_peds=8, res=0.2, view_cells=48, beams=400, grid_size=64, clearance=0.5, flags=["COMPOSE_DENSE"]),
    "nw8_p0_a0_sum": dict(n_robots=24, n_peds=8, res=0.1, beams=719, grid_size=120, clearance=0.5, flags=["LAYER_SUM"], **_V37),
    # ---- k_view<.., 4>: LDS-bound views, 16 robots
    "nw4_p1_a1_stamp": dict(n_robots=16, n_peds=8, res=0.125, view_cells=96, beams=720, grid_size=72, clearance=0.5),
    "nw4_p1_a0_stamp": dict(n_robots=16, n_peds=8, res=0.125, view_cells=98, beams=720, grid_size=72, clearance=0.5),
    "nw4_p0_a1_stamp": dict(n_robots=16, n_peds=8, res=0.1, view_cells=96, beams=720, grid_size=90, clearance=0.5),
    "nw4_p0_a0_stamp": dict(seed=1, n_robots=16, n_peds=8, res=0.1, view_cells=98, beams=720, grid_size=80, clearance=0.5),
    "nw4_p1_a1_composed": dict(n_robots=16, n_peds=8, res=0.125, view_cells=96, beams=720, grid_size=72, clearance=0.5, flags=["COMPOSE_DENSE"]),
    "nw4_p1_a0_sum": dict(n_robots=16, n_peds=8, res=0.125, view_cells=98, beams=720, grid_size=72, clearance=0.5, flags=["LAYER_SUM"]),
    "nw4_p0_a1_sum": dict(seed=2, n_robots=16, n_peds=8, res=0.1, view_cells=96, beams=720, grid_size=90, clearance=0.5, flags=["LAYER_SUM"]),
    "nw4_p0_a0_composed": dict(n_robots=16, n_peds=8, res=0.1, view_cells=98, beams=720, grid_size=90, clearance=0.5, flags=["COMPOSE_DENSE"]),
    # ---- k_view<.., 2>: 1025 robots.  Without pedestrians the move stays fused up to 4096 robots: k_move_raster<.., 1>; beside
    # pedestrians it is k_integrate with the gated early k_obs, and k_raster<.., 1> in roomy blocks of their own
    "nw2_p1_a1_stamp_fused": dict(n_robots=1025, n_peds=0, res=0.25, view_cells=48, beams=400, grid_size=164, clearance=0.75, flags=["COMPOSE_SPARSE"]),
    "nw2_p1_a0_sum_fused": dict(n_robots=1025, n_peds=0, res=0.25, view_cells=50, beams=719, grid_size=164, clearance=0.75, flags=["LAYER_SUM"]),
    "nw2_p0_a1_composed_fused": dict(n_robots=1025, n_peds=0, res=0.2, view_cells=48, beams=719, grid_size=192, clearance=0.75, flags=["COMPOSE_DENSE"]),
    "nw2_p0_a0_stamp_fused": dict(n_robots=1025, n_peds=0, res=0.2, view_cells=50, beams=400, grid_size=192, clearance=0.75, flags=["COMPOSE_SPARSE"]),
    "nw2_p1_a1_composed_fused": dict(n_robots=1025, n_peds=0, res=0.25, view_cells=48, beams=719, grid_size=164, clearance=0.75, flags=["COMPOSE_DENSE"]),
    "nw2_p0_a1_sum_fused": dict(seed=4, n_robots=1025, n_peds=0, res=0.2, view_cells=48, beams=400, grid_size=192, clearance=0.75, flags=["LAYER_SUM"]),
    "nw2_p1_a0_stamp_early": dict(n_robots=1025, n_peds=12, res=0.25, view_cells=50, beams=400, grid_size=164, clearance=0.75, flags=["COMPOSE_SPARSE"]),
    "nw2_p0_a0_sum_early": dict(n_robots=1025, n_peds=12, res=0.2, view_cells=50, beams=719, grid_size=192, clearance=0.75, flags=["LAYER_SUM"]),
    "nw2_p0_a1_stamp_early": dict(n_robots=1025, n_peds=12, res=0.2, view_cells=48, beams=719, grid_size=192, clearance=0.75, flags=["COMPOSE_SPARSE"]),
    "nw2_p1_a1_sum_early": dict(n_robots=1025, n_peds=12, res=0.25, view_cells=48, beams=400, grid_size=164, clearance=0.75, flags=["LAYER_SUM"]),
    "nw2_p0_a0_composed_early": dict(n_robots=1025, n_peds=12, res=0.2, view_cells=50, beams=400, grid_size=192, clearance=0.75, flags=["COMPOSE_DENSE"]),
    "nw2_p1_a0_composed_early": dict(n_robots=1025, n_peds=12, res=0.25, view_cells=50, beams=719, grid_size=164, clearance=0.75, flags=["COMPOSE_DENSE"]),
    # ---- k_view<.., 1>: 4097 robots (eight of the ten cases above 4096 robots the suite allows itself; one of them with 8193 robots
    # and pedestrians: more than 8192 blocks of rasters, where robots and pedestrians share blocks again -- neither split nor roomy)
    "nw1_p1_a1_stamp": dict(n_robots=4097, n_peds=12, res=0.25, view_cells=48, beams=400, grid_size=304, clearance=0.75, flags=["COMPOSE_SPARSE"]),
    "nw1_p1_a0_stamp_unsplit": dict(n_robots=8193, n_peds=12, res=0.25, view_cells=50, beams=400, grid_size=428, clearance=0.75, flags=["COMPOSE_SPARSE"]),
    "nw1_p0_a1_stamp": dict(n_robots=4097, n_peds=0, res=0.2, view_cells=48, beams=400, grid_size=380, clearance=0.75, flags=["COMPOSE_SPARSE"]),
    "nw1_p0_a0_stamp": dict(n_robots=4097, n_peds=12, res=0.2, view_cells=50, beams=400, grid_size=380, clearance=0.75, flags=["COMPOSE_SPARSE"]),
    "nw1_p1_a1_composed": dict(n_robots=4097, n_peds=0, res=0.25, view_cells=48, beams=400, grid_size=304, clearance=0.75, flags=["COMPOSE_DENSE"]),
    "nw1_p1_a0_sum": dict(n_robots=4097, n_peds=12, res=0.25, view_cells=50, beams=400, grid_size=304, clearance=0.75),
    "nw1_p0_a1_sum": dict(n_robots=4097, n_peds=12, res=0.2, view_cells=48, beams=400, grid_size=380, clearance=0.75),
    "nw1_p0_a0_composed": dict(n_robots=4097, n_peds=12, res=0.2, view_cells=50, beams=400, grid_size=380, clearance=0.75, flags=["COMPOSE_DENSE"]),
    # ---- more than 8192 blocks of rasters on the counting layer of ONE robot class: four robots to a wavefront (k_raster_pack<.., 4>)
    "packed_p0": dict(n_robots=8192, n_peds=12, res=0.2, view_cells=50, beams=400, grid_size=536, clearance=0.75, one_class=True),
    "packed_p1": dict(n_robots=8193, n_peds=12, res=0.25, view_cells=50, beams=400, grid_size=428, clearance=0.75, one_class=True),
    # ---- robot shards against the oracle's whole world: k_remote<pow2> behind the exchange (counting layer), or every rank's
    # rasters over everybody (composed)
    "shards_p0_sum_interleaved": dict(n_robots=48, n_peds=10, res=0.1, view_cells=50, beams=400, grid_size=110, clearance=0.5, kind="shards", flags=["LAYER_SUM"], one_class=True),
    "shards_p0_sum_spatial": dict(n_robots=48, n_peds=10, res=0.1, beams=719, grid_size=110, clearance=0.5, kind="shards", spatial=True, flags=["LAYER_SUM"], one_class=True, **_V37),
    "shards_p0_composed_interleaved": dict(n_robots=48, n_peds=10, res=0.1, beams=400, grid_size=110, clearance=0.5, kind="shards", flags=["COMPOSE_DENSE"], **_V37),
    "shards_p0_composed_spatial": dict(n_robots=48, n_peds=10, res=0.1, view_cells=50, beams=719, grid_size=110, clearance=0.5, kind="shards", spatial=True, flags=["COMPOSE_DENSE"]),
    "shards_p1_sum_interleaved": dict(n_robots=64, n_peds=10, res=0.25, view_cells=50, beams=400, grid_size=52, clearance=0.55, kind="shards", flags=["LAYER_SUM"], one_class=True),
    # ---- several worlds in one handle, two of them reset in mid-episode (the listed chain)
    "worlds_p0_a0_stamp": dict(seed=2, n_robots=8, n_peds=5, res=0.1, beams=400, grid_size=100, clearance=0.5, kind="worlds", worlds=3, listed=2, **_V37),
    "worlds_p0_a0_sum": dict(n_robots=8, n_peds=5, res=0.2, view_cells=50, beams=719, grid_size=52, clearance=0.5, kind="worlds", worlds=3, listed=2, flags=["LAYER_SUM"]),
    # ---- the tiled kernels (csrc/view_big.h): k_crop_big, k_beams_big<pow2, stamp, bits_in_lds>, the shrunk sensor_map's k_taps_big
    "big_p1_stamp": dict(seed=1, n_robots=24, n_peds=8, res=0.125, view_cells=50, beams=400, grid_size=64, clearance=0.5, flags=["VIEW_TILED"]),
    "big_p0_stamp_shrunk": dict(n_robots=24, n_peds=8, res=0.1, view_cells=98, beams=719, grid_size=80, clearance=0.5, image=48),
    "big_p1_composed_shrunk": dict(n_robots=24, n_peds=8, res=0.125, view_cells=98, beams=719, grid_size=64, clearance=0.5, image=48, flags=["COMPOSE_DENSE"]),
    "big_p0_composed": dict(seed=1, n_robots=24, n_peds=8, res=0.2, view_cells=50, beams=400, grid_size=48, clearance=0.5, flags=["VIEW_TILED", "COMPOSE_DENSE"]),
    # ... and views of more than 1108 x 1108 cells, whose crop bitmap no longer fits the LDS beside the hit words (plan_big_bits_in_lds)
    "huge_p1_stamp": dict(seed=2, n_robots=10, n_peds=6, res=0.015625, view_cells=1112, beams=400, grid_size=384, clearance=0.45, flags=["VIEW_TILED"]),
    "huge_p0_stamp": dict(n_robots=10, n_peds=6, res=0.015, view_cells=1112, beams=719, grid_size=384, clearance=0.45, flags=["VIEW_TILED"]),
    "huge_p1_composed": dict(n_robots=10, n_peds=6, res=0.015625, view_cells=1112, beams=719, grid_size=384, clearance=0.45, flags=["VIEW_TILED", "COMPOSE_DENSE"]),
    "huge_p0_composed": dict(n_robots=10, n_peds=6, res=0.015, view_cells=1112, beams=400, grid_size=384, clearance=0.45, flags=["VIEW_TILED", "COMPOSE_DENSE"]),
}
INDEX = {name: q for q, name in enumerate(CASES)}


def case_flags(case):
    return sum(getattr(_cabi, "FLAG_" + f) for f in case.get("flags", ()))


def _draw(name, case):
    """the seeded part of a case: what small_world takes beyond the table, and whether the footprints are mixed"""
    rng = np.random.default_rng(INDEX[name])
    kw = dict(dt=float(rng.choice([0.1, 0.25, 0.4])), state_dim=int(rng.choice([3, 4, 5])),
              robot_ktype=str(rng.choice(["diff", "omni"])), ped_shape=str(rng.choice(["circle", "leg"])))
    return kw, bool(rng.random() < 0.6) and not case.get("one_class")


def _mix_footprints(params, n, rng):
    """circles of two sizes and rectangles in one world (tests/test_gpu_parity.py::_fuzz_case)"""
    shape = np.full(n, _cabi.SHAPE_CIRCLE, np.int32)
    size = np.tile(np.array([0, 0, 0.17, 0], np.float32), (n, 1))
    size[1::2] = (0.01, 0.02, float(rng.uniform(0.12, 0.3)), 0)
    shape[::3] = _cabi.SHAPE_RECTANGLE
    size[::3] = (-0.22, 0.18, -0.12, 0.1)
    params.update(robot_shape=shape, robot_size=size,
                  robot_size_last=np.where(shape == _cabi.SHAPE_CIRCLE, size[:, 2], 0.1).astype(np.float64))


def build(name, seed=None):
    """(grid, params of ONE world, [layout of the first episode per world], [layouts of the listed reset], lateral speeds?)"""
    case = CASES[name]
    drawn, mixed = _draw(name, case)
    skip = ("flags", "kind", "spatial", "worlds", "listed", "image", "one_class", "seed")
    kw = {k: v for k, v in case.items() if k not in skip}
    kw.update(drawn)
    seed = case.get("seed", 0) if seed is None else seed
    n, P = kw.pop("n_robots"), kw.pop("n_peds")
    if "view_width" not in kw:  # (float32(cells * res) / float32(res) may fall just short of `cells`: half a cell of room)
        kw["view_width"] = kw["view_height"] = (kw["view_cells"] + 0.5) * kw["res"]
    grid, params, layout = small_world(n, P, seed=100 * INDEX[name] + seed, n_obstacles=3, **kw)
    if mixed:
        _mix_footprints(params, n, np.random.default_rng(INDEX[name]))
    if case.get("image"):
        params["image_size"] = (case["image"], case["image"])
    params["flags"] = int(params.get("flags", 0)) | case_flags(case)
    if case.get("spatial"):  # contiguous index ranges = vertical strips of the map
        order = np.argsort(layout.robot_pose[:, 0], kind="stable")
        layout.robot_pose, layout.robot_goal = layout.robot_pose[order].copy(), layout.robot_goal[order].copy()
    W = case.get("worlds", 1)
    pick = dict(grid_size=kw["grid_size"], res=kw["res"], n_obstacles=2, clearance=kw["clearance"])
    first = [layout] + [small_world(n, P, seed=100 * INDEX[name] + seed + 7 * k, **pick)[2] for k in range(1, W)]
    again = [small_world(n, P, seed=100 * INDEX[name] + seed + 50 + k, **pick)[2] for k in range(case.get("listed", 0))]
    return grid, params, first, again, drawn.get("robot_ktype") == "omni"


def stack_params(params, W):
    """the parameter dict of W copies of one world: per-robot / per-pedestrian rows repeat, world-major"""
    p = dict(params)
    for k in ("robot_shape", "robot_size", "robot_sensor_cfg", "robot_size_last", "ped_shape", "ped_size", "ped_max_speed"):
        p[k] = np.concatenate([np.asarray(p[k])] * W, axis=0)
    p["n_robots"], p["n_peds"], p["n_worlds"] = params["n_robots"] * W, params["n_peds"] * W, W
    return p


def handle_params(name, params):
    """the parameter dicts of the HIP handles a case creates: the whole world, the two ranks, or the stacked worlds"""
    case = CASES[name]
    kind = case.get("kind", "whole")
    if kind == "shards":
        n = params["n_robots"]
        return [dict(params, robot_begin=r * n // 2, robot_end=(r + 1) * n // 2) for r in range(2)]
    if kind == "worlds":
        return [stack_params(params, case["worlds"])]
    return [params]


def actions(rng, n, lateral):
    a = random_actions(rng, n)
    if lateral:
        a[:, 2] = rng.uniform(-0.3, 0.3, n).astype(np.float32)
    return a


# ---------------------------------------------------------------------------------------- the census's input
def census_line(name, params, grid_shape, listed=0, raster_pack=-1, early_obs_off=0, split_step=0):
    """one case of tests/host/variant_census.cpp: the configuration `_cabi.make_cfg` would hand to imgenv_create, as words"""
    p = params
    R, P = int(p["n_robots"]), int(p["n_peds"])
    words = ["name=" + name, "Hg=%d" % grid_shape[0], "Wg=%d" % grid_shape[1], "listed=%d" % listed, "raster_pack=%d" % raster_pack,
             "early_obs_off=%d" % early_obs_off, "split_step=%d" % split_step, "n_robots=%d" % R, "n_peds=%d" % P, "robot_begin=%d" % p.get("robot_begin", 0),
             "robot_end=%d" % p.get("robot_end", R), "n_worlds=%d" % p.get("n_worlds", 1), "flags=%d" % p.get("flags", 0),
             "image_w=%d" % p["image_size"][0], "image_h=%d" % p["image_size"][1]]
    for k in ("max_ped", "state_dim", "use_laser", "range_total", "ped_scene_type", "relation_ped_robo"):
        words.append("%s=%d" % (k, int(p[k])))
    for k in ("view_resolution", "global_resolution", "view_width", "view_height", "view_angle_begin", "view_angle_end",
              "view_min_dist", "view_max_dist", "step_hz"):
        words.append("%s=%r" % (k, float(np.float32(p[k]))))
    for k in ("beep_r", "ped_ca_p"):
        words.append("%s=%r" % (k, float(p.get(k, 0.0))))
    rc = np.concatenate([np.asarray(p["robot_shape"], np.float32).reshape(R, 1), np.asarray(p["robot_size"], np.float32).reshape(R, 4),
                         np.asarray(p.get("robot_sensor_cfg", np.zeros((R, 2))), np.float32).reshape(R, 2)], axis=1)
    for row in np.unique(rc, axis=0):
        words.append("rc=" + ":".join(repr(float(v)) for v in row))
    if P:
        pc = np.concatenate([np.asarray(p["ped_shape"], np.float32).reshape(P, 1), np.asarray(p["ped_size"], np.float32).reshape(P, 6)], axis=1)
        for row in np.unique(pc, axis=0):
            words.append("pc=" + ":".join(repr(float(v)) for v in row))
    return " ".join(words)


def case_census_lines(name):
    """the census input of every handle the case creates (the ranks of a sharded case as <name>/rank0, <name>/rank1)"""
    grid, params, _, _, _ = build(name)
    hp = handle_params(name, params)
    names = [name] if len(hp) == 1 else ["%s/rank%d" % (name, r) for r in range(len(hp))]
    return [census_line(nm, p, grid.shape, listed=CASES[name].get("listed", 0)) for nm, p in zip(names, hp)]


KERNELS = ("k_view", "k_raster", "k_move_raster", "k_raster_pack", "k_remote", "k_crop_big", "k_beams_big", "k_obs", "k_taps_big",
           "k_fullview_big", "k_compose", "k_integrate")


def parse_census(text):
    """{handle name: {chain: [words]}} from the census's output"""
    out = {}
    for line in text.splitlines():
        w = line.split()
        if len(w) < 2 or w[1] == "REFUSED" or w[0] in ("BAD", "LATTICE:"):
            raise ValueError("census: " + line)
        out.setdefault(w[0], {})[w[1]] = w[2:]
    return out


def tuple_of(chains):
    """the variant tuple of one handle, as a test id carries it: the step (both outcomes of gates_work where they differ), then
    what the reset and the listed reset run differently"""
    step, cold = chains["step/gates=1"], chains["step/gates=0"]
    parts = [" ".join(w for w in step if not w.startswith(("serial_move=0", "lds_bound=", "k_compose", "k_integrate", "k_taps", "k_fullview")))]
    if cold != step:
        parts.append("gates=0: " + " ".join(w for w in cold if w not in step))
    for chain in ("reset", "listed"):
        extra = [w for w in chains.get(chain, ()) if w not in step and w.startswith("k_")]
        if extra:
            parts.append(chain + ": " + " ".join(extra))
    return "; ".join(parts)


# what the census said when the table was written (tests/test_variant_census.py keeps it true)
EXPECT = {
    "nw8_p1_a1_stamp": "fuse_move=1 early_step=0 k_move_raster<1,STAMP,4> split=1 roomy=0 k_obs<1> k_view<1,1,1,8>; reset: k_raster<1,STAMP,4>",
    "nw8_p1_a0_stamp": "fuse_move=1 early_step=0 k_move_raster<1,STAMP,4> split=1 roomy=0 k_obs<1> k_view<1,0,1,8>; reset: k_raster<1,STAMP,4>",
    "nw8_p0_a1_stamp": "fuse_move=1 early_step=0 k_move_raster<0,STAMP,4> split=1 roomy=0 k_obs<1> k_view<0,1,1,8>; reset: k_raster<0,STAMP,4>",
    "nw8_p0_a0_stamp": "fuse_move=1 early_step=0 k_move_raster<0,STAMP,4> split=1 roomy=0 k_obs<1> k_view<0,0,1,8>; reset: k_raster<0,STAMP,4>",
    "nw8_p1_a1_sum": "fuse_move=1 early_step=0 k_move_raster<1,SUM,4> split=1 roomy=0 k_obs<1> k_view<1,1,0,8>; reset: k_raster<1,SUM,4>",
    "nw8_p1_a0_composed": "fuse_move=1 early_step=0 k_move_raster<1,COMPOSED,4> split=1 roomy=0 k_obs<1> k_view<1,0,0,8>; reset: k_raster<1,COMPOSED,4>",
    "nw8_p0_a1_composed": "fuse_move=1 early_step=0 k_move_raster<0,COMPOSED,4> split=1 roomy=0 k_obs<1> k_view<0,1,0,8>; reset: k_raster<0,COMPOSED,4>",
    "nw8_p0_a0_sum": "fuse_move=1 early_step=0 k_move_raster<0,SUM,4> split=1 roomy=0 k_obs<1> k_view<0,0,0,8>; reset: k_raster<0,SUM,4>",
    "nw4_p1_a1_stamp": "fuse_move=1 early_step=0 k_move_raster<1,STAMP,4> split=1 roomy=0 k_obs<1> k_view<1,1,1,4>; reset: k_raster<1,STAMP,4>",
    "nw4_p1_a0_stamp": "fuse_move=1 early_step=0 k_move_raster<1,STAMP,4> split=1 roomy=0 k_obs<1> k_view<1,0,1,4>; reset: k_raster<1,STAMP,4>",
    "nw4_p0_a1_stamp": "fuse_move=1 early_step=0 k_move_raster<0,STAMP,4> split=1 roomy=0 k_obs<1> k_view<0,1,1,4>; reset: k_raster<0,STAMP,4>",
    "nw4_p0_a0_stamp": "fuse_move=1 early_step=0 k_move_raster<0,STAMP,4> split=1 roomy=0 k_obs<1> k_view<0,0,1,4>; reset: k_raster<0,STAMP,4>",
    "nw4_p1_a1_composed": "fuse_move=1 early_step=0 k_move_raster<1,COMPOSED,4> split=1 roomy=0 k_obs<1> k_view<1,1,0,4>; reset: k_raster<1,COMPOSED,4>",
    "nw4_p1_a0_sum": "fuse_move=1 early_step=0 k_move_raster<1,SUM,4> split=1 roomy=0 k_obs<1> k_view<1,0,0,4>; reset: k_raster<1,SUM,4>",
    "nw4_p0_a1_sum": "fuse_move=1 early_step=0 k_move_raster<0,SUM,4> split=1 roomy=0 k_obs<1> k_view<0,1,0,4>; reset: k_raster<0,SUM,4>",
    "nw4_p0_a0_composed": "fuse_move=1 early_step=0 k_move_raster<0,COMPOSED,4> split=1 roomy=0 k_obs<1> k_view<0,0,0,4>; reset: k_raster<0,COMPOSED,4>",
    "nw2_p1_a1_stamp_fused": "fuse_move=1 early_step=0 k_move_raster<1,STAMP,1> split=0 roomy=1 k_view<1,1,1,2>; reset: k_raster<1,STAMP,1>",
    "nw2_p1_a0_sum_fused": "fuse_move=1 early_step=0 k_move_raster<1,SUM,1> split=0 roomy=1 k_view<1,0,0,2>; reset: k_raster<1,SUM,1>",
    "nw2_p0_a1_composed_fused": "fuse_move=1 early_step=0 k_move_raster<0,COMPOSED,1> split=0 roomy=1 k_view<0,1,0,2>; reset: k_raster<0,COMPOSED,1>",
    "nw2_p0_a0_stamp_fused": "fuse_move=1 early_step=0 k_move_raster<0,STAMP,1> split=0 roomy=1 k_view<0,0,1,2>; reset: k_raster<0,STAMP,1>",
    "nw2_p1_a1_composed_fused": "fuse_move=1 early_step=0 k_move_raster<1,COMPOSED,1> split=0 roomy=1 k_view<1,1,0,2>; reset: k_raster<1,COMPOSED,1>",
    "nw2_p0_a1_sum_fused": "fuse_move=1 early_step=0 k_move_raster<0,SUM,1> split=0 roomy=1 k_view<0,1,0,2>; reset: k_raster<0,SUM,1>",
    "nw2_p1_a0_stamp_early": "fuse_move=0 early_step=1 k_raster<1,STAMP,1> split=1 roomy=1 k_obs<1> k_view<1,0,1,2>; gates=0: early_step=0",
    "nw2_p0_a0_sum_early": "fuse_move=0 early_step=1 k_raster<0,SUM,1> split=1 roomy=1 k_obs<1> k_view<0,0,0,2>; gates=0: early_step=0",
    "nw2_p0_a1_stamp_early": "fuse_move=0 early_step=1 k_raster<0,STAMP,1> split=1 roomy=1 k_obs<1> k_view<0,1,1,2>; gates=0: early_step=0",
    "nw2_p1_a1_sum_early": "fuse_move=0 early_step=1 k_raster<1,SUM,1> split=1 roomy=1 k_obs<1> k_view<1,1,0,2>; gates=0: early_step=0",
    "nw2_p0_a0_composed_early": "fuse_move=0 early_step=1 k_raster<0,COMPOSED,1> split=1 roomy=1 k_obs<1> k_view<0,0,0,2>; gates=0: early_step=0",
    "nw2_p1_a0_composed_early": "fuse_move=0 early_step=1 k_raster<1,COMPOSED,1> split=1 roomy=1 k_obs<1> k_view<1,0,0,2>; gates=0: early_step=0",
    "nw1_p1_a1_stamp": "fuse_move=0 early_step=1 k_raster<1,STAMP,1> split=1 roomy=1 k_obs<1> k_view<1,1,1,1>; gates=0: early_step=0",
    "nw1_p1_a0_stamp_unsplit": "fuse_move=0 early_step=1 k_raster<1,STAMP,1> split=0 roomy=0 k_obs<1> k_view<1,0,1,1>; gates=0: early_step=0",
    "nw1_p0_a1_stamp": "fuse_move=0 early_step=0 k_raster<0,STAMP,1> split=0 roomy=1 k_view<0,1,1,1>",
    "nw1_p0_a0_stamp": "fuse_move=0 early_step=1 k_raster<0,STAMP,1> split=1 roomy=1 k_obs<1> k_view<0,0,1,1>; gates=0: early_step=0",
    "nw1_p1_a1_composed": "fuse_move=0 early_step=0 k_raster<1,COMPOSED,1> split=0 roomy=1 k_view<1,1,0,1>",
    "nw1_p1_a0_sum": "fuse_move=0 early_step=1 k_raster<1,SUM,1> split=1 roomy=1 k_obs<1> k_view<1,0,0,1>; gates=0: early_step=0",
    "nw1_p0_a1_sum": "fuse_move=0 early_step=1 k_raster<0,SUM,1> split=1 roomy=1 k_obs<1> k_view<0,1,0,1>; gates=0: early_step=0",
    "nw1_p0_a0_composed": "fuse_move=0 early_step=1 k_raster<0,COMPOSED,1> split=1 roomy=1 k_obs<1> k_view<0,0,0,1>; gates=0: early_step=0",
    "packed_p0": "fuse_move=0 early_step=1 k_raster_pack<0,4> k_obs<1> k_view<0,0,0,1>; gates=0: early_step=0; reset: k_raster<0,SUM,1>",
    "packed_p1": "fuse_move=0 early_step=1 k_raster_pack<1,4> k_obs<1> k_view<1,0,0,1>; gates=0: early_step=0; reset: k_raster<1,SUM,1>",
    "shards_p0_sum_interleaved": "fuse_move=1 early_step=0 k_move_raster<0,SUM,4> split=1 roomy=0 k_remote<0> k_obs<1> k_view<0,0,0,8>; reset: k_raster<0,SUM,4>",
    "shards_p0_sum_spatial": "fuse_move=1 early_step=0 k_move_raster<0,SUM,4> split=1 roomy=0 k_remote<0> k_obs<1> k_view<0,0,0,8>; reset: k_raster<0,SUM,4>",
    "shards_p0_composed_interleaved": "fuse_move=0 early_step=1 k_raster<0,COMPOSED,4> split=1 roomy=0 k_obs<1> k_view<0,0,0,8>; gates=0: early_step=0",
    "shards_p0_composed_spatial": "fuse_move=0 early_step=1 k_raster<0,COMPOSED,4> split=1 roomy=0 k_obs<1> k_view<0,0,0,8>; gates=0: early_step=0",
    "shards_p1_sum_interleaved": "fuse_move=1 early_step=0 k_move_raster<1,SUM,4> split=1 roomy=0 k_remote<1> k_obs<1> k_view<1,0,0,8>; reset: k_raster<1,SUM,4>",
    "worlds_p0_a0_stamp": "fuse_move=1 early_step=0 k_move_raster<0,STAMP,4> split=1 roomy=0 k_obs<1> k_view<0,0,1,8>; reset: k_raster<0,STAMP,4>; listed: k_raster<0,STAMP,4>",
    "worlds_p0_a0_sum": "fuse_move=1 early_step=0 k_move_raster<0,SUM,4> split=1 roomy=0 k_obs<1> k_view<0,0,0,8>; reset: k_raster<0,SUM,4>; listed: k_raster<0,SUM,4>",
    "big_p1_stamp": "fuse_move=1 early_step=0 k_move_raster<1,STAMP,4> split=1 roomy=0 k_obs<1> k_crop_big<2> k_beams_big<1,1,1>; reset: k_raster<1,STAMP,4>",
    "big_p0_stamp_shrunk": "fuse_move=1 early_step=0 k_move_raster<0,STAMP,4> split=1 roomy=0 k_obs<1> k_crop_big<2> k_beams_big<0,1,1>; reset: k_raster<0,STAMP,4>",
    "big_p1_composed_shrunk": "fuse_move=1 early_step=0 k_move_raster<1,COMPOSED,4> split=1 roomy=0 k_obs<1> k_crop_big<0> k_beams_big<1,0,1>; reset: k_raster<1,COMPOSED,4>",
    "big_p0_composed": "fuse_move=1 early_step=0 k_move_raster<0,COMPOSED,4> split=1 roomy=0 k_obs<1> k_crop_big<0> k_beams_big<0,0,1>; reset: k_raster<0,COMPOSED,4>",
    "huge_p1_stamp": "fuse_move=1 early_step=0 k_move_raster<1,STAMP,4> split=1 roomy=0 k_obs<1> k_crop_big<2> k_beams_big<1,1,0>; reset: k_raster<1,STAMP,4>",
    "huge_p0_stamp": "fuse_move=1 early_step=0 k_move_raster<0,STAMP,4> split=1 roomy=0 k_obs<1> k_crop_big<2> k_beams_big<0,1,0>; reset: k_raster<0,STAMP,4>",
    "huge_p1_composed": "fuse_move=1 early_step=0 k_move_raster<1,COMPOSED,4> split=1 roomy=0 k_obs<1> k_crop_big<0> k_beams_big<1,0,0>; reset: k_raster<1,COMPOSED,4>",
    "huge_p0_composed": "fuse_move=1 early_step=0 k_move_raster<0,COMPOSED,4> split=1 roomy=0 k_obs<1> k_crop_big<0> k_beams_big<0,0,0>; reset: k_raster<0,COMPOSED,4>",
}


def case_id(name):
    return "%s [%s]" % (name, EXPECT.get(name, "?"))


# ---------------------------------------------------------------------------------------- no vacuous passes
def _away(t):
    """C round(): half away from zero"""
    return np.where(t >= 0, np.floor(t + 0.5), np.ceil(t - 0.5)).astype(np.int64)


def _rot(z, w):
    """Matrix3x3::setRotation(Quaternion(0, 0, z, w)) (csrc/tfm.h)"""
    s = 2.0 / (z * z + w * w)
    return 1.0 - z * z * s, -w * z * s, w * z * s, 1.0 - z * z * s


class Exercise:
    """What an episode exercised, from the ORACLE's snapshots alone: collisions between robots and with obstacles or pedestrians, a
    view that holds another robot's cells (with a laser: a beam that ends on them), robots changing grid cell."""

    def __init__(self, params):
        self.res = float(np.float32(params["view_resolution"]))
        self.vw, self.vh = float(np.float32(params["view_width"])), float(np.float32(params["view_height"]))
        self.laser = bool(params["use_laser"])
        self.robot_robot = self.robot_other = self.sees_robot = False
        self.moved = []  # per step: the share of robots that changed grid cell
        self.shape, self.size, self._samples = np.asarray(params["robot_shape"]), np.asarray(params["robot_size"], np.float32), {}
        self._cell = None

    def add(self, snap, is_step):
        coll = snap["is_collisions"]
        self.robot_robot |= bool((coll == 3).any())
        self.robot_other |= bool(((coll == 1) | (coll == 2)).any())
        pose = snap["robot_pose"].astype(np.float64)
        cell = _away(pose[:, :2] / self.res)
        if is_step and self._cell is not None:
            self.moved.append(float((cell != self._cell).any(axis=1).mean()))
        self._cell = cell
        if not self.sees_robot:
            self.sees_robot = self._view_holds_a_robot(snap, pose, cell)

    def footprint_cells(self, j, pose):
        """the grid cells robot j covers: its 0.01 m samples (Agent::init_shape_circle / _rectangle, agent.cpp:18-62) through its pose"""
        key = (int(self.shape[j]),) + tuple(float(v) for v in self.size[j])
        if key not in self._samples:
            s = [float(v) for v in self.size[j]]
            if key[0] == _cabi.SHAPE_CIRCLE:
                bb = int(np.ceil(s[2] / 0.01))
                m, n = np.meshgrid(np.arange(-bb, bb + 1), np.arange(-bb, bb + 1), indexing="ij")
                keep = np.sqrt(m * 0.01 * m * 0.01 + n * 0.01 * n * 0.01) <= s[2]
                self._samples[key] = (m[keep] * 0.01 + s[0], n[keep] * 0.01 + s[1])
            else:
                m, n = np.meshgrid(np.arange(int(np.floor(s[0] / 0.01)), int(np.ceil(s[1] / 0.01)) + 1),
                                   np.arange(int(np.floor(s[2] / 0.01)), int(np.ceil(s[3] / 0.01)) + 1), indexing="ij")
                self._samples[key] = (m.ravel() * 0.01, n.ravel() * 0.01)
        fx, fy = self._samples[key]
        x, y, yaw = pose[j]
        p00, p01, p10, p11 = _rot(np.sin(yaw * 0.5), np.cos(yaw * 0.5))
        return _away(np.stack([(p00 * fx + p01 * fy) + x, (p10 * fx + p11 * fy) + y], axis=1) / self.res)

    def _view_holds_a_robot(self, snap, pose, cell):
        """a view cell of value 0 -- occupied; with a laser: where a beam ended -- that the oracle's own cell arithmetic (agent.cpp:
        373-392: view cell -> world -> grid cell) puts on a grid cell another robot's footprint covers"""
        res, view = self.res, snap["view_maps"]
        v00, v01, v10, v11 = _rot(np.sin(3.14159 * 0.5), np.cos(3.14159 * 0.5))  # view_base: Agent::init_view_map
        ox, oy = self.vh / 2, self.vw / 2
        live = np.flatnonzero((snap["is_collisions"] == 0) & (snap["is_arrives"] == 0))
        reach = 0.5 * min(self.vw, self.vh)
        for i in live[:64]:
            x, y, yaw = pose[i]
            near = np.flatnonzero((np.abs(pose[:, :2] - (x, y)) < reach).all(axis=1))
            near = near[near != i]
            ab = np.argwhere(view[i] == 0)
            if not len(near) or not len(ab):
                continue
            p00, p01, p10, p11 = _rot(np.sin(yaw * 0.5), np.cos(yaw * 0.5))
            xv, yv = ab[:, 0] * res, ab[:, 1] * res
            xb, yb = (v00 * xv + v01 * yv) + ox, (v10 * xv + v11 * yv) + oy
            g = _away(np.stack([(p00 * xb + p01 * yb) + x, (p10 * xb + p11 * yb) + y], axis=1) / res)
            seen = set(map(tuple, g))
            for j in near[:16]:
                if seen.intersection(map(tuple, np.unique(self.footprint_cells(j, pose), axis=0))):
                    return True
        return False


def missing(seen):
    """the conditions an episode did not meet, over all the worlds of its case (`seen`: an Exercise per world)"""
    out = []
    if not any(e.robot_robot for e in seen):
        out.append("no robot ran into another robot")
    if not any(e.robot_other for e in seen):
        out.append("no robot ran into an obstacle or a pedestrian")
    if not any(e.sees_robot for e in seen):
        out.append("no view holds another robot's cells" + (" (no beam ends on another robot)" if seen[0].laser else ""))
    moved = np.mean([e.moved for e in seen], axis=0) if all(len(e.moved) == len(seen[0].moved) for e in seen) else np.zeros(1)
    if not len(moved) or moved.min() < 0.05:
        out.append("fewer than 5 %% of the robots changed grid cell in a step: %s" % ["%.3f" % m for m in moved])
    return out


# ---------------------------------------------------------------------------------------- the episode
def _exchange_by_hand(ranks, bounds):
    """what the all-gather of a robot-sharded world delivers: every rank's own slice of the records, to every other rank"""
    import torch
    torch.cuda.synchronize()
    for r, w in enumerate(ranks):
        for q, o in enumerate(ranks):
            if q != r:
                w.records[bounds[q]:bounds[q + 1]].copy_(o.records[bounds[q]:bounds[q + 1]])


def run_case(name, OracleWorld, World=None, seed=None):
    """A reset, STEPS_A steps, the reset of the listed worlds (where the case has any), STEPS_B more steps -- on the oracle and, given
    `World`, on the case's HIP handles beside it, every EXACT and CLOSE field compared after every call.
    Returns (fails, [Exercise per world], [timing_read() of each handle over the last STEPS_B steps])."""
    from parity import CLOSE, EXACT, compare
    case = CASES[name]
    kind = case.get("kind", "whole")
    grid, params, first, again, lateral = build(name, seed)
    W, n, P = case.get("worlds", 1), params["n_robots"], params["n_peds"]
    per_robot = tuple(f for f in EXACT + CLOSE if f not in ("counters", "ped_state"))
    sliced = per_robot + (("ped_state",) if P else ())
    cpus = [OracleWorld(params, grid) for _ in range(W)]
    gpus = [World(p, grid) for p in handle_params(name, params)] if World else []
    seen, fails, timing = [Exercise(params) for _ in range(W)], [], []
    bounds = [0, n // 2, n]

    def check(where, is_step):
        wants = [c.snapshot() for c in cpus]
        for k, want in enumerate(wants):
            seen[k].add(want, is_step)
        if not gpus or len(fails) > 4:
            return
        if kind == "whole":
            bad = compare(gpus[0].snapshot(), wants[0])
            if bad:
                fails.append((where, bad))
        elif kind == "shards":  # each rank's slice of the oracle's whole world
            for r, g in enumerate(gpus):
                cut = {k: (v[bounds[r]:bounds[r + 1]] if k in per_robot else v) for k, v in wants[0].items()}
                bad = compare(g.snapshot(), cut, sliced)
                if bad:
                    fails.append((where, "rank %d" % r, bad))
        else:                   # each world's slice of the handle against that world's own oracle
            got = gpus[0].snapshot()
            for k, want in enumerate(wants):
                mine = {f: got[f][k * n:(k + 1) * n] for f in per_robot}
                mine["ped_state"] = got["ped_state"][k * P:(k + 1) * P]
                bad = compare(mine, want, sliced)
                if bad:
                    fails.append((where, "world %d" % k, bad))

    def step(a):
        for k, c in enumerate(cpus):
            c.step(a[k * n:(k + 1) * n])
        if kind == "shards" and gpus:
            for r, g in enumerate(gpus):
                g.step_begin(a[bounds[r]:bounds[r + 1]])
            _exchange_by_hand(gpus, bounds)
            for g in gpus:
                g.step_end()
        elif gpus:
            gpus[0].step(a)

    try:
        for c, lay in zip(cpus, first):
            c.reset(lay)
        for g in gpus:
            g.reset(first if kind == "worlds" else first[0])
        check("reset", False)
        rng = np.random.default_rng(INDEX[name])
        for s in range(STEPS_A):
            step(actions(rng, W * n, lateral))
            check(s, True)
        if again:  # several worlds end their episode on the same step: one imgenv_reset_worlds call
            ks = [0, W - 1][:len(again)]
            for k, lay in zip(ks, again):
                cpus[k].reset(lay)
            for g in gpus:
                g.reset_worlds(ks, again)
            check("listed reset", False)
        for g in gpus:
            g.timing(1)
        for s in range(STEPS_A, STEPS_A + STEPS_B):
            step(actions(rng, W * n, lateral))
            check(s, True)
        for g in gpus:
            timing.append(g.timing_read())
            g.timing(0)
        return fails, seen, timing
    finally:
        for w in cpus + gpus:
            w.close()
