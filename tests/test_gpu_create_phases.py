"""imgenv_create's phases on the device (csrc/imgenv_hip.hip: create_*; the plan they follow is checked on the CPU, test_create_plan.py).

The smallest handles that reach every phase variant -- 2 worlds x 2 robots x 1 pedestrian, 48 x 48 views -- are created, reset and
stepped twice against one oracle per world at the suite's usual bars (parity.py).  The arena's pointers are compared with the
offsets tests/host/create_plan_check.cpp derives by hand for its configuration 1 (4 robots, state_dim 3, 181 beams, max_ped 3: the
same byte sizes), in the working arena and, under IMGENV_FLAG_FULL_REWRITE, in the public one.  A create that is refused after the
first allocations in the old order (out_arena one byte short) must answer EINVAL with its text and leave the process able to
create and step a valid handle."""
import ctypes as C

import numpy as np
import pytest

from parity import EXTRAS, compare
from scenarios import random_actions, small_world
from test_gpu_multiworld import _run, _stack_params

pytestmark = pytest.mark.gpu

# configuration 1 of tests/host/create_plan_check.cpp: every array's offset in plan_arena's order, derived by hand there
NAMES = ["vector_states", "view_maps", "sensor_maps", "lasers_raw", "lasers", "ped_vector_states", "ped_maps", "is_collisions", "is_arrives",
         "step_ds", "ped_min_dists", "base_rewards", "base_dones", "rewards", "dones", "dones_info", "is_clean", "robot_pose", "ped_state",
         "counters", "records", "paper_rewards", "step_rewards", "step_dones", "step_dones_info", "step_is_clean", "step_is_arrives",
         "step_is_collisions", "step_all_down", "hits_x", "hits_y", "angular_map"]
OFFSETS = [0, 256, 9472, 27904, 30976, 36864, 37376, 147968, 148224, 148480, 148736, 148992, 149248, 149504, 149760, 150016, 150272, 150528,
           150784, 151040, 151296, 151552, 151808, 152064, 152320, 152576, 152832, 153088, 153344, 153600, 153856, 154112]
TOTAL = 154368
CASE = dict(beams=181, max_ped=3, n_obstacles=2, grid_size=100, clearance=0.6)


@pytest.fixture(scope="module")
def worlds():
    import torch
    assert torch.cuda.is_available()
    from img_env_amd.world import World
    from oracle_binding import OracleWorld, build_oracle
    build_oracle()
    return World, OracleWorld


def _handle(World, **over):
    grid, params, lay0 = small_world(2, 1, seed=71, **CASE)
    lays = [lay0, small_world(2, 1, seed=171, **CASE)[2]]
    return World(dict(_stack_params(params, 2), **over), grid), lays


def _pointers(w):
    from img_env_amd import _cabi
    o = _cabi.Out()
    assert w.lib.imgenv_outputs(w.h, C.byref(o)) == 0
    rec = C.c_void_p()
    assert w.lib.imgenv_records(w.h, C.byref(rec), None) == 0
    return {n: (rec.value if n == "records" else getattr(o, n)) for n in NAMES}


def test_arena_pointers_lie_at_the_planned_offsets(worlds):
    World, _ = worlds
    from img_env_amd import _cabi
    for flags in (0, _cabi.FLAG_AGENT_STATE_EXTRAS):
        w, _ = _handle(World, flags=flags)
        try:
            base, ptr = w.arena.data_ptr(), _pointers(w)
            if not flags:
                assert w.arena.numel() == TOTAL
                want = dict(zip(NAMES, OFFSETS))
                assert all(not ptr[n] for n in EXTRAS)
                assert {n: ptr[n] - base for n in NAMES if n not in EXTRAS} == {n: want[n] for n in NAMES if n not in EXTRAS}
            else:  # (configuration 2 there: the three extras have their arrays, and nothing in front of them has moved)
                assert w.arena.numel() == 161024
                assert [ptr[n] - base for n in NAMES[:30]] == OFFSETS[:30] and [ptr[n] - base for n in EXTRAS[1:]] == [156672, 159744]
        finally:
            w.close()


def test_full_rewrite_pointers_lie_in_the_public_arena_at_the_same_offsets(worlds):
    World, _ = worlds
    w, lays = _handle(World, output_guard="copy")
    try:
        base, ptr = w.arena.data_ptr(), _pointers(w)
        want = dict(zip(NAMES, OFFSETS))
        shown = {n: p - base for n, p in ptr.items() if p and n != "records"}
        assert sorted(shown) == sorted(n for n in NAMES if n not in EXTRAS and n != "records")
        assert shown == {n: want[n] for n in shown}
        assert not 0 <= ptr["records"] - base < TOTAL  # the records stay in the private arena
        w.reset(lays)
        w.step(random_actions(np.random.default_rng(1), 4))
        assert np.isfinite(w.snapshot()["vector_states"]).all()
    finally:
        w.close()


VARIANTS = {
    "composed": dict(flags=2),
    "stamped": dict(flags=4),
    "sum": dict(flags=512),
    "shrunk_image_big_view_taps": dict(image_size=(24, 24)),
    "pedscene_two_worlds_crowd_ahead": dict(scene="pedscene", relation_ped_robo=0, grid_size=88),
    "extras": dict(flags=16),
    "check_outputs": dict(output_guard="check"),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_each_phase_variant_resets_and_steps_like_the_oracle(worlds, variant):
    World, OracleWorld = worlds
    kw = dict(CASE, **VARIANTS[variant])
    fails, snap, cpus = _run(World, OracleWorld, 2, 2, 1, 2, {}, seed=71, **kw)
    assert not fails, fails[:3]
    want_mode = {"composed": (3, 0), "stamped": (3, 1), "sum": (3, 2), "pedscene_two_worlds_crowd_ahead": (16, 16)}.get(variant)
    if want_mode:  # (imgenv_layer_mode: the layer in bits 0-1, 16 = a crowd stepped a step ahead) the variant is the one it says
        grid, params, _ = small_world(2, 1, seed=71, **kw)
        w = World(_stack_params(params, 2), grid)
        try:
            assert w.lib.imgenv_layer_mode(w.h) & want_mode[0] == want_mode[1]
        finally:
            w.close()
    if variant == "extras":
        for k, c in enumerate(cpus):
            bad = compare({f: snap[f][2 * k:2 * k + 2] for f in EXTRAS}, c, EXTRAS)
            assert not bad, (k, bad)


def test_a_create_refused_behind_the_plan_leaves_the_process_able_to_create(worlds):
    World, _ = worlds
    import torch
    from img_env_amd import _cabi
    grid, params, lay0 = small_world(2, 1, seed=71, **CASE)
    params = _stack_params(params, 2)
    lib = _cabi.load_library()
    cfg, keep = _cabi.make_cfg(dict(params, device=0))
    nbytes = lib.imgenv_arena_bytes(C.byref(cfg))
    assert nbytes == TOTAL
    arena = torch.zeros(int(nbytes), dtype=torch.uint8, device="cuda:0")
    cfg.out_arena, cfg.out_arena_bytes = arena.data_ptr(), nbytes - 1
    g = np.ascontiguousarray(grid, np.uint8)
    h = C.c_void_p()
    assert lib.imgenv_create(C.byref(cfg), g.ctypes.data, g.shape[0], g.shape[1], C.byref(h)) == _cabi.EINVAL
    assert lib.imgenv_last_error().decode() == "out_arena too small: 154367 < 154368"
    assert not h.value
    w = World(params, grid)
    try:
        w.reset([lay0, small_world(2, 1, seed=171, **CASE)[2]])
        w.step(random_actions(np.random.default_rng(2), 4))
        assert np.isfinite(w.snapshot()["vector_states"]).all()
    finally:
        w.close()
