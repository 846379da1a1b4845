"""What a host-placed reset chooses for its worlds -- the map and the recorded crowd its placement's seed draws under the
"placement" policies -- on its way from the entry point to the launches: imgenv_reset_worlds_spawn (a list that is not ascending),
imgenv_step_autoreset (the finished worlds, sorted, from seed0 + q), the n_worlds = 1 delegation to the whole-handle reset, and a
refused call in between.  No single bank's test crosses this plumbing with both banks at once.

The checker is the explicit path: a twin handle under "keep" whose worlds are put on the same maps and sets with set_world_maps /
set_world_tracks and then reset with the same placements through reset_worlds -- sensor_maps, vector_states and ped_vector_states
equal byte for byte.  Which map and set a seed draws is computed here, without the device (_cabi.map_for_placement /
_cabi.tracks_for_placement).

All cases: 4 worlds x 2 robots x 2 pedestrians of a dataset scene on a 40 x 40 map at the handle's resolution, a bank of 3 maps
(2 added), 3 track sets of 4 records."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, R, P, CAP, N_OBS, DT, RES = 4, 2, 2, 4, 1, 0.25, 0.25
N_MAPS = N_SETS = 3
FIELDS = ("sensor_maps", "vector_states", "ped_vector_states")
U64 = (1 << 64) - 1


def _grids():
    """three maps that differ in what a robot sees: a border and one wall each, at another place"""
    out = []
    for m in range(N_MAPS):
        g = np.full((40, 40), 255, np.uint8)
        g[:2] = g[-2:] = 0
        g[:, :2] = g[:, -2:] = 0
        g[8 + 10 * m:11 + 10 * m, 6:34] = 0
        out.append(g)
    return out


def _sets():
    """three sets of straight walks, lengths 1 .. 4 mixed; the records behind a pedestrian's length hold junk that must never show"""
    rng = np.random.default_rng(5)
    out = []
    for lens in ([4, 1], [2, 4], [1, 3]):
        d = np.full((P, CAP, 5), 777.0)
        for j in range(P):
            x0, y0 = rng.uniform(3.0, 7.0, 2)
            vx, vy = rng.uniform(-0.5, 0.5, 2)
            for q in range(lens[j]):
                d[j, q] = [x0 + vx * DT * q, y0 + vy * DT * q, np.arctan2(vy, vx), vx if q else 0.0, vy if q else 0.0]
        out.append((d, np.asarray(lens, np.int32)))
    return out


def _cfg(peds):
    from img_env_amd import worldgen
    return worldgen.make_yaml_cfg(R, peds, _grids()[0], res=RES, scene="dataset" if peds else "rvoscene", time_max=1,
                                  n_obstacles=N_OBS, seed=9, dt=DT)


def _handle(cfg, n_worlds, policy, tracks=True):
    from img_env_amd import config
    from img_env_amd.vec_env import stack_params
    from img_env_amd.world import World
    w = World(stack_params(config.params_from_cfg(cfg), n_worlds), _grids())
    w.set_maps_policy(policy)
    if tracks:
        w.tracks_add(_sets())
        w.tracks_policy(policy)
    return w


def _draws(seeds):
    from img_env_amd import _cabi
    return ([_cabi.map_for_placement(s & U64, N_MAPS) for s in seeds], [_cabi.tracks_for_placement(s & U64, N_SETS) for s in seeds])


def _follow(twin, cfg, worlds, seeds, tracks=True):
    """the twin's explicit reset: the worlds put on the maps and sets the seeds draw, then the seeds' placements"""
    from img_env_amd import spawn
    maps, sets = _draws(seeds)
    twin.set_world_maps(worlds, maps)
    if tracks:
        twin.set_world_tracks(worlds, sets)
    twin.reset_worlds(worlds, [spawn.native_spawn(cfg, s & U64) for s in seeds])


def _same(a, b, where):
    sa, sb = a.snapshot(), b.snapshot()
    for f in FIELDS:
        if f in sa or f in sb:
            assert sa[f].shape == sb[f].shape and sa[f].tobytes() == sb[f].tobytes(), (where, f)
    assert a.world_maps().tolist() == b.world_maps().tolist(), where
    assert a.world_tracks().tolist() == b.world_tracks().tolist(), where


def _two_seeds(held_maps, held_sets):
    """two seeds whose map draws differ and whose set draws differ, each draw also another than what its world holds"""
    for s0 in range(2000, 2400):
        for s1 in range(s0 + 1, s0 + 40):
            (m0, m1), (t0, t1) = _draws([s0, s1])
            if m0 != m1 and t0 != t1 and m0 != held_maps[0] and m1 != held_maps[1] and t0 != held_sets[0] and t1 != held_sets[1]:
                return s0, s1
    raise AssertionError("no seeds")


def test_host_placed_resets_carry_their_draws_to_the_launches():
    import torch
    from img_env_amd import spawn
    cfg = _cfg(P)
    spawn_cfg = spawn.make_spawn_cfg(cfg)
    drawn, twin = _handle(cfg, W, "placement"), _handle(cfg, W, "keep")
    try:
        # every world once (a step needs them all): imgenv_reset_worlds_spawn over the whole list
        first = [1000 + k for k in range(W)]
        drawn.reset_worlds_spawn(range(W), spawn_cfg, first)
        _follow(twin, cfg, list(range(W)), first)
        maps, sets = _draws(first)
        assert drawn.world_maps().tolist() == maps and drawn.world_tracks().tolist() == sets
        _same(drawn, twin, "first reset")

        # (a) imgenv_reset_worlds_spawn of worlds [3, 1]: the list is not ascending, entry q belongs to worlds[q]
        s0, s1 = _two_seeds([maps[3], maps[1]], [sets[3], sets[1]])
        (m0, m1), (t0, t1) = _draws([s0, s1])
        drawn.reset_worlds_spawn([3, 1], spawn_cfg, [s0, s1])
        maps[3], maps[1], sets[3], sets[1] = m0, m1, t0, t1
        assert drawn.world_maps().tolist() == maps and drawn.world_tracks().tolist() == sets  # (worlds 0 and 2 untouched)
        _follow(twin, cfg, [3, 1], [s0, s1])
        _same(drawn, twin, "worlds [3, 1]")

        # (d) a refused call applies nothing and leaves nothing behind: the next reset, which brings no seeds, keeps map and set
        with pytest.raises(RuntimeError, match="listed twice"):
            drawn.reset_worlds_spawn([2, 2], spawn_cfg, [s0, s1])
        assert drawn.world_maps().tolist() == maps and drawn.world_tracks().tolist() == sets
        lay = spawn.native_spawn(cfg, 31)
        drawn.reset_worlds([2], [lay])
        twin.reset_worlds([2], [lay])
        assert drawn.world_maps().tolist() == maps and drawn.world_tracks().tolist() == sets
        _same(drawn, twin, "after a refused call")

        # (b) imgenv_step_autoreset: time_max 1 ends every world at once, with the second step (TimeLimitWrapper: elapsed > time_max);
        # the finished worlds come back sorted and world q of that list takes the draws of seed0 + q -- here wrapping past 2^64
        # (the list is the call's own: imgenv_autoreset_last answers for the device-side reset alone, IMGENV_ESTATE on this handle)
        seed0 = U64 - 1
        actions = torch.zeros((W * R, 3), dtype=torch.float32, device="cuda")
        _, finished = drawn.step_autoreset(actions, spawn_cfg, seed0)
        assert finished == []
        twin.step(actions)
        _same(drawn, twin, "a step")
        _, finished = drawn.step_autoreset(actions, spawn_cfg, seed0)
        assert finished == list(range(W))
        seeds = [seed0 + q for q in range(W)]
        maps, sets = _draws(seeds)
        assert drawn.world_maps().tolist() == maps and drawn.world_tracks().tolist() == sets
        twin.step(actions)
        _follow(twin, cfg, finished, seeds)
        _same(drawn, twin, "step_autoreset")
    finally:
        drawn.close()
        twin.close()


@pytest.mark.parametrize("peds", [P, 0], ids=["dataset_crowd", "no_pedestrians"])
def test_a_handle_of_one_world_takes_its_draws_through_the_whole_handle_reset(peds):
    """(c) n_worlds = 1: imgenv_reset_worlds_spawn(1, [0]) is the whole-handle reset underneath, and still lands on the seed's map
    and set; without pedestrians there is no track bank and the map alone is drawn"""
    from img_env_amd import spawn
    cfg = _cfg(peds)
    spawn_cfg = spawn.make_spawn_cfg(cfg)
    tracks = peds > 0
    drawn, twin = _handle(cfg, 1, "placement", tracks), _handle(cfg, 1, "keep", tracks)
    try:
        for seed in (s for s in range(3000, 3100) if _draws([s])[0][0] != 0 and _draws([s])[1][0] != 0):
            break
        for s in (seed, seed + 1, seed + 2):  # (three placements in a row: a world that moves between maps and sets)
            drawn.reset_worlds_spawn([0], spawn_cfg, [s])
            (m,), (t,) = _draws([s])
            assert drawn.world_maps().tolist() == [m] and drawn.world_tracks().tolist() == [t if tracks else -1]
            _follow(twin, cfg, [0], [s], tracks)
            _same(drawn, twin, s)
    finally:
        drawn.close()
        twin.close()
