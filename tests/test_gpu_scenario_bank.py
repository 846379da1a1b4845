"""The scenario bank (include/imgenv.h, "scenario bank"): recorded episodes as a bank inside ONE handle, replayed by the device-side
reset -- k_scenario_fill (img_env_amd/csrc/scenario_bank.h) fills the placement pool from the bank instead of sampling, everything
behind the pool is what it was.

Checkers.  Against the oracle: one OracleWorld per env, fed on every reset the bank's own scenario out of the PYTHON list -- the one
tests/scenario_bank_model.py names for the placement number ``autoreset_last()`` reports -- and compared after every step with the
bars of tests/parity.py; what the world received (``world_placement``) must be the bank's entry byte for byte.  Against the paths
that existed before: twin handles without a bank, every output byte equal.

All cases: a 200 x 200 grid, 48 x 48 views, 360 beams."""
import copy

import numpy as np
import pytest

from parity import compare
from scenario_bank_model import ScenarioModel

pytestmark = pytest.mark.gpu

VEC_FIELDS = ("is_collisions", "is_arrives", "view_maps", "sensor_maps", "vector_states", "lasers", "ped_maps",
              "ped_vector_states", "rewards", "dones", "dones_info", "robot_pose")  # the checker of tests/test_gpu_envs.py's vec envs
PLACEMENT_FIELDS = {"robot_pose": np.float64, "robot_goal": np.float64, "ped_pose": np.float64, "ped_goal": np.float64, "ped_traj": np.float64,
                    "ped_traj_len": np.int32, "obs_shape": np.int32, "obs_size": np.float32, "obs_pose": np.float64}
DT = 0.25


def make_cfg(R, P, n_obs, time_max, scene="rvoscene", **over):
    from img_env_amd import worldgen
    grid = worldgen.make_grid(200, 3)
    return worldgen.make_yaml_cfg(R, P, grid, scene=scene, time_max=time_max, n_obstacles=n_obs, seed=9, dt=DT, **over)


def env_slices(snap, k, R, P, fields):
    return {f: snap[f][k * P:(k + 1) * P] if f == "ped_state" else snap[f][k * R:(k + 1) * R] for f in fields}


def all_equal(a, b, where, skip=()):
    assert set(a) == set(b), where
    for f in a:
        if f in skip:
            continue
        assert a[f].shape == b[f].shape and a[f].tobytes() == b[f].tobytes(), (where, f)


def same_placement(got, want, where):
    """poses, goals, trajectories and obstacles, byte for byte"""
    for f, dt in PLACEMENT_FIELDS.items():
        a, b = np.ascontiguousarray(getattr(got, f), dt), np.ascontiguousarray(getattr(want, f), dt)
        assert a.tobytes() == b.tobytes(), (where, f, a, b)


def placement_bytes(lay):
    return b"".join(np.ascontiguousarray(getattr(lay, f), dt).tobytes() for f, dt in PLACEMENT_FIELDS.items())


def random_actions(rng, n, moving=True):
    a = np.zeros((n, 3), np.float32)
    if moving:
        a[:, 0], a[:, 1] = rng.uniform(0, 0.6, n), rng.uniform(-0.9, 0.9, n)
    return a


SHAPES = {  # E, R, P, obstacles, N, time_max, scene, random actions, resets wanted, steps at most
    # the queue wraps (N = 7 is coprime to the 5 envs and to the 256 slots) and every scenario runs: at least 2 N + 5 resets
    "a:5x2x3": (5, 2, 3, 2, 7, 4, "rvoscene", True, 2 * 7 + 5, 40),
    # robots at rest: the envs run into the time limit on the same step -- more finished worlds than a wavefront, and more than the
    # workgroups the chain's grids are sized for from the step before (plan_dev_reset: max(16, 4 x that)): the stride path
    "b:70x1x0": (70, 1, 0, 2, 7, 3, "rvoscene", False, 2 * 70, 12),
    # pedscene: the slot's obstacle segments (s_seg); needs n_worlds > 1
    "c:3x2x4": (3, 2, 4, 2, 7, 4, "pedscene", True, 2 * 3, 14),
    # no pedestrians, no obstacles, a one-entry bank: the `nob ? nob : 1` strides
    "d:2x1x0": (2, 1, 0, 0, 1, 4, "rvoscene", True, 2 * 2, 14),
}
CASES = [(s, "queue") for s in SHAPES] + [("a:5x2x3", "placement")]


# ---- 1. the device-side reset against oracles ----
@pytest.mark.parametrize("shape,policy", CASES)
def test_device_side_reset_replays_the_bank_and_matches_oracles(shape, policy):
    import torch
    from img_env_amd import spawn
    from img_env_amd.vec_env import VecImageEnv
    from oracle_binding import OracleWorld, build_oracle
    build_oracle()
    E, R, P, n_obs, N, time_max, scene, moving, want_resets, max_steps = SHAPES[shape]
    cfg = make_cfg(R, P, n_obs, time_max, scene=scene)
    bank = spawn.record_scenarios(cfg, N, 1000)
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, scenarios=bank, scenario_policy=policy)
    cpus = [OracleWorld(vec.params, vec.grid) for _ in range(E)]
    fields = VEC_FIELDS + ("ped_state",)
    model = ScenarioModel(E, N, seed0=vec._device_seed0)

    def check(where):
        snap = vec.world.snapshot()
        for k, c in enumerate(cpus):
            bad = compare(env_slices(snap, k, R, P, fields), env_slices(c.snapshot(), 0, R, P, fields), fields)
            assert not bad, (where, k, bad)

    try:
        assert vec.n_scenarios == N and (vec.world_scenarios() == -1).all()
        vec.reset()  # env k replays scenario k % N (a host reset), the device continues the queue at env_num
        model.set_policy(policy, first=E)
        for k in range(E):
            model.host_reset(k, k % N)
            cpus[k].reset(bank[k % N])
        assert np.array_equal(vec.world_scenarios(), model.cur)
        check("reset")
        rng = np.random.default_rng(2)
        resets, used, last_n, strided, expect = 0, set(model.cur.tolist()), 0, 0, 0
        for s in range(max_steps):
            a = random_actions(rng, E * R, moving)
            _, rew, done, info = vec.step(torch.as_tensor(a, device="cuda"))
            assert info["reset_envs"] is None
            worlds, first = vec.world.autoreset_last()
            assert first == expect, s
            rew, done = rew.cpu().numpy(), done.cpu().numpy()
            for k, c in enumerate(cpus):
                c.step(a[k * R:(k + 1) * R])
                ref = c.snapshot()  # what the step itself returned, also for the envs the library has already reset
                assert np.array_equal(rew[k * R:(k + 1) * R], ref["rewards"]), (s, k)
                assert np.array_equal(done[k * R:(k + 1) * R], ref["dones"]), (s, k)
            for q, k in enumerate(worlds):  # the envs that ended: the oracle takes the scenario out of the Python list
                sid = model.device_reset(k, first + q)
                assert 0 <= sid < N
                lay, serial = vec.world.world_placement(k, n_obs)
                assert serial == first + q, (s, k)
                same_placement(lay, bank[sid], (s, k, sid))
                cpus[k].reset(bank[sid])
                used.add(sid)
            assert np.array_equal(vec.world_scenarios(), model.cur), (s, model.cur)
            expect += len(worlds)
            resets += len(worlds)
            strided += int(len(worlds) > max(64, 16, 4 * last_n))  # more than a wavefront, and than the grid sized from the step before
            last_n = len(worlds)
            print(shape, policy, "step", s, "resets", len(worlds))
            check(s)
            if resets >= want_resets:
                break
        assert resets >= want_resets, resets
        if policy == "queue":
            assert used == set(range(N)), used  # one pass of N resets runs every scenario once
            assert model.cur.tolist() == vec.world_scenarios().tolist()
        else:
            assert len(used) > 1
        if shape.startswith("b:"):
            assert strided >= 1
    finally:
        vec.close()
        for c in cpus:
            c.close()


# ---- 2. the host path ----
def test_reset_worlds_scenarios_equals_reset_worlds_with_the_same_layouts():
    """a banked handle's reset_worlds_scenarios(envs, ids) against a twin WITHOUT a bank that gets reset_worlds(envs, [the same
    layouts]): every output byte after the reset and after 3 steps; the rows of the worlds that were not listed are untouched"""
    from img_env_amd import spawn
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, n_obs, N = 5, 2, 3, 2, 7
    cfg = make_cfg(R, P, n_obs, 100)
    bank = spawn.record_scenarios(cfg, N, 1000)
    mine = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, auto_reset=False, scenarios=bank)
    twin = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, auto_reset=False)
    rng = np.random.default_rng(5)
    try:
        mine.reset()
        twin.reset([bank[k % N] for k in range(E)])
        all_equal(mine.world.snapshot(), twin.world.snapshot(), "reset")
        assert mine.world_scenarios().tolist() == [k % N for k in range(E)] and (twin.world_scenarios() == -1).all()
        for s in range(2):
            a = random_actions(rng, E * R)
            mine.step(a)
            twin.step(a)
        before = mine.world.snapshot()
        mine.reset_envs([3, 1], scenario_ids=[6, 5])
        twin.reset_envs([3, 1], [bank[6], bank[5]])
        after = mine.world.snapshot()
        all_equal(after, twin.world.snapshot(), "reset of two envs")
        assert mine.world_scenarios().tolist() == [0, 5, 2, 6, 4]
        for f in before:  # the other worlds are untouched
            if f.startswith("step_") or f == "counters":
                continue
            rows = P if f == "ped_state" else R
            keep = np.ones(len(before[f]), bool)
            keep[1 * rows:2 * rows] = keep[3 * rows:4 * rows] = False
            assert np.array_equal(before[f][keep], after[f][keep], equal_nan=True), f
        for s in range(3):
            a = random_actions(rng, E * R)
            mine.step(a)
            twin.step(a)
            all_equal(mine.world.snapshot(), twin.world.snapshot(), "step %d behind the reset" % s)
        mine.world.reset_worlds([2], [bank[3]])  # an explicit batch: not from the bank, whatever it holds
        assert mine.world_scenarios().tolist() == [0, 5, -1, 6, 4]
    finally:
        mine.close()
        twin.close()


# ---- 3. switching the policy in mid-run ----
def test_switching_off_queue_off_in_mid_run_against_a_twin_that_never_had_a_bank():
    """OFF: the sampler's placement n depends on n alone -- equal serials are byte-equal between the two handles, before and after
    the QUEUE phase.  QUEUE: no reset takes a sampled placement.  The first reset behind each switch already obeys the new policy
    (the pool's slots, filled ahead under the old one, must not be handed out)."""
    import torch
    from img_env_amd import spawn
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, n_obs, N = 5, 2, 3, 2, 7
    cfg = make_cfg(R, P, n_obs, 4)
    bank = spawn.record_scenarios(cfg, N, 1000)
    bank_bytes = [placement_bytes(l) for l in bank]
    mine = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True)
    twin = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True)
    mine.world.scenarios_add(bank)  # a bank, policy OFF: the VecImageEnv keeps resetting from the sampler
    model = ScenarioModel(E, N, seed0=mine._device_seed0)
    rng = np.random.default_rng(7)
    sampled = {"mine": {}, "twin": {}}  # placement number -> bytes, for the placements each handle's SAMPLER handed out
    count = {"mine": 0, "twin": 0}

    def step(vec, who, a, phase):
        vec.step(torch.as_tensor(a, device="cuda"))
        worlds, first = vec.world.autoreset_last()
        assert first == count[who]
        for q, k in enumerate(worlds):
            lay, serial = vec.world.world_placement(k, n_obs)
            assert serial == first + q
            if who == "mine":
                sid = model.device_reset(k, serial)
                if phase == "queue":
                    assert sid == (3 + serial) % N, (serial, sid)
                    same_placement(lay, bank[sid], (phase, serial))
                else:
                    assert sid == -1
            if phase != "queue" or who == "twin":
                sampled[who][serial] = placement_bytes(lay)
                assert sampled[who][serial] not in bank_bytes
        count[who] += len(worlds)
        return len(worlds)

    try:
        mine.reset()
        twin.reset()
        for k in range(E):
            model.host_reset(k)
        all_equal(mine.world.snapshot(), twin.world.snapshot(), "reset")
        for s in range(6):  # OFF: the two handles are one
            a = random_actions(rng, E * R)
            step(mine, "mine", a, "off")
            step(twin, "twin", a, "off")
            all_equal(mine.world.snapshot(), twin.world.snapshot(), "off, step %d" % s)
            assert np.array_equal(mine.world_scenarios(), model.cur) and (model.cur == -1).all()
        assert count["mine"] >= E
        at = count["mine"]
        mine.world.scenarios_policy("queue", first=3)  # between two calls: the pool holds sampled placements for the next serials
        model.set_policy("queue", first=3, at=at)
        got = 0
        for s in range(11):
            a = random_actions(rng, E * R)
            got += step(mine, "mine", a, "queue")
            step(twin, "twin", a, "off")
            assert np.array_equal(mine.world_scenarios(), model.cur), (s, model.cur)
        assert got >= 2 * E and set(model.cur.tolist()) <= set(range(N))
        at2 = count["mine"]
        mine.world.scenarios_policy("off")
        model.set_policy("off", at=at2)
        got = 0
        for s in range(11):
            a = random_actions(rng, E * R)
            got += step(mine, "mine", a, "off again")
            step(twin, "twin", a, "off")
            assert np.array_equal(mine.world_scenarios(), model.cur), (s, model.cur)
        assert got >= 2 * E and (model.cur == -1).all()
        for s in range(10):  # (the twin's episodes end at their own pace: it catches up with the serials the banked handle reached)
            if count["twin"] >= count["mine"]:
                break
            step(twin, "twin", random_actions(rng, E * R), "off")
        both = sorted(set(sampled["mine"]) & set(sampled["twin"]))
        assert [n for n in both if n < at] == list(range(at)) and not [n for n in sampled["mine"] if at <= n < at2]
        assert len([n for n in both if n >= at2]) >= E, both  # the sampler's placements behind the queue phase, on both handles
        for n in both:
            assert sampled["mine"][n] == sampled["twin"][n], n
    finally:
        mine.close()
        twin.close()


# ---- 4. nothing waits for the host ----
def test_fill_and_policy_are_ordered_on_the_stream_without_any_synchronisation(monkeypatch):
    """30 rounds of torch op -> imgenv_step_autoreset_device queued behind a busy stream, never waited for -- with the policy switched
    in the middle of them -- against a twin that synchronises after every step: all bytes and world_scenarios() are equal"""
    import torch
    from img_env_amd import spawn
    from img_env_amd.vec_env import VecImageEnv
    from test_gpu_stream_order import _delay
    monkeypatch.setenv("IMGENV_OUTPUT_GUARD", "none")  # (the default guard synchronises during a handle's first calls)
    E, R, P, n_obs, N = 5, 2, 3, 2, 7
    cfg = make_cfg(R, P, n_obs, 4)
    bank = spawn.record_scenarios(cfg, N, 1000)
    mk = lambda: VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, scenarios=bank)
    run, twin = mk(), mk()
    try:
        rng = np.random.default_rng(6)
        acts = [torch.as_tensor(random_actions(rng, E * R), device="cuda") for s in range(30)]
        big = torch.randn(3072, 3072, device="cuda")
        twin.reset()
        seen = set()
        for s in range(30):
            if s == 14:
                twin.world.scenarios_policy("placement")
            twin.step(acts[s])
            torch.cuda.synchronize()
            seen |= set(twin.world_scenarios().tolist())
        assert seen == set(range(N))
        run.reset()
        torch.cuda.synchronize()
        keep = []
        for s in range(30):
            keep.append(_delay(big))
            if s == 14:
                run.world.scenarios_policy("placement")
            run.step(acts[s])
        torch.cuda.synchronize()
        all_equal(run.world.snapshot(), twin.world.snapshot(), "after 30 rounds")
        assert np.array_equal(run.world_scenarios(), twin.world_scenarios())
    finally:
        run.close()
        twin.close()


# ---- 5. together with the other device-side features ----
def test_recorded_episodes_beside_stacks_statistics_wrappers_a_map_bank_and_a_track_bank():
    """stacks, episode statistics, wrappers=True, a two-map bank (KEEP) and a dataset crowd with a track bank on one handle whose
    device-side resets replay a scenario bank: each feature's own model holds for 12 steps"""
    from img_env_amd import _cabi, spawn, worldgen
    from img_env_amd.vec_env import VecImageEnv
    from action_model import TABLE, ActionModel
    from episode_model import EpisodeModel
    from stack_model import StackModel, bits, depths
    from test_gpu_actions import TABLE8, WRAPPERS, check_post, host, raw_policy, same
    from test_gpu_episodes import device_arrays, same_arrays, step_inputs
    from test_gpu_track_bank import make_sets
    E, R, P, n_obs, N = 5, 2, 3, 2, 7
    cfg = make_cfg(R, P, n_obs, 4, scene="dataset", wrappers=WRAPPERS, discrete_action=True, discrete_actions=TABLE8, image_batch=2,
                   state_batch=3, laser_batch=2, max_ped=10)
    cfg["global_map"]["map_array"] = np.stack([worldgen.make_grid(200, 3), worldgen.make_grid(200, 4)])
    sets = make_sets(P, [[1, 2, 5], [5, 1, 2], [2, 5, 1]], 5, seed=11)
    bank = spawn.record_scenarios(cfg, N, 1000)
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, stack=True, episode_stats=True, wrappers=True,
                      map_policy="keep", ped_tracks=sets, tracks_policy="placement", info_track_sets=True, scenarios=bank)
    try:
        w = vec.world
        fields = ("sensor_maps", "vector_states", "lasers")
        stacks = {f: StackModel(k) for f, k in zip(fields, depths(2, 3, 2))}
        am = ActionModel(E * R, TABLE, table=TABLE8, clip=cfg["continuous_actions"])
        ep = EpisodeModel(E * R, cfg["control_hz"])
        model = ScenarioModel(E, N)
        vec.reset()
        model.set_policy("queue", first=E)
        for k in range(E):
            model.host_reset(k, k % N)
        snap = w.snapshot()
        for f in fields:
            stacks[f].reset(snap[f], np.ones(E * R, bool))
        ep.reset(np.ones(E * R, bool), np.zeros(E * R, np.int32))
        check_post(vec, "reset")
        track_sets = [0] * E  # (a bank-fed host reset without a seed keeps the world's choice: set 0)
        maps = [k % 2 for k in range(E)]
        assert vec.world_maps().tolist() == maps and vec.world_tracks().tolist() == track_sets
        assert np.array_equal(vec.world_scenarios(), model.cur)
        resets = 0
        for s in range(12):
            raw = raw_policy(snap["vector_states"], True)
            state, _, done, info = vec.step(raw)
            want = am.decode(raw)
            same(host(w.action_outputs["actions"]), want, "step %d actions" % s)
            same(host(info["speeds"]), am.speeds, "step %d speeds" % s)
            got = step_inputs(w)
            am.step_done(host(done))
            rows = host(info["all_down"]).astype(bool)
            am.reset(rows)
            ep.step(want, got["step_is_clean"], got["step_rewards"])
            ep.reset(rows, got["step_dones_info"])
            same_arrays(device_arrays(w), ep.arrays(), "step %d statistics" % s)
            snap = w.snapshot()
            for f in fields:
                wanted = stacks[f].update(snap[f], rows)
                mine = w.stack[f].cpu().numpy()
                assert (bits(mine) == bits(wanted.reshape(mine.shape))).all(), (s, f)
            check_post(vec, "step %d" % s)
            worlds, first = w.autoreset_last()
            for q, k in enumerate(worlds):
                sid = model.device_reset(k, first + q)
                lay, _ = w.world_placement(k, n_obs)
                same_placement(lay, bank[sid], (s, k))
                track_sets[k] = _cabi.tracks_for_placement(vec._device_seed0 + first + q, 3)
            resets += len(worlds)
            assert np.array_equal(vec.world_scenarios(), model.cur), s
            assert vec.world_maps().tolist() == maps, s  # KEEP: the worlds stay on the maps the episodes were recorded on
            assert info["track_sets"].tolist() == track_sets, s
        assert resets >= 2 * E
    finally:
        vec.close()


# ---- 6. a bank nobody uses ----
def test_a_bank_with_policy_off_is_invisible_and_a_plain_step_launches_what_it_launched():
    import torch
    from img_env_amd import spawn
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, n_obs, N = 5, 2, 3, 2, 7
    cfg = make_cfg(R, P, n_obs, 4)
    bank = spawn.record_scenarios(cfg, N, 1000)
    off = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True)
    off.world.scenarios_add(bank)
    plain = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True)
    queue = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, scenarios=bank)
    try:
        off.reset()
        plain.reset()
        all_equal(off.world.snapshot(), plain.world.snapshot(), "reset")
        rng = np.random.default_rng(8)
        resets = 0
        for s in range(6):
            a = torch.as_tensor(random_actions(rng, E * R), device="cuda")
            off.step(a)
            plain.step(a)
            assert off.world.launches() == plain.world.launches() > 0, s
            all_equal(off.world.snapshot(), plain.world.snapshot(), "auto-reset step %d" % s)
            resets += len(off.world.autoreset_last()[0])
        assert resets >= E and (off.world_scenarios() == -1).all()
        queue.reset()
        a = torch.zeros(E * R, 3, device="cuda")
        queue.world.step(a)  # the bank does not leak into a step
        plain.world.step(a)
        assert queue.world.launches() == plain.world.launches() > 0
        queue.step(a)
        plain.step(a)
        assert queue.world.launches() == plain.world.launches()  # ... nor into the chain: the fill is one launch either way
    finally:
        off.close()
        plain.close()
        queue.close()


# ---- 7. refusals ----
def test_refusals():
    import ctypes as C
    import torch
    from img_env_amd import _cabi, config, spawn
    from img_env_amd.vec_env import VecImageEnv, stack_params
    from img_env_amd.world import World
    E, R, P, n_obs, N = 3, 2, 3, 2, 4
    cfg = make_cfg(R, P, n_obs, 4)
    bank = spawn.record_scenarios(cfg, N, 1000)
    lib = _cabi.load_library()
    arrays = _cabi.pack_scenarios(bank, R, P, n_obs)

    def add(h, n=N, O=n_obs, **over):
        a = dict(arrays, **over)
        return lib.imgenv_scenarios_add(h, n, O, *[a[k].ctypes.data for k in arrays])

    ids = lambda *v: (C.c_int32 * len(v))(*v)
    zero = torch.zeros(E * R, 3, device="cuda")

    params = stack_params(config.params_from_cfg(cfg), 1)
    shard = World(dict(params, robot_begin=0, robot_end=1), config.load_map(cfg))
    try:
        assert add(shard.h) == _cabi.EINVAL and b"shard" in lib.imgenv_last_error()
    finally:
        shard.close()

    none = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True)
    try:  # a policy, a scenario reset, a question without a bank
        h = none.world.h
        assert lib.imgenv_scenarios_policy(h, _cabi.SCENARIOS_QUEUE, 0, None) == _cabi.ESTATE and b"no scenario bank" in lib.imgenv_last_error()
        assert lib.imgenv_scenarios_policy(h, _cabi.SCENARIOS_OFF, 0, None) == _cabi.ESTATE
        assert lib.imgenv_reset_worlds_scenarios(h, 1, ids(0), ids(0), None) == _cabi.ESTATE
        assert (none.world_scenarios() == -1).all()
        # bad banks: the handle stays without one
        assert add(h, n=0) == _cabi.EINVAL
        assert add(h, O=_cabi.SPAWN_MAX_OBST + 1) == _cabi.EINVAL and b"obstacles" in lib.imgenv_last_error()
        bad = arrays["robot_pose"].copy()
        bad[2, 1, 0] = np.nan
        assert add(h, robot_pose=bad) == _cabi.EINVAL and b"scenario 2, robot 1" in lib.imgenv_last_error() and b"finite" in lib.imgenv_last_error()
        bad = arrays["ped_pose"].copy()
        bad[1, 2, 2:] = 0.0
        assert add(h, ped_pose=bad) == _cabi.EINVAL and b"scenario 1, pedestrian 2" in lib.imgenv_last_error() and b"quaternion" in lib.imgenv_last_error()
        bad = arrays["ped_traj_len"].copy()
        bad[3, 0] = 3
        assert add(h, ped_traj_len=bad) == _cabi.EINVAL and b"length" in lib.imgenv_last_error()
        bad = arrays["obs_shape"].copy()
        bad[0, 1] = 9
        assert add(h, obs_shape=bad) == _cabi.EINVAL and b"scenario 0, obstacle 1" in lib.imgenv_last_error() and b"shape" in lib.imgenv_last_error()
        assert none.world.n_scenarios == 0 and lib.imgenv_scenarios_policy(h, _cabi.SCENARIOS_QUEUE, 0, None) == _cabi.ESTATE
        with pytest.raises(ValueError):  # a cast mismatch at add: the layouts hold another number of robots
            none.world.scenarios_add(spawn.record_scenarios(make_cfg(R + 1, P, n_obs, 4), 2, 5))
        none.reset()
        none.step(zero)
        assert add(h) == _cabi.ESTATE and b"after the first" in lib.imgenv_last_error()  # the pool exists
    finally:
        none.close()

    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, scenarios=bank)
    try:
        h = vec.world.h
        assert add(h) == _cabi.ESTATE and b"already" in lib.imgenv_last_error()  # a second add
        assert lib.imgenv_scenarios_policy(h, 3, 0, None) == _cabi.EINVAL
        assert lib.imgenv_reset_worlds_scenarios(h, 1, ids(0), ids(N), None) == _cabi.EINVAL and b"out of range" in lib.imgenv_last_error()
        assert lib.imgenv_reset_worlds_scenarios(h, 1, ids(0), ids(-1), None) == _cabi.EINVAL
        assert lib.imgenv_reset_worlds_scenarios(h, 1, ids(E), ids(0), None) == _cabi.EINVAL  # a bad world
        assert lib.imgenv_reset_worlds_scenarios(h, 2, ids(1, 1), ids(0, 1), None) == _cabi.EINVAL and b"twice" in lib.imgenv_last_error()
        with pytest.raises(ValueError):
            vec.reset_envs([0, 1], scenario_ids=[0, N + 3])
        vec.reset()
        assert vec.world_scenarios().tolist() == [0, 1, 2]  # nothing of the refused calls was applied
        # a cast mismatch at the auto-reset call: a spawn cfg with another number of obstacles
        other = spawn.make_spawn_cfg(make_cfg(R, P, n_obs + 1, 4))
        with pytest.raises(RuntimeError, match="the scenario bank"):
            vec.world.step_autoreset_device(zero, other, vec._device_seed0)
        vec.world.scenarios_policy("off")  # ... which the sampler would take
        vec.world.scenarios_policy("queue", first=E)
        vec.step(zero)
    finally:
        vec.close()

    # the VecImageEnv argument errors
    with pytest.raises(ValueError, match="device_reset=True or auto_reset=False"):
        VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, scenarios=bank)
    with pytest.raises(ValueError, match="device_reset=True or auto_reset=False"):
        VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=True, scenarios=bank)
    with pytest.raises(ValueError, match="scenario_policy"):
        VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, scenarios=bank, scenario_policy="cycle")
    plain = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, auto_reset=False)
    try:
        with pytest.raises(ValueError):
            plain.reset_envs([0], scenario_ids=[0])
    finally:
        plain.close()
