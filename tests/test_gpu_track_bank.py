"""The track bank (include/imgenv.h, "track bank"): the recorded crowds of the dataset pedestrian scene as a bank inside ONE handle,
one set per world and episode, installed by k_tracks_install (img_env_amd/csrc/track_bank.h) in every reset chain -- the host's
(imgenv_reset_worlds_spawn, imgenv_step_autoreset, an explicit batch without ped_traj_v) and the device's own
(imgenv_step_autoreset_device), where the host never learns that an episode ended.

Two checkers.  Against the oracle: one OracleWorld per env, fed the placement its world really received and, over it, the tracks
of the set ``world_tracks()`` names (EnvPos.init_ped_dataset), compared after every step and reset with the bars of
tests/parity.py.  Against the path that existed before: a twin handle without a bank that gets the same placements with the
set's tracks uploaded in the batch -- every output byte equal ("bank equals upload").  Which set a reset takes is
tests/tracks_model.py's business.

All cases: a 200 x 200 grid, 48 x 48 views, 360 beams; sets of up to 5 records with lengths 1, 2 and 5 mixed per pedestrian."""
import copy

import numpy as np
import pytest

from parity import compare
from tracks_model import TracksModel, replayed_state

pytestmark = pytest.mark.gpu

VEC_FIELDS = ("is_collisions", "is_arrives", "view_maps", "sensor_maps", "vector_states", "lasers", "ped_maps",
              "ped_vector_states", "rewards", "dones", "dones_info", "robot_pose")  # the checker of tests/test_gpu_envs.py's vec envs
N_OBS = 2
DT = 0.25


def dataset_cfg(R, P, time_max, **over):
    from img_env_amd import worldgen
    grid = worldgen.make_grid(200, 3)
    return worldgen.make_yaml_cfg(R, P, grid, scene="dataset", time_max=time_max, n_obstacles=N_OBS, seed=9, dt=DT, **over)


def make_sets(P, lengths, cap, seed, box=(8.0, 17.0), speed=0.5):
    """len(lengths) sets of P straight walks inside ``box``: (series [P, cap, 5], true lengths [P]); the records behind a
    pedestrian's length hold junk that must never show"""
    rng = np.random.default_rng(seed)
    out = []
    for lens in lengths:
        d = np.full((P, cap, 5), 777.0)
        for j in range(P):
            x0, y0 = rng.uniform(box[0], box[1], 2)
            vx, vy = rng.uniform(-speed, speed, 2)
            for q in range(int(lens[j])):
                d[j, q] = [x0 + vx * DT * q, y0 + vy * DT * q, np.arctan2(vy, vx), vx if q else 0.0, vy if q else 0.0]
        out.append((d, np.asarray(lens, np.int32)))
    return out


def with_tracks(layout, packed, s):
    """EnvPos.init_ped_dataset (reset_helper.py:417-432) with set ``s``: the recorded tracks over the sampler's pedestrians"""
    _, _, pose, traj, traj_v, length = packed
    lay = copy.copy(layout)
    lay.ped_pose, lay.ped_traj, lay.ped_traj_v, lay.ped_traj_len = pose[s].copy(), traj[s].copy(), traj_v[s].copy(), length[s].copy()
    return lay


def env_slices(snap, k, R, P, fields):
    return {f: snap[f][k * P:(k + 1) * P] if f == "ped_state" else snap[f][k * R:(k + 1) * R] for f in fields}


def all_equal(a, b, where, skip=()):
    assert set(a) == set(b), where
    for f in a:
        if f in skip:
            continue
        assert a[f].shape == b[f].shape and a[f].tobytes() == b[f].tobytes(), (where, f)


SHAPES = {  # E, R, P, time_max, steps, lengths of the three sets, cap, where the tracks run, random actions
    # Pw * stride = 15 is odd: world 1's rows of the tables are 8-byte aligned only; length 1 holds its record from step 0
    "5x2x3": (5, 2, 3, 4, 13, [[1, 2, 5], [5, 1, 2], [2, 5, 1]], 5, (8.0, 17.0), True),
    # robots at rest far from the tracks: the envs run into the time limit on the same step -- more finished worlds than the
    # workgroups the chain's grid is sized for from the last step's count (plan_dev_reset: max(16, 4 x that)): the stride path
    # (a few placements touch a wall and end at once, so a wave is not quite all 70)
    "70x1x2": (70, 1, 2, 3, 12, [[1, 4], [4, 2], [2, 1]], 4, (0.4, 0.7), False),
}


# ---- 1. the device-side reset against oracles ----
@pytest.mark.parametrize("policy", ["keep", "placement", "cycle"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_device_side_reset_of_recorded_crowds_matches_oracles(shape, policy):
    import torch
    from img_env_amd import _cabi, spawn
    from img_env_amd.vec_env import VecImageEnv
    from oracle_binding import OracleWorld, build_oracle
    build_oracle()
    E, R, P, time_max, steps, lengths, cap, box, moving = SHAPES[shape]
    cfg = dataset_cfg(R, P, time_max)
    sets = make_sets(P, lengths, cap, seed=11, box=box, speed=0.5 if moving else 0.3)
    packed = _cabi.pack_track_sets(sets, P)
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, ped_tracks=sets, tracks_policy=policy, tracks_repeat=1)
    cpus = [OracleWorld(vec.params, vec.grid) for _ in range(E)]
    fields = VEC_FIELDS + ("ped_state",)
    model = TracksModel(E, len(sets), policy, 1)

    def check(where):
        snap = vec.world.snapshot()
        for k, c in enumerate(cpus):
            bad = compare(env_slices(snap, k, R, P, fields), env_slices(c.snapshot(), 0, R, P, fields), fields)
            assert not bad, (where, k, bad)

    try:
        assert vec.n_track_sets == 3 and (vec.world_tracks() == -1).all()
        if policy == "keep":  # nobody else spreads the envs over the sets
            vec.set_world_tracks(range(E), [k % 3 for k in range(E)])
            model.select(range(E), [k % 3 for k in range(E)])
        seed0, dev0 = vec._spawn_seed, vec._device_seed0
        vec.reset()  # the first episodes: placed by the host-side library spawn (imgenv_reset_worlds_spawn), fed by the bank
        for k in range(E):
            model.reset(k, seed0 + k)
        tr = vec.world_tracks()
        assert np.array_equal(tr, model.cur)
        for k in range(E):
            cpus[k].reset(with_tracks(spawn.native_spawn(cfg, seed0 + k), packed, tr[k]))
        check("reset")
        rng = np.random.default_rng(2)
        resets, used, last_n, strided = 0, set(tr.tolist()), 0, 0
        for s in range(steps):
            a = np.zeros((E * R, 3), np.float32)
            if moving:
                a[:, 0], a[:, 1] = rng.uniform(0, 0.6, E * R), rng.uniform(-0.9, 0.9, E * R)
            _, rew, done, info = vec.step(torch.as_tensor(a, device="cuda"))
            assert info["reset_envs"] is None
            worlds, first = vec.world.autoreset_last()
            rew, done = rew.cpu().numpy(), done.cpu().numpy()
            for k, c in enumerate(cpus):
                c.step(a[k * R:(k + 1) * R])
                ref = c.snapshot()  # what the step itself returned, also for the envs the library has already reset
                assert np.array_equal(rew[k * R:(k + 1) * R], ref["rewards"]), (s, k)
                assert np.array_equal(done[k * R:(k + 1) * R], ref["dones"]), (s, k)
            lays = {}
            for q, k in enumerate(worlds):  # the envs that ended: the placement the device drew, the set the chain installed
                lays[k], serial = vec.world.world_placement(k, N_OBS)
                assert serial == first + q, (s, k)
                model.reset(k, dev0 + serial)
            tr = vec.world_tracks()
            assert np.array_equal(tr, model.cur), (s, tr, model.cur)
            for k in worlds:
                cpus[k].reset(with_tracks(lays[k], packed, tr[k]))
                used.add(int(tr[k]))
            resets += len(worlds)
            strided += int(len(worlds) > max(16, 4 * last_n))  # (the grid is sized from the count of the step before)
            last_n = len(worlds)
            print(shape, policy, "step", s, "resets", len(worlds))
            check(s)
            if policy == "keep" and s == 1:  # a choice made in mid-episode waits for the env's next reset
                vec.set_world_tracks([0, E - 1], [2, 0])
                model.select([0, E - 1], [2, 0])
                assert np.array_equal(vec.world_tracks(), tr)
        assert resets >= 2 * E and used == {0, 1, 2}, (resets, used)
        if not moving:
            assert strided >= 2  # the install's workgroups strode over the list, at both waves of time limits
    finally:
        vec.close()
        for c in cpus:
            c.close()


# ---- 2. the host paths: bank equals upload ----
@pytest.mark.parametrize("policy", ["keep", "placement", "cycle"])
def test_host_side_resets_from_the_bank_equal_the_same_tracks_uploaded(policy):
    """imgenv_reset_worlds_spawn, imgenv_step_autoreset and an explicit batch with ped_traj_v == NULL on a banked handle, against a
    twin WITHOUT a bank that is stepped by imgenv_step and reset by imgenv_reset_worlds with the same placements and the set's
    tracks in the batch: every output byte, after each reset and over the steps behind it"""
    import torch
    from img_env_amd import _cabi, spawn
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, time_max, _, lengths, cap, box, _ = SHAPES["5x2x3"]
    cfg = dataset_cfg(R, P, time_max)
    sets = make_sets(P, lengths, cap, seed=11, box=box)
    packed = _cabi.pack_track_sets(sets, P)
    bank = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=True, ped_tracks=sets, tracks_policy=policy, tracks_repeat=2)
    twin = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, auto_reset=False)
    model = TracksModel(E, len(sets), policy, 2)
    skip = tuple(f for f in bank.world.out if f.startswith("step_"))  # (the step's own scalars: only the auto-reset call keeps them)

    def same(where):
        all_equal(bank.world.snapshot(), twin.world.snapshot(), where, skip)

    def follow(envs, seeds, drawn=True):
        """the twin's reset of ``envs``: the placements of ``seeds`` with the tracks of the sets the bank installed (``drawn``: the
        bank's reset knew the seeds, so "placement" draws from them)"""
        for k, sd in zip(envs, seeds):
            model.reset(k, sd if drawn else None)
        tr = bank.world_tracks()
        assert np.array_equal(tr, model.cur), (tr, model.cur)
        twin.reset_envs(envs, [with_tracks(spawn.native_spawn(cfg, sd), packed, tr[k]) for k, sd in zip(envs, seeds)])

    try:
        if policy == "keep":
            bank.set_world_tracks(range(E), [k % 3 for k in range(E)])
            model.select(range(E), [k % 3 for k in range(E)])
        seed0 = bank._spawn_seed
        bank.reset()  # imgenv_reset_worlds_spawn of every env
        follow(list(range(E)), [seed0 + k for k in range(E)])
        same("reset")
        rng = np.random.default_rng(3)
        n_eps, resets, used = E, 0, set()
        for s in range(12):  # imgenv_step_autoreset (the time limit ends an episode on its 5th step: two waves)
            a = np.zeros((E * R, 3), np.float32)
            a[:, 0], a[:, 1] = rng.uniform(0, 0.6, E * R), rng.uniform(-0.9, 0.9, E * R)
            _, _, _, info = bank.step(torch.as_tensor(a, device="cuda"))
            twin.step(torch.as_tensor(a, device="cuda"))
            fin = list(info["reset_envs"])
            if fin:
                follow(fin, [seed0 + n_eps + q for q in range(len(fin))])
            n_eps += len(fin)
            resets += len(fin)
            used |= set(bank.world_tracks().tolist())
            same("autoreset step %d" % s)
        assert resets >= 2 * E and len(used) > 1, (resets, used)
        bank.reset_envs([1, 3])  # imgenv_reset_worlds_spawn of two envs in mid-episode
        follow([1, 3], [seed0 + n_eps, seed0 + n_eps + 1])
        n_eps += 2
        same("reset of two envs")
        lay = spawn.native_spawn(cfg, 4242)  # an explicit batch with ped_traj_v == NULL (and no seed: "placement" keeps the choice)
        assert lay.ped_traj_v is None
        bank.world.reset_worlds([2], [lay])
        follow([2], [4242], drawn=False)
        same("explicit batch without tracks")
        for s in range(6):
            a = np.zeros((E * R, 3), np.float32)
            a[:, 0], a[:, 1] = rng.uniform(0, 0.6, E * R), rng.uniform(-0.9, 0.9, E * R)
            bank.world.step(a)
            twin.world.step(a)
            same("step %d behind the explicit batch" % s)
    finally:
        bank.close()
        twin.close()


# ---- 3. mixing explicit tracks and the bank ----
def test_a_batch_with_tracks_bypasses_the_bank_and_a_choice_waits_for_the_next_reset():
    from img_env_amd import _cabi, spawn
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, _, _, lengths, cap, box, _ = SHAPES["5x2x3"]
    cfg = dataset_cfg(R, P, 100)
    sets = make_sets(P, lengths, cap, seed=11, box=box)
    packed = _cabi.pack_track_sets(sets, P)
    own = _cabi.pack_track_sets(make_sets(P, [[3, 3, 2]], 3, seed=77, box=(3.0, 6.0)), P)  # tracks no set of the bank holds
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=True, auto_reset=False, ped_tracks=sets, tracks_policy="cycle")
    model = TracksModel(E, 3, "cycle", 1)
    zero = np.zeros((E * R, 3), np.float32)

    def ped_state(k):
        return vec.world.snapshot()["ped_state"][k * P:(k + 1) * P]

    def replays(k, pk, s, step, where):
        want = replayed_state(pk[2][s], pk[3][s], pk[4][s], pk[5][s], step)  # (pk: pack_track_sets' arrays)
        got = ped_state(k)
        col = slice(0, 2) if step == 0 else slice(0, 4)
        assert np.array_equal(got[:, col], want[:, col]), (where, got, want)

    try:
        vec.reset()
        for k in range(E):
            model.reset(k)
        vec.reset_envs([1])  # env 1 is one reset ahead: on set 1, its count at 2
        model.reset(1)
        assert np.array_equal(vec.world_tracks(), model.cur) and model.cur.tolist() == [0, 1, 0, 0, 0]
        vec.world.step(zero)
        replays(1, packed, 1, 1, "bank set 1")
        before = vec.world.snapshot()
        vec.world.reset_worlds([1], [with_tracks(spawn.native_spawn(cfg, 99), own, 0)])  # its own tracks, in mid-run
        model.reset_explicit(1)
        after = vec.world.snapshot()
        assert vec.world_tracks().tolist() == [0, -1, 0, 0, 0]
        replays(1, own, 0, 0, "own tracks, reset")
        for f in before:  # the other worlds are untouched
            if f.startswith("step_") or f == "counters":
                continue
            rows = P if f == "ped_state" else R
            keep = np.ones(len(before[f]), bool)
            keep[1 * rows:2 * rows] = False
            assert np.array_equal(before[f][keep], after[f][keep], equal_nan=True), f
        for step in (1, 2, 3, 4):
            vec.world.step(zero)
            replays(1, own, 0, step, "own tracks")
            replays(0, packed, 0, step + 1, "bank set 0 beside it")
        vec.reset_envs([1, 2])  # bank-fed again: env 1's count did not move with the explicit batch (2 -> set 2), env 2 is at 1
        model.reset(1)
        model.reset(2)
        assert model.cur.tolist() == [0, 2, 1, 0, 0] and np.array_equal(vec.world_tracks(), model.cur)
        replays(1, packed, 2, 0, "bank set 2")
        # a choice between two steps does not touch the running episode
        vec.world.tracks_policy("keep")
        model.set_policy("keep")
        vec.world.step(zero)
        vec.set_world_tracks([1, 0], [0, 1])
        model.select([1, 0], [0, 1])
        assert np.array_equal(vec.world_tracks(), model.cur)
        vec.world.step(zero)
        replays(1, packed, 2, 2, "set 2 runs on")
        replays(2, packed, 1, 2, "set 1 runs on")
        vec.reset_envs([1])
        model.reset(1)
        assert model.cur[1] == 0 and np.array_equal(vec.world_tracks(), model.cur)
        replays(1, packed, 0, 0, "the choice at the next reset")
    finally:
        vec.close()


# ---- 4. nothing waits for the host ----
def test_install_is_ordered_on_the_stream_without_any_synchronisation(monkeypatch):
    """30 rounds of imgenv_step_autoreset_device queued behind a busy stream, never waited for, against a twin that synchronises
    after every step: final outputs and world_tracks() are equal"""
    import torch
    from img_env_amd.vec_env import VecImageEnv
    from test_gpu_stream_order import _delay
    monkeypatch.setenv("IMGENV_OUTPUT_GUARD", "none")  # (the default guard synchronises during a handle's first calls)
    E, R, P, time_max, _, lengths, cap, box, _ = SHAPES["5x2x3"]
    cfg = dataset_cfg(R, P, time_max)
    sets = make_sets(P, lengths, cap, seed=11, box=box)
    mk = lambda: VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, ped_tracks=sets, tracks_policy="placement")
    run, twin = mk(), mk()
    try:
        rng = np.random.default_rng(6)
        acts = []
        for s in range(30):
            a = np.zeros((E * R, 3), np.float32)
            a[:, 0], a[:, 1] = rng.uniform(0, 0.6, E * R), rng.uniform(-0.9, 0.9, E * R)
            acts.append(torch.as_tensor(a, device="cuda"))
        big = torch.randn(3072, 3072, device="cuda")
        twin.reset()
        seen = set()
        for s in range(30):
            twin.step(acts[s])
            torch.cuda.synchronize()
            seen |= set(twin.world_tracks().tolist())
        assert seen == {0, 1, 2}
        run.reset()
        torch.cuda.synchronize()
        keep = []
        for s in range(30):
            keep.append(_delay(big))
            run.step(acts[s])
        torch.cuda.synchronize()
        all_equal(run.world.snapshot(), twin.world.snapshot(), "after 30 rounds")
        assert np.array_equal(run.world_tracks(), twin.world_tracks())
    finally:
        run.close()
        twin.close()


# ---- 5. together with the other device-side features ----
def test_recorded_crowds_beside_stacks_statistics_wrappers_and_a_map_bank():
    """stacks, episode statistics, wrappers=True and a map bank on one dataset handle with device-side resets: each feature's own
    model holds for 12 steps, the maps and the track sets follow their placement draws"""
    from img_env_amd import _cabi, worldgen
    from img_env_amd.vec_env import VecImageEnv
    from action_model import TABLE, ActionModel
    from episode_model import EpisodeModel
    from stack_model import StackModel, bits, depths
    from test_gpu_actions import TABLE8, WRAPPERS, check_post, host, raw_policy, same
    from test_gpu_episodes import device_arrays, same_arrays, step_inputs
    E, R, P, _, _, lengths, cap, box, _ = SHAPES["5x2x3"]
    cfg = dataset_cfg(R, P, 4, wrappers=WRAPPERS, discrete_action=True, discrete_actions=TABLE8, image_batch=2, state_batch=3, laser_batch=2,
                      max_ped=10)
    cfg["global_map"]["map_array"] = np.stack([worldgen.make_grid(200, 3), worldgen.make_grid(200, 4)])
    sets = make_sets(P, lengths, cap, seed=11, box=box)
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, stack=True, episode_stats=True, wrappers=True,
                      map_policy="placement", ped_tracks=sets, tracks_policy="placement", info_track_sets=True)
    try:
        w = vec.world
        fields = ("sensor_maps", "vector_states", "lasers")
        stacks = {f: StackModel(k) for f, k in zip(fields, depths(2, 3, 2))}
        am = ActionModel(E * R, TABLE, table=TABLE8, clip=cfg["continuous_actions"])
        ep = EpisodeModel(E * R, cfg["control_hz"])
        state = vec.reset()
        snap = w.snapshot()
        for f in fields:
            stacks[f].reset(snap[f], np.ones(E * R, bool))
        ep.reset(np.ones(E * R, bool), np.zeros(E * R, np.int32))
        check_post(vec, "reset")
        seeds = [vec._spawn_seed + k for k in range(E)]
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
                seeds[k] = vec._device_seed0 + first + q
            resets += len(worlds)
            assert vec.world_maps().tolist() == [_cabi.map_for_placement(sd, 2) for sd in seeds], s
            assert info["track_sets"].tolist() == [_cabi.tracks_for_placement(sd, 3) for sd in seeds], s
        assert resets >= 2 * E
    finally:
        vec.close()


# ---- 6. refusals, and a bank nobody sees ----
def test_refusals_and_a_handle_without_a_bank_is_what_it_was():
    import ctypes as C
    import torch
    from img_env_amd import _cabi, config, spawn, worldgen
    from img_env_amd.vec_env import VecImageEnv, stack_params
    from img_env_amd.world import World
    E, R, P, _, _, lengths, cap, box, _ = SHAPES["5x2x3"]
    cfg = dataset_cfg(R, P, 4)
    sets = make_sets(P, lengths, cap, seed=11, box=box)
    n, cap, pose, traj, traj_v, length = _cabi.pack_track_sets(sets, P)
    lib = _cabi.load_library()
    add = lambda h, ln=length, tr=traj: lib.imgenv_tracks_add(h, n, cap, pose.ctypes.data, tr.ctypes.data, traj_v.ctypes.data, ln.ctypes.data)
    ids = lambda *v: (C.c_int32 * len(v))(*v)

    rvo = VecImageEnv(worldgen.make_yaml_cfg(R, P, cfg["global_map"]["map_array"], time_max=4, n_obstacles=N_OBS, seed=9), env_num=2, seed=9)
    try:  # not a dataset scene; not a bank-less handle's calls either
        assert add(rvo.world.h) == _cabi.EINVAL and b"DATASET" in lib.imgenv_last_error()
        assert lib.imgenv_tracks_policy(rvo.world.h, _cabi.TRACKS_CYCLE, 1) == _cabi.ESTATE
        assert lib.imgenv_world_tracks_set(rvo.world.h, 1, ids(0), ids(0), None) == _cabi.ESTATE
        assert (rvo.world_tracks() == -1).all()
        with pytest.raises(ValueError):
            VecImageEnv(worldgen.make_yaml_cfg(R, P, cfg["global_map"]["map_array"]), env_num=2, ped_tracks=sets)
    finally:
        rvo.close()

    params = stack_params(config.params_from_cfg(cfg), 1)
    shard = World(dict(params, robot_begin=0, robot_end=1), config.load_map(cfg))
    try:
        assert add(shard.h) == _cabi.EINVAL and b"shard" in lib.imgenv_last_error()
    finally:
        shard.close()

    plain = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True)  # a dataset handle WITHOUT a bank: as before
    bank = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=True, auto_reset=False, ped_tracks=sets)
    try:
        h = bank.world.h
        assert add(h) == _cabi.ESTATE and b"already" in lib.imgenv_last_error()                   # twice
        fresh = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9)
        try:
            for bad in (0, cap + 1):                                                                  # a bad length
                ln = length.copy()
                ln[1, 2] = bad
                assert add(fresh.world.h, ln=ln) == _cabi.EINVAL and b"length" in lib.imgenv_last_error()
            tr = traj.copy()
            tr[2, 0, 0, 1] = np.nan
            assert add(fresh.world.h, tr=tr) == _cabi.EINVAL and b"finite" in lib.imgenv_last_error()
            assert (fresh.world_tracks() == -1).all() and fresh.world.n_track_sets == 0            # ... and the handle is unchanged
            assert add(fresh.world.h) == 0
        finally:
            fresh.close()
        assert lib.imgenv_world_tracks_set(h, 1, ids(0), ids(3), None) == _cabi.EINVAL                # a bad set id
        assert lib.imgenv_world_tracks_set(h, 1, ids(0), ids(-1), None) == _cabi.EINVAL
        assert lib.imgenv_world_tracks_set(h, 1, ids(E), ids(0), None) == _cabi.EINVAL                # a bad world
        assert lib.imgenv_world_tracks_set(h, 2, ids(1, 1), ids(0, 1), None) == _cabi.EINVAL          # a world listed twice
        assert b"twice" in lib.imgenv_last_error()
        assert lib.imgenv_tracks_policy(h, _cabi.TRACKS_CYCLE, 0) == _cabi.EINVAL                     # repeat = 0
        assert lib.imgenv_tracks_policy(h, 3, 1) == _cabi.EINVAL
        with pytest.raises(ValueError):
            bank.set_world_tracks([0, 1], [0, 7])
        bank.reset()
        assert bank.world_tracks().tolist() == [0] * E                                                # nothing of the refused calls was applied
        assert add(h) == _cabi.ESTATE                                                                 # after the first reset

        # without a bank: the spawn reset still fails for want of ped_traj_v, the device-side reset still refuses the scene
        with pytest.raises(RuntimeError, match="ped_traj_v is missing"):
            plain.reset()
        plain.reset([with_tracks(spawn.native_spawn(cfg, 5 + k), (n, cap, pose, traj, traj_v, length), 0) for k in range(E)])
        with pytest.raises(RuntimeError, match="recorded crowds come with the reset call"):
            plain.step(torch.zeros(E * R, 3, device="cuda"))

        # the bank does not leak into a step: a banked handle's plain step launches what an unbanked one's launches
        a = torch.zeros(E * R, 3, device="cuda")
        bank.world.step(a)
        plain.world.step(a)
        assert bank.world.launches() == plain.world.launches() > 0
    finally:
        plain.close()
        bank.close()
