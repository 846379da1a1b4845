"""The episode log on the device (imgenv_episode_log_enable, csrc/episode_log.h: one record per finished episode in a ring, tagged
with what the episode ran on) against the numpy model of tests/episode_log_model.py, which tests/test_episode_log_model.py holds to
the reference's own log file.  The kernel records what the fold behind it counts, from the one figure function both share, so the
float columns are compared bit for bit; the order of the records is the chains' in stream order and the rows' in chain order.  The
tags are compared with what a synchronised twin handle answered (``world_scenarios()``, ``world_maps()``, ``world_tracks()``, the
placement number) while each episode ran."""
import copy
import ctypes as C

import numpy as np
import pytest

from episode_log_model import F64_NAMES, I32_NAMES, NONE64, EpisodeLogModel
from stack_model import bits
from test_gpu_episodes import (assert_every_kind_of_end, device_arrays, env_rows, episode_cfg, policy, print_totals, same_arrays,
                               step_inputs)

pytestmark = pytest.mark.gpu
INT_COLUMNS = tuple(k for k in I32_NAMES if k != "scenario_raw") + ("scenario",)


def same_records(got, want, where):
    """the dict of columns ``VecImageEnv.episode_log()`` returns against the model's: integers equal, floats bit for bit"""
    assert set(got) == set(want), (where, sorted(set(got) ^ set(want)))
    assert (got["oldest"], got["n_written"]) == (want["oldest"], want["n_written"]), (where, got["oldest"], got["n_written"], want["oldest"], want["n_written"])
    for k in want:
        if k in ("oldest", "n_written"):
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (where, k, g.dtype, w.dtype, g.shape, w.shape)
        same = bits(g) == bits(w)
        if not same.all():
            at = int(np.flatnonzero(~same)[0])
            raise AssertionError("%s: column %s differs at record %d (seq %d): got %r, want %r (%d of %d)" %
                                 (where, k, at, int(want["seq"][at]), g[at], w[at], (~same).sum(), same.size))


def same_ring(world, model, where):
    """the device's ring itself (``World.episode_log``, zero-copy views) against the model's, slot for slot"""
    import torch
    torch.cuda.synchronize()
    want = model.ring()
    got = {k: v.cpu().numpy() for k, v in world.episode_log.items()}
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape, (where, k, got[k].shape, want[k].shape)
        assert (bits(got[k]) == bits(want[k])).all(), (where, k)


def run_vec(mode, capacity, steps=36, E=64, R=2, P=3, each_step=None):
    """test_gpu_episodes' run of a VecImageEnv in one of its reset modes, with the log: the model is fed what each step handed out.
    ``each_step(vec, log, s)`` runs after every step.  Returns the model."""
    import torch
    from img_env_amd.vec_env import VecImageEnv
    cfg = episode_cfg(R, P)
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=mode != "host_reset", device_reset=mode == "device_reset",
                      episode_log=capacity)
    try:
        assert vec.episode_stats and vec.world.episode_log["i32"].shape == (10, capacity) and vec.world.episode_log["f64"].shape == (9, capacity)
        n = E * R
        log = EpisodeLogModel(n, cfg["control_hz"], capacity=capacity, robots_per_world=R)
        same_ring(vec.world, log, "enabled")
        state = vec.reset()
        log.reset(np.ones(n, bool), np.zeros(n, np.int32))  # the first reset opens every episode and logs nothing
        same_ring(vec.world, log, "first reset")
        assert log.n_written == 0
        rng = np.random.default_rng(4)
        for s in range(steps):
            a = policy(rng, state.vector_states.cpu().numpy())
            state, rew, done, info = vec.step(torch.as_tensor(a, device="cuda"))
            got = step_inputs(vec.world)
            place = np.full(n, NONE64, np.uint64)
            if mode == "device_reset":
                worlds, first = vec.world.autoreset_last()  # ascending; the q-th of them took placement first + q
                for q, k in enumerate(worlds):
                    place[k * R:(k + 1) * R] = first + q
                assert np.array_equal(env_rows(worlds, E, R), info["all_down"].cpu().numpy().astype(bool)), s
            else:
                worlds = list(info["reset_envs"])
            order = np.array([k * R + i for k in worlds for i in range(R)], np.int64)
            log.step(a, got["step_is_clean"], got["step_rewards"])
            log.reset(order, got["step_dones_info"], placements=place)
            where = "%s step %d" % (mode, s)
            same_arrays(device_arrays(vec.world), log.m.arrays(), where)
            same_ring(vec.world, log, where)
            same_records(vec.episode_log(since=0), log.columns(scenario=lambda r: -1), where)
            if each_step:
                each_step(vec, log, s)
        print_totals(mode, log.m)
        print("%s: %d records, %d counted" % (mode, log.n_written, sum(r["counted"] for r in log.records)))
        return log
    finally:
        vec.close()


# ---- 1. VecImageEnv in its three reset modes ----
@pytest.mark.parametrize("mode", ["host_reset", "native_spawn", "device_reset"])
def test_vec_env_log_equals_the_model_after_every_step(mode):
    """64 envs of 2 robots and 3 pedestrians, time limit 10, 36 steps of test_gpu_episodes' policy: after every step the records in
    [oldest, n_written), the ring itself and the statistics equal the model; arrivals, time-outs, collisions and short episodes all
    occur, and a record of each kind is in the log"""
    log = run_vec(mode, 4096)
    assert_every_kind_of_end(log.m)
    rec = log.columns()
    assert rec["n_written"] == len(rec["seq"]) == int(log.m.episodes.sum() + log.m.short_episodes.sum()) > 64
    assert rec["counted"].sum() == log.m.episodes.sum() and (rec["counted"] == 0).sum() == log.m.short_episodes.sum() > 0
    codes = set(rec["code"][rec["counted"] != 0].tolist())
    assert 5 in codes and 10 in codes and codes & {1, 2, 3}
    short = rec["counted"] == 0
    assert (rec["episode"][short] == 0).all() and (rec["steps"][short] <= 3).all() and all((rec[k][short] == 0).all() for k in F64_NAMES[1:])
    assert (rec["map"] == 0).all() and (rec["tracks"] == -1).all() and (rec["scenario"] == -1).all()
    if mode == "device_reset":  # the first episodes were placed by the host, the later ones carry the device's placement number
        assert (rec["placement"] == NONE64).sum() == 128 and len(set(rec["placement"].tolist())) > 64
    else:
        assert (rec["placement"] == NONE64).all()


# ---- 2. tags: scenario bank and map bank ----
def placement_number(world, k):
    """imgenv_world_placement's number alone (~0: the device has not placed world k)"""
    n = C.c_uint64(0xFFFFFFFFFFFFFFFF)
    world.lib.imgenv_world_placement(world.h, int(k), C.byref(n), *([None] * 9))
    return int(n.value)


def test_tags_are_what_a_synchronised_twin_saw_while_the_episode_ran():
    """8 envs, a bank of 5 recorded scenarios, two maps.  The first reset is the host's (reset_envs(scenario_ids=...)), then the device
    resets under QUEUE and, from half way, BY_PLACEMENT; two envs change map in mid-run.  A twin without a log is asked after every
    step which scenario, map and placement number every env runs; each record of the logged handle must carry what the twin
    answered for its env before the step that ended the episode."""
    import torch
    from img_env_amd import spawn, worldgen
    from img_env_amd.vec_env import VecImageEnv
    from test_gpu_map_bank import _grids
    E, R, P, n_obs, N, steps = 8, 2, 3, 2, 5, 28
    grids = _grids(2, 200, 3)
    cfg = worldgen.make_yaml_cfg(R, P, grids[0], time_max=4, n_obstacles=n_obs, seed=9, dt=0.25)
    bank = spawn.record_scenarios(cfg, N, 1000)
    cfg["global_map"]["map_array"] = np.stack(grids)
    mk = lambda **kw: VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, scenarios=bank, scenario_policy="queue",
                                  world_maps=[k % 2 for k in range(E)], **kw)
    run, twin = mk(episode_log=1024, episode_min_steps=1), mk()
    try:
        first_ids = [(3 * k + 1) % N for k in range(E)]
        for v in (run, twin):
            v.reset_envs(range(E), scenario_ids=first_ids)
            v.world.scenarios_policy("queue", first=2)

        def note():
            torch.cuda.synchronize()
            return dict(scenario=twin.world_scenarios().copy(), map=twin.world_maps().copy(),
                        placement=np.array([placement_number(twin.world, k) for k in range(E)], np.uint64))
        notes = [note()]
        assert notes[0]["scenario"].tolist() == first_ids and notes[0]["map"].tolist() == [k % 2 for k in range(E)]
        assert (notes[0]["placement"] == NONE64).all()
        assert run.episode_log()["n_written"] == 0  # the first reset logs nothing
        rng = np.random.default_rng(2)
        seen, n_rec = 0, 0
        for s in range(steps):
            if s == steps // 2:
                for v in (run, twin):
                    v.world.scenarios_policy("placement")
            if s in (5, 17):
                for v in (run, twin):
                    v.set_world_maps([1, 6], [0, 1] if s == 5 else [1, 0])
            a = np.zeros((E * R, 3), np.float32)
            a[:, 0], a[:, 1] = rng.uniform(0, 0.6, E * R), rng.uniform(-0.9, 0.9, E * R)
            for v in (run, twin):
                v.step(torch.as_tensor(a, device="cuda"))
            rec = run.episode_log()  # the records this step's reset chain appended
            before = notes[-1]
            assert rec["seq"].tolist() == list(range(n_rec, rec["n_written"])), s
            n_rec = rec["n_written"]
            for q in range(len(rec["seq"])):
                k = int(rec["world"][q])
                assert rec["robot"][q] // R == k
                got = (int(rec["scenario"][q]), int(rec["map"][q]), int(rec["placement"][q]))
                want = (int(before["scenario"][k]), int(before["map"][k]), int(before["placement"][k]))
                assert got == want, (s, q, k, got, want)
            notes.append(note())
            finished = sorted(set(rec["world"].tolist()))
            assert finished == twin.world.autoreset_last()[0], s
            seen += len(finished)
        everything = run.episode_log(since=0)
        assert everything["n_written"] == n_rec == seen * R and everything["oldest"] == 0
        assert len(set(everything["scenario"].tolist())) >= 4 and set(everything["map"].tolist()) == {0, 1}
        assert (everything["placement"] == NONE64).sum() == E * R and (everything["tracks"] == -1).all()
        # env 1 and env 6 ran episodes on both maps
        for k in (1, 6):
            assert set(everything["map"][everything["world"] == k].tolist()) == {0, 1}, k
        # both policies placed episodes: the queue's ids follow the placement number, the draws do not all
        dev = everything["placement"] != NONE64
        queue_like = (everything["scenario"][dev] == (2 + everything["placement"][dev].astype(np.int64)) % N)
        assert queue_like.any() and not queue_like.all()
    finally:
        run.close()
        twin.close()


# ---- 3. tags: track bank ----
def test_track_sets_and_the_dataset_wrappers_log_lines():
    """a dataset handle with a track bank under CYCLE, repeat 2: the ``tracks`` column is the ``world_tracks()`` history of a
    synchronised twin, and ``episode_log_lines(kind="ped_dataset")`` has one well-formed line per counted record"""
    import torch
    from img_env_amd.envs import episode_log_lines
    from img_env_amd.vec_env import VecImageEnv
    from test_gpu_track_bank import SHAPES, dataset_cfg, make_sets
    E, R, P, time_max, steps, lengths, cap, box, _ = SHAPES["5x2x3"]
    cfg = dataset_cfg(R, P, time_max)
    sets = make_sets(P, lengths, cap, seed=11, box=box)
    mk = lambda **kw: VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, ped_tracks=sets, tracks_policy="cycle",
                                  tracks_repeat=2, **kw)
    run, twin = mk(episode_log=256, episode_min_steps=2), mk()
    try:
        for v in (run, twin):
            v.reset()
        history = [twin.world_tracks().copy()]
        assert (history[0] == 0).all()
        rng = np.random.default_rng(2)
        for s in range(32):  # an episode takes at most time_max + 1 = 5 steps: every env closes six, the fifth and sixth on set 2
            a = np.zeros((E * R, 3), np.float32)
            a[:, 0], a[:, 1] = rng.uniform(0, 0.6, E * R), rng.uniform(-0.9, 0.9, E * R)
            for v in (run, twin):
                v.step(torch.as_tensor(a, device="cuda"))
            rec = run.episode_log()
            for q in range(len(rec["seq"])):
                assert rec["tracks"][q] == history[-1][rec["world"][q]], (s, q)
            history.append(twin.world_tracks().copy())
        rec = run.episode_log(since=0)
        assert rec["n_written"] >= 6 * E * R and set(rec["tracks"].tolist()) == {0, 1, 2}
        assert (rec["map"] == 0).all() and (rec["scenario"] == -1).all()
        lines = episode_log_lines(rec, cfg["control_hz"], "ped_dataset")
        counted = np.flatnonzero(rec["counted"] != 0)
        assert len(lines) == len(counted) > 0  # (short episodes have no line)
        for ln, q in zip(lines, counted):
            f = ln.split(", ")
            assert len(f) == 13, ln
            assert int(f[0]) == rec["tracks"][q] and int(f[12]) == rec["steps"][q] and int(f[10]) == rec["w_zero"][q]
            assert [int(f[1]), int(f[2]), int(f[3])] == [int(rec["code"][q] == c) for c in (5, 2, 10)]
            assert [float(x) for x in f[4:10]] == [rec[k][q] for k in ("v_avg", "w_avg", "v_acc", "w_acc", "v_jerk", "w_jerk")]
            assert float(f[11]) == round(int(rec["steps"][q]) * cfg["control_hz"], 4)
    finally:
        run.close()
        twin.close()


# ---- 4. the ring wraps ----
def test_a_ring_of_fifty_keeps_the_last_fifty():
    """case 1's device-reset run into a ring of 50 records: after every step the survivors are the model's last 50 (run_vec compares
    them), a read from 0 starts at ``oldest`` and reports both counters, reads clip at both ends"""
    seen = {}

    def each_step(vec, log, s):
        N, old = log.n_written, log.oldest
        rec, oldest, written = vec.world.read_episode_log(0)
        assert (oldest, written) == (old, N) and rec["seq"].tolist() == list(range(old, N)), s
        if N > 60 and "clipped" not in seen:
            seen["clipped"] = True
            part, _, _ = vec.world.read_episode_log(old + 3, 5)
            assert part["seq"].tolist() == list(range(old + 3, old + 8))
            assert part["robot"].tolist() == [log.records[q]["robot"] for q in range(old + 3, old + 8)]
            early, _, _ = vec.world.read_episode_log(old - 2, 5)  # two of the five are gone
            assert early["seq"].tolist() == list(range(old, old + 3))
            late, _, _ = vec.world.read_episode_log(N - 2, 50)
            assert late["seq"].tolist() == [N - 2, N - 1]
            assert len(vec.world.read_episode_log(N)[0]) == 0 and len(vec.world.read_episode_log(N + 7, 3)[0]) == 0
            assert len(vec.world.read_episode_log(0, 0)[0]) == 0
    log = run_vec("device_reset", 50, each_step=each_step)
    assert log.n_written > 300 and log.oldest == log.n_written - 50 and seen.get("clipped")


# ---- 5. more than one chunk of 1024 rows ----
def test_one_chain_of_1280_rows_logs_them_in_ascending_order():
    """640 envs of 2 robots, min_steps 2, no auto-reset: 5 steps, then ``reset()`` of every env -- one chain whose 1280 rows take two
    chunks of the kernel's walk; 1280 records, rows ascending, equal to the model's.  The first reset of the run logs nothing."""
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P = 640, 2, 3
    n = E * R
    cfg = episode_cfg(R, P, time_max=30)
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=5, native_spawn=True, auto_reset=False, episode_log=2048, episode_min_steps=2)
    try:
        log = EpisodeLogModel(n, cfg["control_hz"], min_steps=2, capacity=2048, robots_per_world=R)
        state = vec.reset()
        log.reset(np.ones(n, bool), np.zeros(n, np.int32))
        assert vec.episode_log()["n_written"] == 0
        rng = np.random.default_rng(1)
        for s in range(5):
            a = policy(rng, state.vector_states.cpu().numpy())
            state, _, _, info = vec.step(torch.as_tensor(a, device="cuda"))
            last = step_inputs(vec.world)
            log.step(a, last["step_is_clean"], last["step_rewards"])
        assert vec.episode_log()["n_written"] == 0  # steps append nothing
        vec.reset()
        log.reset(np.ones(n, bool), last["step_dones_info"])
        rec = vec.episode_log()
        same_records(rec, log.columns(scenario=lambda r: -1), "reset of every env")
        assert rec["n_written"] == n == 1280 and rec["robot"].tolist() == list(range(n)) and rec["world"].tolist() == [r // R for r in range(n)]
        assert (rec["counted"] == 1).all() and (rec["steps"] == 5).all() and (rec["episode"] == 1).all()
        assert len(set(rec["code"].tolist())) > 1 and np.abs(rec["v_avg"]).sum() > 0
        same_ring(vec.world, log, "reset of every env")
        same_arrays(device_arrays(vec.world), log.m.arrays(), "reset of every env")
    finally:
        vec.close()


# ---- 6. a handle with statistics only ----
@pytest.mark.parametrize("device_reset", [False, True], ids=["native_spawn", "device_reset"])
def test_the_log_disturbs_nothing_and_costs_one_launch_per_reset_chain(device_reset):
    """same cfg, seed and actions on a handle that keeps statistics only and on one with the log: every output byte and every
    statistics array equal on every step; ``imgenv_step_launches`` differs by exactly one per reset chain.  After
    imgenv_step_autoreset_device the count covers the step's chain and the reset chain behind it: always 1 more.  After
    imgenv_step_autoreset it covers the last chain alone: 1 more where a world was reset, 0 where the call only stepped, and both
    kinds of call must occur."""
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P = 16, 2, 3
    cfg = episode_cfg(R, P)
    stats = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=True, device_reset=device_reset, episode_stats=True)
    logged = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=True, device_reset=device_reset, episode_log=512)
    try:
        assert stats.world.episode_log is None
        with pytest.raises(RuntimeError):
            stats.episode_log()
        with pytest.raises(RuntimeError):
            stats.world.read_episode_log()
        for v in (stats, logged):
            v.reset()
        assert logged.world.launches() == stats.world.launches() + 1
        rng = np.random.default_rng(2)
        extra = set()
        for s in range(24):
            a = torch.as_tensor(policy(rng, stats.world.out["vector_states"].cpu().numpy()), device="cuda")
            infos = [v.step(a)[3] for v in (stats, logged)]
            sa, sb = stats.world.snapshot(), logged.world.snapshot()
            assert set(sa) == set(sb)
            for f in sa:
                assert sa[f].tobytes() == sb[f].tobytes(), (s, f)
            same_arrays(device_arrays(logged.world), device_arrays(stats.world), "step %d" % s)
            diff = logged.world.launches() - stats.world.launches()
            if device_reset:
                assert diff == 1, (s, diff)
            else:
                assert infos[0]["reset_envs"] == infos[1]["reset_envs"], s
                assert diff == (1 if infos[0]["reset_envs"] else 0), (s, diff, infos[0]["reset_envs"])
            extra.add(diff)
        assert extra == ({1} if device_reset else {0, 1}), extra
        assert logged.episode_log()["n_written"] == int(device_arrays(stats.world)["episodes"].sum() + device_arrays(stats.world)["short_episodes"].sum()) > 0
    finally:
        stats.close()
        logged.close()


# ---- 7. stream order ----
def test_the_log_is_ordered_on_the_stream_without_any_synchronisation():
    """40 device-reset steps with device-resident actions queued behind a stream kept busy by large matrix products, no
    synchronisation until the end; the model is fed from a twin run of the same cfg, seed and actions that is synchronised after
    every step"""
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, steps = 64, 2, 3, 40
    n = E * R
    cfg = episode_cfg(R, P, time_max=5)
    run = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, episode_log=4096)
    twin = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True)
    try:
        g = torch.Generator(device="cuda").manual_seed(1)
        acts = torch.zeros(steps, n, 3, device="cuda")
        acts[:, :, 0] = torch.rand(steps, n, generator=g, device="cuda") * 0.6
        acts[:, :, 1] = torch.rand(steps, n, generator=g, device="cuda") * 1.8 - 0.9
        acts[::3, ::2, 1] = 0.0
        log = EpisodeLogModel(n, cfg["control_hz"], capacity=4096, robots_per_world=R)
        twin.reset()
        log.reset(np.ones(n, bool), np.zeros(n, np.int32))
        host_acts = acts.cpu().numpy()
        for s in range(steps):
            _, _, _, info = twin.step(acts[s])
            got = step_inputs(twin.world)
            worlds, first = twin.world.autoreset_last()
            place = np.full(n, NONE64, np.uint64)
            for q, k in enumerate(worlds):
                place[k * R:(k + 1) * R] = first + q
            log.step(host_acts[s], got["step_is_clean"], got["step_rewards"])
            log.reset(env_rows(worlds, E, R), got["step_dones_info"], placements=place)
        torch.cuda.synchronize()
        busy = torch.randn(4096, 4096, device="cuda")
        for q in range(20):
            busy = (busy @ busy).clamp_(-1, 1)
        run.reset()
        for s in range(steps):
            run.step(acts[s])
        assert "synchronis" in VecImageEnv.episode_log.__doc__.lower()
        same_records(run.episode_log(), log.columns(scenario=lambda r: -1), "after %d unsynchronised steps" % steps)
        same_ring(run.world, log, "after %d unsynchronised steps" % steps)
        assert log.n_written >= 4 * n and log.m.ends[1].sum() > 0
    finally:
        run.close()
        twin.close()


# ---- 8. robot shards ----
def test_shards_log_their_local_rows():
    """two handles owning halves of one 24-robot world against the whole-world handle and the model, through resets in the middle:
    each shard logs its local rows (robot 0 .. 11, world 0), and the union of the shards' records is the whole handle's log"""
    import torch
    from img_env_amd.world import World
    from scenarios import random_actions, small_world
    n, n_peds = 24, 10
    grid, params, layout = small_world(n, n_peds, seed=31, grid_size=320, clearance=0.8)
    _, _, layout2 = small_world(n, n_peds, seed=32, grid_size=320, clearance=0.8)
    bounds = [0, n // 2, n]
    full = World(params, grid)
    ranks = [World(dict(params, robot_begin=bounds[r], robot_end=bounds[r + 1]), grid) for r in range(2)]
    try:
        for w in [full] + ranks:
            w.enable_episodes(min_steps=3, dt=0.25)
            w.enable_episode_log(80)  # (holds all 72 records of the whole handle; a ring that wraps is test 4's)
        log = EpisodeLogModel(n, 0.25, capacity=80)

        def exchange():
            torch.cuda.synchronize()
            for r, w in enumerate(ranks):
                for q, o in enumerate(ranks):
                    if q != r:
                        w.records[bounds[q]:bounds[q + 1]].copy_(o.records[bounds[q]:bounds[q + 1]])
        codes = np.zeros(n, np.int32)
        rng = np.random.default_rng(5)
        chains = 0
        for lay, k in ((layout, 5), (layout2, 2), (layout, 6), (layout2, 0)):
            for w in [full] + ranks:
                w.reset(lay)
            log.reset(np.ones(n, bool), codes)
            chains += 1
            for s in range(k):
                a = random_actions(rng, n)
                full.step(a)
                for r, w in enumerate(ranks):
                    w.step_begin(a[bounds[r]:bounds[r + 1]])
                exchange()
                for w in ranks:
                    w.step_end()
                got = step_inputs(full)
                log.step(a, got["step_is_clean"], got["step_rewards"])
                codes = got["step_dones_info"]
        whole, oldest, written = full.read_episode_log(0)
        want = log.columns(scenario=lambda r: -1)
        assert (oldest, written) == (want["oldest"], want["n_written"]) == (0, 3 * n)
        for k in INT_COLUMNS + F64_NAMES + ("placement", "seq"):
            assert (bits(np.ascontiguousarray(whole[k] if k not in F64_NAMES[1:] else whole["figures"][:, F64_NAMES.index(k) - 1])) ==
                    bits(want[k])).all(), k
        assert (whole["world"] == 0).all() and set(whole["counted"].tolist()) == {0, 1}
        # the shards: 3 chains of 12 records each -- every chain, record by record and on every column, with the whole handle's rows
        # of that shard
        for r, w in enumerate(ranks):
            part, p_old, p_written = w.read_episode_log(0)
            assert (p_old, p_written) == (0, 3 * (n // 2)) and (part["world"] == 0).all()
            for c in range(3):
                mine = part[c * (n // 2):(c + 1) * (n // 2)]
                theirs = whole[(whole["seq"] >= c * n + bounds[r]) & (whole["seq"] < c * n + bounds[r + 1])]
                assert len(mine) == len(theirs) == n // 2
                assert mine["robot"].tolist() == list(range(n // 2)) and theirs["robot"].tolist() == list(range(bounds[r], bounds[r + 1]))
                for k in ("code", "steps", "len", "counted", "episode", "map", "tracks", "scenario", "placement"):
                    assert np.array_equal(mine[k], theirs[k]), (r, c, k)
                assert (bits(mine["ep_return"]) == bits(theirs["ep_return"])).all() and (bits(mine["figures"]) == bits(theirs["figures"])).all()
            # ... and every chain against the model, which holds all of them
            for c in range(3):
                mine = part[c * (n // 2):(c + 1) * (n // 2)]
                recs = [log.records[c * n + bounds[r] + j] for j in range(n // 2)]
                assert mine["steps"].tolist() == [x["steps"] for x in recs] and mine["code"].tolist() == [x["code"] for x in recs]
                assert (bits(mine["ep_return"]) == bits(np.array([x["ep_return"] for x in recs]))).all()
                assert (bits(mine["figures"][:, 6]) == bits(np.array([x["v_avg"] for x in recs]))).all()
        assert chains == 4
    finally:
        full.close()
        for w in ranks:
            w.close()


# ---- 9. refusals ----
def test_enable_and_read_refuse_what_the_header_says_they_refuse():
    from img_env_amd import _cabi
    from img_env_amd.world import World
    from scenarios import small_world
    grid, params, layout = small_world(4, 2, seed=4)
    w = World(params, grid)
    try:
        o = _cabi.EpisodeLogOut()
        good = _cabi.make_episode_log_cfg(16)
        assert w.lib.imgenv_episode_log_enable(w.h, C.byref(good), C.byref(o)) == _cabi.ESTATE  # before imgenv_episodes_enable
        with pytest.raises(RuntimeError):
            w.enable_episode_log(16)
        assert w.lib.imgenv_episode_log_outputs(w.h, C.byref(o)) == _cabi.ESTATE
        assert w.lib.imgenv_episode_log_read(w.h, 0, 0, None, None, None, None) == _cabi.ESTATE
        w.enable_episodes(3, 0.25)
        assert w.lib.imgenv_episode_log_outputs(w.h, C.byref(o)) == _cabi.ESTATE
        for cap in (0, -3, _cabi.EPLOG_MAX_CAPACITY + 1):
            with pytest.raises(ValueError, match="capacity"):
                w.enable_episode_log(cap)
        c = _cabi.make_episode_log_cfg(16)
        c.struct_size += 8
        assert w.lib.imgenv_episode_log_enable(w.h, C.byref(c), None) == _cabi.EINVAL
        assert w.episode_log is None
        launches = w.launches()
        first = w.enable_episode_log(16)
        assert w.enable_episode_log(16) is first and w.launches() == launches  # the same capacity again: nothing changes
        with pytest.raises(ValueError, match="already"):
            w.enable_episode_log(17)
        assert w.lib.imgenv_episode_log_enable(w.h, C.byref(good), C.byref(o)) == 0
        assert o.capacity == 16 and o.struct_size == C.sizeof(_cabi.EpisodeLogOut)
        o2 = _cabi.EpisodeLogOut()
        assert w.lib.imgenv_episode_log_outputs(w.h, C.byref(o2)) == 0
        for name, t in first.items():
            assert getattr(o, name) == getattr(o2, name) == t.data_ptr(), name
        assert w.lib.imgenv_episode_log_read(w.h, 0, 4, None, None, None, None) == _cabi.EINVAL  # records wanted, nowhere to put them
        assert w.lib.imgenv_episode_log_read(w.h, 0, -1, None, None, None, None) == _cabi.EINVAL
        rec, oldest, written = w.read_episode_log()
        assert len(rec) == 0 and (oldest, written) == (0, 0)
        w.reset(layout)  # the first reset: nothing was open
        assert w.read_episode_log()[2] == 0
        w.reset(layout)  # episodes of zero steps: logged, not counted; opened behind the log, without banks
        rec, oldest, written = w.read_episode_log()
        assert (oldest, written) == (0, 4) and rec["robot"].tolist() == [0, 1, 2, 3] and (rec["counted"] == 0).all() and (rec["steps"] == 0).all()
        assert (rec["map"] == 0).all() and (rec["tracks"] == -1).all() and (rec["scenario"] == -1).all() and (rec["placement"] == NONE64).all()
    finally:
        w.close()


def test_episodes_open_before_the_log_carry_no_tags():
    """statistics enabled, a reset, two steps, THEN the log: the episodes that were open carry map -1, tracks -1, scenario -1 (no
    bank: -1 either way) and placement ~0; the next ones the handle's tags"""
    from img_env_amd.world import World
    from scenarios import random_actions, small_world
    n = 6
    grid, params, layout = small_world(n, 2, seed=4)
    w = World(params, grid)
    try:
        w.enable_episodes(0, 0.25)
        w.reset(layout)
        rng = np.random.default_rng(0)
        for s in range(2):
            w.step(random_actions(rng, n))
        w.enable_episode_log(64)
        w.reset(layout)
        w.step(random_actions(rng, n))
        w.reset(layout)
        rec, _, written = w.read_episode_log()
        assert written == 2 * n and rec["steps"].tolist() == [2] * n + [1] * n and (rec["counted"] == 1).all()
        assert rec["map"].tolist() == [-1] * n + [0] * n and (rec["tracks"] == -1).all() and (rec["placement"] == NONE64).all()
        assert rec["episode"].tolist() == [1] * n + [2] * n
        w.clear_episodes()  # the log stays, `episode` follows the cleared counter
        w.step(random_actions(rng, n))
        w.reset(layout)
        rec, _, written = w.read_episode_log(2 * n)
        assert written == 3 * n and rec["episode"].tolist() == [1] * n
    finally:
        w.close()
