"""The episode statistics on the device (imgenv_episodes_enable, csrc/episodes.h: TestEpisodeWrapper per robot of a handle) against
the numpy model of tests/episode_model.py, which tests/test_episode_model.py holds to the reference's own recording.  The kernel
only adds, subtracts, multiplies, divides, takes |x| and rint in float64 without contraction, so every per-robot array is compared
bit for bit, after every step.  The model is fed what the step itself handed out: the actions, ``step_is_clean``,
``step_dones_info``, ``step_rewards`` and which envs restarted."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest

from episode_model import ENDS, EpisodeModel
from scenarios import random_actions, small_world
from stack_model import StackModel, bits, depths

pytestmark = pytest.mark.gpu
STEP_FIELDS = ("step_is_clean", "step_dones_info", "step_rewards")


def episode_cfg(R, P, time_max=10, **over):
    """envs whose episodes end in every way within a few dozen steps: starts and goals of robots and pedestrians drawn in one
    4.5 m box of the map (a few wall cells in it), goals from 0.4 m away (an arrival is 0.3 m), starts 0.7 m apart"""
    from img_env_amd import worldgen
    grid = worldgen.make_grid(200, 3)
    cfg = worldgen.make_yaml_cfg(R, P, grid, time_max=time_max, n_obstacles=2, seed=9, **over)
    box = [2.5, 7.0, 2.5, 7.0]
    cfg["robot"].update(begin_poses=[box] * R, target_poses_type=["range"] * R, target_poses=[box] * R)
    cfg["ped_sim"].update(begin_poses=[box] * P, target_poses_type=["range"] * P, target_poses=[box] * P)
    cfg["object"].update(poses=[box] * 2)
    cfg["target_min_dist"] = 0.4
    cfg["spawn_clearance"] = 0.7
    return cfg


def policy(rng, vector_states):
    """turn towards the goal and drive (vector_states[:, :2] is the goal in the robot's frame), w exactly 0 when it is dead ahead;
    a quarter of the commands are random"""
    vs = np.asarray(vector_states, np.float64)
    n = len(vs)
    ang = np.arctan2(vs[:, 1], vs[:, 0])
    a = np.zeros((n, 3), np.float32)
    a[:, 0] = np.where(np.abs(ang) < 0.7, 0.6, 0.1)
    a[:, 1] = np.clip(2.0 * ang, -0.9, 0.9)
    a[np.abs(ang) < 0.05, 1] = 0.0
    wild = rng.uniform(size=n) < 0.25
    a[wild, 0] = rng.uniform(0, 0.6, wild.sum())
    a[wild, 1] = rng.uniform(-0.9, 0.9, wild.sum())
    return a


def env_rows(envs, E, R):
    rows = np.zeros(E * R, bool)
    for k in envs:
        rows[k * R:(k + 1) * R] = True
    return rows


def same_arrays(got, want, where):
    """every array of imgenv_episodes_out, bit for bit"""
    assert set(got) == set(want), where
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (where, k, g.dtype, w.dtype, g.shape, w.shape)
        same = bits(g) == bits(w)
        if not same.all():
            at = np.argwhere(~same)[0]
            raise AssertionError("%s: %s differs at %s: got %r, want %r (%d of %d)" %
                                 (where, k, at.tolist(), g[tuple(at)], w[tuple(at)], (~same).sum(), same.size))


def device_arrays(world):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in world.episodes.items()}


def step_inputs(world):
    """host copies of what the last step handed out (after synchronising)"""
    import torch
    torch.cuda.synchronize()
    return {f: world.out[f].cpu().numpy().copy() for f in STEP_FIELDS}


def print_totals(where, m):
    print("%s: %s short %d episodes %d" % (where, dict(zip(ENDS, m.ends.sum(axis=1).tolist())), m.short_episodes.sum(), m.episodes.sum()))


def assert_every_kind_of_end(m):
    """the run only counts as a test if the model itself saw every branch of the fold"""
    ends = dict(zip(ENDS, m.ends.sum(axis=1).tolist()))
    assert m.episodes.sum() > 0 and m.short_episodes.sum() > 0, (int(m.episodes.sum()), int(m.short_episodes.sum()))
    assert ends["timeout"] > 0 and ends["arrive"] > 0, ends
    assert ends["static_collision"] + ends["ped_collision"] + ends["other_collision"] > 0, ends


# ---- 1. VecImageEnv in its three reset modes ----
@pytest.mark.parametrize("mode", ["host_reset", "native_spawn", "device_reset"])
def test_vec_env_statistics_equal_the_model_after_every_step(mode):
    """64 envs of 2 robots and 3 pedestrians, time limit 10, a goal-seeking policy with random commands mixed in: arrivals, all three
    collision classes, time-outs and episodes of three steps or fewer all occur (asserted on the model's own totals).  Host reset
    = imgenv_step + imgenv_reset_worlds, native_spawn = imgenv_step_autoreset, device_reset = imgenv_step_autoreset_device."""
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, steps = 64, 2, 3, 36
    cfg = episode_cfg(R, P)
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=mode != "host_reset", device_reset=mode == "device_reset",
                      episode_stats=True)
    try:
        assert vec.episode_tensors() is vec.world.episodes and vec.world.episodes["ends"].shape == (6, E * R)
        m = EpisodeModel(E * R, cfg["control_hz"])
        same_arrays(device_arrays(vec.world), m.arrays(), "enabled")
        state = vec.reset()
        m.reset(np.ones(E * R, bool), np.zeros(E * R, np.int32))
        same_arrays(device_arrays(vec.world), m.arrays(), "first reset")
        rng = np.random.default_rng(4)
        for s in range(steps):
            a = policy(rng, state.vector_states.cpu().numpy())
            state, rew, done, info = vec.step(torch.as_tensor(a, device="cuda"))
            got = step_inputs(vec.world)
            all_down = info["all_down"].cpu().numpy().astype(bool)
            if mode == "device_reset":
                assert info["reset_envs"] is None
                rows = all_down
            else:
                rows = env_rows(info["reset_envs"], E, R)
                assert np.array_equal(rows, all_down), s
            m.step(a, got["step_is_clean"], got["step_rewards"])
            m.reset(rows, got["step_dones_info"])
            same_arrays(device_arrays(vec.world), m.arrays(), "%s step %d" % (mode, s))
        print_totals(mode, m)
        assert_every_kind_of_end(m)
        assert m.ends[5].sum() == 0  # nobody reset an unfinished env
        want, got = m.statistics(), vec.episode_statistics()
        assert set(got) == set(want) and "synchronis" in VecImageEnv.episode_statistics.__doc__.lower()
        for k, v in want.items():
            assert got[k] == pytest.approx(v, rel=1e-12, abs=1e-12), k
        assert got["episodes"] == int(m.episodes.sum()) > E and 0 < got["arrive_rate"] < 1 and got["avg_len"] > 0
    finally:
        vec.close()


# ---- 2. manual resets, imgenv_reset, clear ----
def test_a_callers_reset_of_an_unfinished_env_is_aborted_and_clear_starts_over():
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P = 12, 2, 3
    cfg = episode_cfg(R, P, time_max=30)
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=5, native_spawn=True, episode_stats=True, episode_min_steps=2)
    try:
        m = EpisodeModel(E * R, cfg["control_hz"], min_steps=2)
        state = vec.reset()
        m.reset(np.ones(E * R, bool), np.zeros(E * R, np.int32))
        rng = np.random.default_rng(1)
        last = None

        def run(n, tag):
            nonlocal state, last
            for s in range(n):
                a = policy(rng, state.vector_states.cpu().numpy())
                state, _, _, info = vec.step(torch.as_tensor(a, device="cuda"))
                last = step_inputs(vec.world)
                m.step(a, last["step_is_clean"], last["step_rewards"])
                m.reset(env_rows(info["reset_envs"], E, R), last["step_dones_info"])
                same_arrays(device_arrays(vec.world), m.arrays(), "%s %d" % (tag, s))
        run(4, "a")
        unfinished = [k for k in range(E) if (last["step_dones_info"][k * R:(k + 1) * R] == 0).all() and m.open_steps[k * R] == 4][:3]
        assert len(unfinished) == 3
        state = vec.reset_envs(unfinished)  # imgenv_reset_worlds_spawn in mid-episode
        m.reset(env_rows(unfinished, E, R), last["step_dones_info"])
        same_arrays(device_arrays(vec.world), m.arrays(), "manual reset")
        assert m.ends[5].sum() == 3 * R and (m.last_code[env_rows(unfinished, E, R)] == 0).all()
        run(3, "b")
        vec.clear_episode_statistics()
        m.clear()
        same_arrays(device_arrays(vec.world), m.arrays(), "clear")
        assert m.open.all() and m.episodes.sum() == 0
        run(6, "c")
        state = vec.reset()  # every env, whatever it was doing
        m.reset(np.ones(E * R, bool), last["step_dones_info"])
        same_arrays(device_arrays(vec.world), m.arrays(), "reset of every env")
        assert m.ends[5].sum() > 0 and m.episodes.sum() > 0
        assert vec.episode_statistics()["aborted_rate"] == pytest.approx(m.statistics()["aborted_rate"], rel=1e-12)
    finally:
        vec.close()


def test_imgenv_reset_folds_every_robot_of_a_single_world():
    """a plain World (one world, imgenv_reset / imgenv_step): enabled after the first reset, so the steps up to the next reset are
    ignored; then every imgenv_reset folds all robots"""
    from img_env_amd.world import World
    n = 10
    grid, params, layout = small_world(n, 4, seed=4)
    _, _, layout2 = small_world(n, 4, seed=6)
    w = World(params, grid)
    try:
        w.reset(layout)
        w.enable_episodes(min_steps=1, dt=0.25)
        m = EpisodeModel(n, 0.25, min_steps=1)
        rng = np.random.default_rng(0)
        codes = np.zeros(n, np.int32)
        for rnd, lay in enumerate((layout2, layout, layout2)):
            for s in range(3 + rnd):
                a = random_actions(rng, n)
                w.step(a)
                got = step_inputs(w)
                m.step(a, got["step_is_clean"], got["step_rewards"])
                codes = got["step_dones_info"]
                same_arrays(device_arrays(w), m.arrays(), "round %d step %d" % (rnd, s))
            w.reset(lay)
            m.reset(np.ones(n, bool), codes)
            same_arrays(device_arrays(w), m.arrays(), "reset %d" % rnd)
        assert (m.episodes == 2).all() and m.open.all() and m.speed_steps.sum() == n * (4 + 5)
    finally:
        w.close()


def test_enable_refuses_what_the_header_says_it_refuses():
    from img_env_amd import _cabi
    from img_env_amd.world import World
    grid, params, layout = small_world(4, 2, seed=4)
    w = World(params, grid)
    try:
        o = _cabi.EpisodesOut()
        assert w.lib.imgenv_episodes_outputs(w.h, C.byref(o)) == _cabi.ESTATE
        assert w.lib.imgenv_episodes_clear(w.h, None) == _cabi.ESTATE
        for bad in ((3, 0.0), (3, -1.0), (-1, 0.25)):
            with pytest.raises(ValueError):
                w.enable_episodes(*bad)
        c = _cabi.make_episodes_cfg(3, 0.25)
        c.struct_size += 8
        assert w.lib.imgenv_episodes_enable(w.h, C.byref(c), None) == _cabi.EINVAL
        assert w.episodes is None
        first = w.enable_episodes(3, 0.25)
        assert w.enable_episodes(3, 0.25) is first  # the same cfg again: nothing changes
        for other in ((4, 0.25), (3, 0.5)):
            with pytest.raises(ValueError, match="already"):
                w.enable_episodes(*other)
        assert w.lib.imgenv_episodes_outputs(w.h, C.byref(o)) == 0 and o.n_local == 4
        for name, t in first.items():
            assert getattr(o, name) == t.data_ptr(), name
    finally:
        w.close()


# ---- 3. together with the observation stacks ----
def test_statistics_and_stacks_on_one_handle():
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, steps = 16, 2, 3, 24
    cfg = episode_cfg(R, P, image_batch=2, state_batch=3, laser_batch=2)
    kd = depths(2, 3, 2)
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, stack=True, episode_stats=True)
    try:
        fields = ("sensor_maps", "vector_states", "lasers")
        stacks = {f: StackModel(k) for f, k in zip(fields, kd)}
        m = EpisodeModel(E * R, cfg["control_hz"])
        vec.reset()
        snap = vec.world.snapshot()
        for f in fields:
            stacks[f].reset(snap[f], np.ones(E * R, bool))
        m.reset(np.ones(E * R, bool), np.zeros(E * R, np.int32))
        rng = np.random.default_rng(3)
        for s in range(steps):
            a = policy(rng, snap["vector_states"])
            _, _, _, info = vec.step(torch.as_tensor(a, device="cuda"))
            snap = vec.world.snapshot()
            rows = info["all_down"].cpu().numpy().astype(bool)
            m.step(a, snap["step_is_clean"], snap["step_rewards"])
            m.reset(rows, snap["step_dones_info"])
            same_arrays(device_arrays(vec.world), m.arrays(), "step %d" % s)
            for f in fields:
                want = stacks[f].update(snap[f], rows)
                got = vec.world.stack[f].cpu().numpy()
                assert (bits(got) == bits(want.reshape(got.shape))).all(), (s, f)
        assert m.episodes.sum() > E
    finally:
        vec.close()


# ---- 4. a handle that never enables ----
@pytest.mark.parametrize("device_reset", [False, True], ids=["native_spawn", "device_reset"])
def test_the_statistics_disturb_nothing_and_cost_one_launch_per_chain(device_reset):
    """same cfg, seed and actions on a handle that never touches the new calls and on one that keeps statistics: every output byte
    equal on every step, and ``imgenv_step_launches`` differs by exactly the k_episodes launches, one per chain.  After
    imgenv_step_autoreset_device that count covers the step's chain and the reset chain behind it: 2 more.  After
    imgenv_step_autoreset it covers the last chain alone -- the step's, or the reset chain's where a world was reset, since
    imgenv_reset_worlds starts the count over as it always has: 1 more in calls of either kind, and both kinds must occur."""
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P = 16, 2, 3
    cfg = episode_cfg(R, P)
    plain = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=True, device_reset=device_reset)
    stats = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=True, device_reset=device_reset, episode_stats=True)
    try:
        assert plain.world.episodes is None
        with pytest.raises(RuntimeError):
            plain.episode_tensors()
        for v in (plain, stats):
            v.reset()
        assert stats.world.launches() == plain.world.launches() + 1
        rng = np.random.default_rng(2)
        extra, with_reset = set(), set()
        for s in range(24):
            a = torch.as_tensor(policy(rng, plain.world.out["vector_states"].cpu().numpy()), device="cuda")
            infos = [v.step(a)[3] for v in (plain, stats)]
            if not device_reset:
                assert infos[0]["reset_envs"] == infos[1]["reset_envs"], s
                with_reset.add(len(infos[0]["reset_envs"]) > 0)
            sa, sb = plain.world.snapshot(), stats.world.snapshot()
            assert set(sa) == set(sb)
            for f in sa:
                assert sa[f].tobytes() == sb[f].tobytes(), (s, f)
            extra.add(stats.world.launches() - plain.world.launches())
        assert extra == ({2} if device_reset else {1}), extra
        assert device_reset or with_reset == {False, True}, with_reset
    finally:
        plain.close()
        stats.close()


# ---- 5. robot shards ----
def test_shards_keep_the_statistics_of_their_local_rows():
    """two handles owning halves of one 24-robot world (step_begin, the exchange by hand, step_end) against the whole-world handle
    and the model, through resets in the middle"""
    import torch
    from img_env_amd.world import World
    n, n_peds, steps = 24, 10, 12
    grid, params, layout = small_world(n, n_peds, seed=31, grid_size=320, clearance=0.8)
    _, _, layout2 = small_world(n, n_peds, seed=32, grid_size=320, clearance=0.8)
    bounds = [0, n // 2, n]
    full = World(params, grid)
    ranks = [World(dict(params, robot_begin=bounds[r], robot_end=bounds[r + 1]), grid) for r in range(2)]
    try:
        for w in [full] + ranks:
            w.enable_episodes(min_steps=3, dt=0.25)
        assert ranks[1].episodes["ends"].shape == (6, n // 2)
        m = EpisodeModel(n, 0.25)

        def exchange():
            torch.cuda.synchronize()
            for r, w in enumerate(ranks):
                for q, o in enumerate(ranks):
                    if q != r:
                        w.records[bounds[q]:bounds[q + 1]].copy_(o.records[bounds[q]:bounds[q + 1]])

        def same(where):
            whole = device_arrays(full)
            parts = [device_arrays(w) for w in ranks]
            same_arrays(whole, m.arrays(), where)
            same_arrays({k: np.concatenate([p[k] for p in parts], axis=-1) for k in whole}, whole, "%s (shards)" % where)
        codes = np.zeros(n, np.int32)
        rng = np.random.default_rng(5)
        for lay, k in ((layout, 5), (layout2, 2), (layout, 6)):
            for w in [full] + ranks:
                w.reset(lay)
            m.reset(np.ones(n, bool), codes)
            same("reset")
            for s in range(k):
                a = random_actions(rng, n)
                full.step(a)
                for r, w in enumerate(ranks):
                    w.step_begin(a[bounds[r]:bounds[r + 1]])
                exchange()
                for w in ranks:
                    w.step_end()
                got = step_inputs(full)
                m.step(a, got["step_is_clean"], got["step_rewards"])
                codes = got["step_dones_info"]
                same(s)
        assert (m.episodes == 1).all() and (m.short_episodes == 1).all() and m.ends[5].sum() > 0
    finally:
        full.close()
        for w in ranks:
            w.close()


# ---- 6. stream order ----
def test_statistics_are_ordered_on_the_stream_without_any_synchronisation():
    """40 device-reset steps with device-resident actions queued behind a stream kept busy by large matrix products, no
    synchronisation until the end; the model is fed from a twin run of the same cfg, seed and actions that is synchronised after
    every step"""
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, steps = 64, 2, 3, 40
    cfg = episode_cfg(R, P, time_max=5)
    run = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, episode_stats=True)
    twin = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True)
    try:
        g = torch.Generator(device="cuda").manual_seed(1)
        acts = torch.zeros(steps, E * R, 3, device="cuda")
        acts[:, :, 0] = torch.rand(steps, E * R, generator=g, device="cuda") * 0.6
        acts[:, :, 1] = torch.rand(steps, E * R, generator=g, device="cuda") * 1.8 - 0.9
        acts[::3, ::2, 1] = 0.0
        m = EpisodeModel(E * R, cfg["control_hz"])
        twin.reset()
        m.reset(np.ones(E * R, bool), np.zeros(E * R, np.int32))
        host_acts = acts.cpu().numpy()
        for s in range(steps):
            _, _, _, info = twin.step(acts[s])
            got = step_inputs(twin.world)
            m.step(host_acts[s], got["step_is_clean"], got["step_rewards"])
            m.reset(info["all_down"].cpu().numpy().astype(bool), got["step_dones_info"])
        torch.cuda.synchronize()
        busy = torch.randn(4096, 4096, device="cuda")
        for q in range(20):
            busy = (busy @ busy).clamp_(-1, 1)
        run.reset()
        for s in range(steps):
            run.step(acts[s])
        same_arrays(device_arrays(run.world), m.arrays(), "after %d unsynchronised steps" % steps)
        print_totals("stream order", m)
        assert m.episodes.sum() >= 4 * E and m.ends[1].sum() > 0
    finally:
        run.close()
        twin.close()


# ---- the probe's torch variant is the same computation ----
def test_the_probes_torch_episodes_keep_the_same_figures():
    """tools/vec_env_probe.py --episodes-compare measures the library against the same statistics kept with EpisodeStats and torch
    ops on a plain VecImageEnv: both must arrive at the same pooled figures, or the comparison compares nothing"""
    import torch
    from img_env_amd.vec_env import VecImageEnv
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from vec_env_probe import TorchEpisodes
    E, R, P = 24, 2, 3
    cfg = episode_cfg(R, P)
    lib = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, episode_stats=True)
    ref = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True)
    try:
        te = TorchEpisodes(ref)
        lib.reset()
        ref.reset()
        te.reset()
        rng = np.random.default_rng(2)
        for s in range(30):
            a = torch.as_tensor(policy(rng, ref.world.out["vector_states"].cpu().numpy()), device="cuda")
            lib.step(a)
            _, rew, _, info = ref.step(a)
            te.push(a, rew, info)
        want, got = lib.episode_statistics(), te.statistics()
        assert want["episodes"] > E
        for k, v in want.items():
            assert got[k] == pytest.approx(v, rel=1e-9, abs=1e-12), k
    finally:
        lib.close()
        ref.close()
