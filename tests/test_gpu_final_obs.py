"""The final observations on the device (imgenv_final_obs_enable, csrc/final_obs.h: every reset chain first copies the rows it is
about to overwrite).  The kernel only moves bytes, so every comparison is exact: bit patterns, no tolerance.  What a final row must
hold is what ``world.snapshot()`` showed for it before the reset -- taken by the caller where the caller resets, and on a replayed
twin handle, which takes the step in question with plain ``World.step`` (no reset), where the library resets on its own."""
import copy
import ctypes as C

import numpy as np
import pytest

from scenarios import random_actions, small_world
from stack_model import bits

pytestmark = pytest.mark.gpu
IMAGE_STATE = ("vector_states", "sensor_maps", "lasers", "ped_vector_states", "ped_maps", "is_collisions", "is_arrives", "step_ds",
               "ped_min_dists")
WRAPPERS = ["VelActionWrapper", "TimeLimitWrapper", "SensorsPaperRewardWrapper", "InfoLogWrapper", "MultiRobotCleanWrapper",
            "StatePedVectorWrapper"]
TABLE8 = [[0.0, -0.9], [0.0, 0.3], [0.2, -0.6], [0.2, 0.0], [0.4, 0.6], [0.6, -0.3], [0.6, 0.0, 1], [0.6, 0.9]]


def same(got, want, where):
    g, w = np.asarray(got), np.asarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (where, g.dtype, w.dtype, g.shape, w.shape)
    eq = (g == w) if g.dtype.itemsize == 1 else (bits(g) == bits(w))
    if not eq.all():
        at = np.argwhere(~eq)[0]
        raise AssertionError("%s differs at %s: got %r, want %r (%d of %d)" % (where, at.tolist(), g[tuple(at)], w[tuple(at)],
                                                                                 (~eq).sum(), eq.size))


def host(tensors):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in tensors.items()}


def env_rows(envs, E, R):
    rows = np.zeros(E * R, bool)
    for k in envs:
        rows[k * R:(k + 1) * R] = True
    return rows


def narrow_cfg(R, P, **over):
    """the sizes of tests/test_gpu_stack.py's out-of-phase cases, with 181 beams (1448-byte scans: 8-byte chunks) and 5 vector states
    (20 bytes: 4-byte chunks) beside the 16-byte chunks of the maps and the one-byte flags"""
    from img_env_amd import worldgen
    grid = worldgen.make_grid(200, 3)
    return worldgen.make_yaml_cfg(R, P, grid, time_max=5, n_obstacles=3, seed=9, state_dim=5, beams=181, **over)


def fixed_actions(steps, n, seed=2):
    rng = np.random.default_rng(seed)
    a = np.zeros((steps, n, 3), np.float32)
    a[:, :, 0], a[:, :, 1] = rng.uniform(0, 0.6, (steps, n)), rng.uniform(-0.9, 0.9, (steps, n))
    return a


# ---- 3. the caller resets: listed chains from the host ----
def test_final_rows_hold_what_the_reset_envs_showed_before_their_reset():
    """5 envs x 3 robots x 2 pedestrians, auto_reset=False, 14 steps: after each step the finished envs are reset by the caller
    (imgenv_reset_worlds), at step 2 env 1 as well, which puts it out of phase with the others.  The model keeps, per row, the
    snapshot of before the row's last reset and the number of its resets; the final arrays equal it as a whole after every reset
    -- the rows of the reset envs new, every other row and count as they were."""
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, steps = 5, 3, 2, 14
    n = E * R
    vec = VecImageEnv(narrow_cfg(R, P), env_num=E, seed=9, auto_reset=False, final_obs=True)
    try:
        fin = vec.world.final_obs
        assert set(fin) == set(IMAGE_STATE) | {"final_count"}
        for f in IMAGE_STATE:
            assert fin[f].shape == vec.world.out[f].shape and fin[f].dtype == vec.world.out[f].dtype, f
            assert fin[f].data_ptr() != vec.world.out[f].data_ptr() and fin[f].data_ptr() % 256 == 0, f
        assert fin["lasers"].shape == (n, 181) and fin["vector_states"].shape == (n, 5)
        vec.reset()
        model = {f: np.zeros_like(v) for f, v in host(fin).items()}
        for f, v in host(fin).items():  # the handle's first reset captures nothing
            same(v, model[f], "first reset: %s" % f)

        def reset_and_check(envs, where):
            before = vec.world.snapshot()
            vec.reset_envs(envs)
            rows = env_rows(envs, E, R)
            for f in IMAGE_STATE:
                model[f][rows] = before[f][rows]
            model["final_count"][rows] += 1
            got = host(fin)
            for f in model:
                same(got[f], model[f], "%s: %s" % (where, f))
            new = vec.world.snapshot()["vector_states"]
            assert (bits(got["vector_states"][rows]) != bits(new[rows])).any(axis=1).all(), where  # from BEFORE the reset
            return before, rows
        acts = fixed_actions(steps, n)
        partial = timeouts = captures = 0
        for s in range(steps):
            state, rew, done, info = vec.step(torch.as_tensor(acts[s], device="cuda"))
            assert info["final_observation"].vector_states.data_ptr() == fin["vector_states"].data_ptr()
            assert info["final_count"].data_ptr() == fin["final_count"].data_ptr()
            finished = torch.nonzero(info["all_down"].view(E, R).all(dim=1)).flatten().tolist()
            if finished:
                before, rows = reset_and_check(finished, "step %d, envs %s" % (s, finished))
                partial += len(finished) < E
                timeouts += int((before["dones_info"][rows] == 10).sum())
                captures += len(finished)
            if s == 2:
                reset_and_check([1], "step 2, env 1 by hand")
        assert partial >= 1 and timeouts >= 1 and captures >= E, (partial, timeouts, captures)
    finally:
        vec.close()


# ---- 4. the library resets: imgenv_step_autoreset and imgenv_step_autoreset_device ----
def _make(cfg, E, device_reset, final_obs, **kw):
    from img_env_amd.vec_env import VecImageEnv
    return VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=True, device_reset=device_reset, final_obs=final_obs, **kw)


def _run_recorded(vec, acts, E, R):
    """handle A: T steps through the auto-reset call (env 1 reset by hand after step 2); all_down, the final arrays and the ordinary
    outputs after every step"""
    import torch
    vec.reset()
    downs, finals, outs = [], [], []
    for s in range(len(acts)):
        raw = acts[s]
        state, rew, done, info = vec.step(raw if vec.wrappers else torch.as_tensor(raw, device="cuda"))
        if s == 2:
            vec.reset_envs([1])
        torch.cuda.synchronize()
        downs.append(info["all_down"].cpu().numpy().astype(bool))
        finals.append(host(vec.world.final_obs))
        outs.append(vec.world.snapshot())
    return downs, finals, outs


def _replay(twin, acts, t, outs, with_reset_at_2=True):
    """a fresh handle without the feature: steps < t through the same auto-reset call -- its ordinary outputs must equal A's on every
    one of them -- then step t with plain World.step, which resets nothing"""
    import torch
    twin.reset()
    for s in range(t):
        raw = acts[s]
        twin.step(raw if twin.wrappers else torch.as_tensor(raw, device="cuda"))
        if s == 2 and with_reset_at_2:
            twin.reset_envs([1])
        snap = twin.world.snapshot()
        assert set(snap) == set(outs[s])
        for f in snap:
            assert snap[f].tobytes() == outs[s][f].tobytes(), ("step %d of the replay up to %d" % (s, t), f)
    twin.world.step(twin._actions(acts[t] if twin.wrappers else torch.as_tensor(acts[t], device="cuda")))
    return twin.world.snapshot()


def _steps_to_replay(downs, E, R, want=3):
    """`want` steps on which envs finished, one of them a step on which some did and others did not"""
    hit = [t for t, d in enumerate(downs) if d.any() and t != 2]  # (step 2 is followed by the reset by hand, which captures env 1 once more)
    part = [t for t in hit if 0 < d_envs(downs[t], E, R) < E]
    assert len(hit) >= want and part, (hit, part)
    pick = hit[:want] if set(hit[:want]) & set(part) else hit[:want - 1] + [part[0]]
    return sorted(pick)


def d_envs(down, E, R):
    return int(down.reshape(E, R).all(axis=1).sum())


@pytest.mark.parametrize("device_reset", [False, True], ids=["step_autoreset", "step_autoreset_device"])
def test_final_rows_of_an_auto_reset_equal_the_step_replayed_without_a_reset(device_reset):
    E, R, P, T = 5, 3, 2, 12
    cfg = narrow_cfg(R, P)
    acts = fixed_actions(T, E * R)
    a = _make(cfg, E, device_reset, True)
    try:
        downs, finals, outs = _run_recorded(a, acts, E, R)
    finally:
        a.close()
    # final_count: one more on the rows of the envs that finished, and on env 1's at its reset by hand
    count = np.zeros(E * R, np.int32)
    for t in range(T):
        count += downs[t]
        if t == 2:
            count += env_rows([1], E, R)
        same(finals[t]["final_count"], count, "final_count after step %d" % t)
    for t in _steps_to_replay(downs, E, R):
        twin = _make(cfg, E, device_reset, False)
        try:
            assert twin.world.final_obs is None
            snap = _replay(twin, acts, t, outs)
        finally:
            twin.close()
        rows = downs[t]
        assert rows.any()
        for f in IMAGE_STATE:
            same(finals[t][f][rows], snap[f][rows], "step %d: %s" % (t, f))
            if t > 0:  # the rows of the envs that went on are older captures, untouched
                same(finals[t][f][~rows], finals[t - 1][f][~rows], "step %d, the other rows: %s" % (t, f))
        assert (bits(finals[t]["vector_states"][rows]) != bits(outs[t]["vector_states"][rows])).any(axis=1).all(), t


# ---- 5. stacks and the normalised pedestrian vector ----
def test_final_stacks_and_normalised_vector_equal_the_replayed_handles_before_its_restart():
    """stack=True with batches (2, 3, 2), wrappers=True on a YAML that lists StatePedVectorWrapper, device-side resets: the final
    stack rows are the twin's stacks after its push of step t and before any restart, ped_vector_norm likewise; the state handed out
    in info["final_observation"] is an ImageState over exactly those arrays"""
    E, R, P, T = 5, 3, 2, 10
    cfg = narrow_cfg(R, P, max_ped=10, wrappers=WRAPPERS, discrete_action=True, discrete_actions=TABLE8, image_batch=2, state_batch=3,
                     laser_batch=2)
    acts = np.random.default_rng(3).integers(0, len(TABLE8), (T, E * R)).astype(np.int64)
    a = _make(cfg, E, True, True, stack=True, wrappers=True)
    try:
        fin = a.world.final_obs
        assert {"stack_sensor_maps", "stack_vector_states", "stack_lasers", "ped_vector_norm"} <= set(fin)
        for f in ("sensor_maps", "vector_states", "lasers"):
            assert fin["stack_" + f].shape == a.world.stack[f].shape and fin["stack_" + f].dtype == a.world.stack[f].dtype, f
        assert fin["stack_sensor_maps"].shape == (E * R, 2, 48, 48) and fin["stack_vector_states"].shape == (E * R, 15)
        assert fin["stack_lasers"].shape == (E * R, 2, 181) and fin["ped_vector_norm"].shape == (E * R, 71)
        downs, finals, outs = _run_recorded(a, acts, E, R)
        info = a.step(acts[0])[3]
        st = info["final_observation"]
        assert st.vector_states.data_ptr() == fin["stack_vector_states"].data_ptr()
        assert st.sensor_maps.data_ptr() == fin["stack_sensor_maps"].data_ptr() and st.lasers.data_ptr() == fin["stack_lasers"].data_ptr()
        assert st.ped_vector_states.data_ptr() == fin["ped_vector_norm"].data_ptr() and st.ped_maps.data_ptr() == fin["ped_maps"].data_ptr()
        assert st.is_collisions.data_ptr() == fin["is_collisions"].data_ptr() and st.step_ds.data_ptr() == fin["step_ds"].data_ptr()
    finally:
        a.close()
    replayed = 0
    for t in _steps_to_replay(downs, E, R, want=2):
        twin = _make(cfg, E, True, False, stack=True, wrappers=True)
        try:
            snap = _replay(twin, acts, t, outs)
            stacks, norm = host(twin.world.stack), host({"n": twin.world.obs_post["ped_vector_norm"]})["n"]
        finally:
            twin.close()
        rows = downs[t]
        for f in ("sensor_maps", "vector_states", "lasers"):
            same(finals[t]["stack_" + f][rows], stacks[f][rows], "step %d: stack of %s" % (t, f))
        same(finals[t]["ped_vector_norm"][rows], norm[rows], "step %d: ped_vector_norm" % t)
        same(finals[t]["ped_vector_states"][rows], snap["ped_vector_states"][rows], "step %d: the raw vector" % t)
        assert (finals[t]["ped_vector_norm"][rows] != finals[t]["ped_vector_states"][rows]).any()  # (normalised: not the raw row)
        older = finals[t]["stack_vector_states"][rows].reshape(-1, 3, 5)[:, :2]
        assert (older != 0).any()  # (a stack of before the restart: its older slots are not the restart's zero padding)
        replayed += 1
    assert replayed == 2


def test_final_observation_takes_the_filter_wrappers_list_form():
    """a wrapper list that ends in ObsLaserStateTmp: the state and the final observation are [lasers, vector_states, ped_maps]; a
    stack of depth 1 (image_batch 1) is the final field itself"""
    import torch
    E, R, P = 2, 2, 2
    cfg = narrow_cfg(R, P, wrappers=WRAPPERS[:5] + ["StateBatchWrapper", "ObsLaserStateTmp"], image_batch=1, state_batch=3, laser_batch=2)
    vec = _make(cfg, E, True, True, stack=True)
    try:
        fin = vec.world.final_obs
        assert "stack_sensor_maps" not in fin and "stack_lasers" in fin
        vec.reset()
        info = vec.step(torch.as_tensor(fixed_actions(1, E * R)[0], device="cuda"))[3]
        st = info["final_observation"]
        assert isinstance(st, list) and len(st) == 3
        assert [t.data_ptr() for t in st] == [fin["stack_lasers"].data_ptr(), fin["stack_vector_states"].data_ptr(), fin["ped_maps"].data_ptr()]
        full = vec._state(final=True)
        assert isinstance(full, list)
        vec._filter = None
        full = vec._state(final=True)
        assert full.sensor_maps.data_ptr() == fin["sensor_maps"].data_ptr() and full.sensor_maps.shape == vec.world.stack["sensor_maps"].shape
    finally:
        vec.close()


# ---- 6. a reset without a list, and more chunks than one pass of the grid ----
def test_imgenv_reset_captures_every_row_through_the_grid_stride_loop():
    """300 envs x 4 robots, no pedestrians, as ONE imgenv_reset batch (no world list): the second reset captures all 1200 rows, more
    chunks than FINAL_MAX_BLOCKS x FINAL_BLOCK lanes take in one pass; the first leaves final_count at 0"""
    import torch
    from img_env_amd import _cabi, worldgen
    from img_env_amd.vec_env import VecImageEnv
    E, R = 300, 4
    n = E * R
    cfg = narrow_cfg(R, 0)
    grid = cfg["global_map"]["map_array"]
    vec = VecImageEnv(cfg, env_num=E, seed=9, auto_reset=False, final_obs=True)
    try:
        fin = vec.world.final_obs

        def batch(seed):  # every world gets the same cast: the worlds are independent, and their robots are driven differently
            lay = worldgen.make_layout(grid, 0.125, R, 0, seed=seed, n_obstacles=3).as_batch()
            return dict(lay, robot_pose=np.tile(lay["robot_pose"], (E, 1)), robot_goal=np.tile(lay["robot_goal"], (E, 1)))
        row_bytes = [int(np.prod(fin[f].shape[1:])) * fin[f].element_size() for f in IMAGE_STATE]
        chunks = sum(b // next(u for u in (16, 8, 4, 2, 1) if b % u == 0) for b in row_bytes)
        assert n * chunks > _cabi.FINAL_MAX_BLOCKS * _cabi.FINAL_BLOCK, (chunks, n * chunks)
        vec.world.reset(batch(11))
        first = host(fin)
        assert (first["final_count"] == 0).all() and not any(v.any() for v in first.values())
        acts = fixed_actions(2, n, seed=5)
        for s in range(2):
            vec.world.step(torch.as_tensor(acts[s], device="cuda"))
        before = vec.world.snapshot()
        vec.world.reset(batch(12))
        got = host(fin)
        assert (got["final_count"] == 1).all()
        for f in IMAGE_STATE:
            same(got[f], before[f], f)
        after = vec.world.snapshot()
        assert (bits(got["vector_states"]) != bits(after["vector_states"])).any(axis=1).all()
        assert (bits(before["vector_states"]).reshape(E, -1) != bits(before["vector_states"]).reshape(E, -1)[0]).any(axis=1).sum() >= E - 2  # (the worlds differ)
    finally:
        vec.close()


# ---- 7. no cost when off, one launch per reset chain when on ----
@pytest.mark.parametrize("device_reset", [False, True], ids=["native_spawn", "device_reset"])
def test_the_feature_disturbs_nothing_and_costs_one_launch_per_reset_chain(device_reset):
    """same cfg, seed and actions on a handle without the feature and on one with it: every output byte equal on every step;
    ``imgenv_step_launches`` differs by exactly one per reset chain -- none for the handle's first reset, which captures nothing.
    After imgenv_step_autoreset_device the count covers the step's chain and the reset chain behind it: always 1 more.  After
    imgenv_step_autoreset it covers the last chain alone: 1 more where a world was reset, 0 where the call only stepped, and both
    kinds of call must occur.  A plain step chain: 0."""
    import torch
    E, R, P, T = 5, 3, 2, 12
    cfg = narrow_cfg(R, P)
    acts = fixed_actions(T, E * R)
    off, on = _make(cfg, E, device_reset, False), _make(cfg, E, device_reset, True)
    try:
        assert off.world.final_obs is None
        for v in (off, on):
            v.reset()
        assert on.world.launches() == off.world.launches()
        extra = set()
        for s in range(T):
            a = torch.as_tensor(acts[s], device="cuda")
            infos = [v.step(a)[3] for v in (off, on)]
            assert "final_observation" not in infos[0] and "final_observation" in infos[1]
            sa, sb = off.world.snapshot(), on.world.snapshot()
            assert set(sa) == set(sb)
            for f in sa:
                assert sa[f].tobytes() == sb[f].tobytes(), (s, f)
            diff = on.world.launches() - off.world.launches()
            if device_reset:
                assert diff == 1, (s, diff)
            else:
                assert infos[0]["reset_envs"] == infos[1]["reset_envs"], s
                assert diff == (1 if infos[0]["reset_envs"] else 0), (s, diff, infos[0]["reset_envs"])
            extra.add(diff)
        assert extra == ({1} if device_reset else {0, 1}), extra
        for v in (off, on):
            v.world.step(torch.as_tensor(acts[0], device="cuda"))
        assert on.world.launches() == off.world.launches()
        for v in (off, on):
            v.reset_envs([0, 3])
        assert on.world.launches() == off.world.launches() + 1
    finally:
        off.close()
        on.close()


# ---- the entry points on a live handle ----
def test_enable_refuses_what_the_header_says_and_is_legal_at_any_time():
    from img_env_amd import _cabi
    from img_env_amd.world import World
    n = 6
    grid, params, layout = small_world(n, 3, seed=4)
    _, _, layout2 = small_world(n, 3, seed=5)
    w = World(dict(params, output_guard="copy"), grid)  # IMGENV_FLAG_FULL_REWRITE: the copy is taken from the working arena
    no_laser = World(dict(params, use_laser=0), grid)
    no_views = World(dict(params, flags=_cabi.FLAG_NO_VIEW_MAPS), grid)
    shallow = World(params, grid)
    try:
        o = _cabi.FinalObsOut()
        assert w.lib.imgenv_final_obs_outputs(w.h, C.byref(o)) == _cabi.ESTATE
        with pytest.raises(RuntimeError, match="imgenv_stack_enable"):
            w.enable_final_obs(["vector_states", "stacks"])
        with pytest.raises(RuntimeError, match="imgenv_obs_post_enable"):
            w.enable_final_obs(["ped_vector_norm"])
        with pytest.raises(ValueError, match="unknown"):
            w.enable_final_obs(["vector_state"])
        with pytest.raises(ValueError, match="use_laser"):
            no_laser.enable_final_obs(["lasers"])
        with pytest.raises(ValueError, match="use_laser"):
            no_laser.enable_final_obs(["lasers_raw", "vector_states"])
        assert "lasers" not in no_laser.enable_final_obs() and "sensor_maps" in no_laser.final_obs
        with pytest.raises(ValueError, match="NO_VIEW_MAPS"):
            no_views.enable_final_obs(["view_maps"])
        shallow.enable_stack(1, 1, 0)
        with pytest.raises(ValueError, match="deeper than 1"):
            shallow.enable_final_obs(["stacks"])
        assert w.final_obs is None
        # legal at any time: after a reset and a step
        rng = np.random.default_rng(0)
        w.reset(layout)
        w.step(random_actions(rng, n))
        launches = w.launches()
        fin = w.enable_final_obs(["vector_states", "view_maps", "lasers_raw", "is_collisions"])
        assert set(fin) == {"vector_states", "view_maps", "lasers_raw", "is_collisions", "final_count"} and w.launches() == launches
        assert w.enable_final_obs(["is_collisions", "vector_states", "view_maps", "lasers_raw"]) is fin  # the same bits: nothing changes
        with pytest.raises(ValueError, match="already"):
            w.enable_final_obs()
        assert w.lib.imgenv_final_obs_outputs(w.h, C.byref(o)) == 0 and o.vector_states == fin["vector_states"].data_ptr()
        assert o.sensor_maps is None and o.final_count == fin["final_count"].data_ptr() and o.n_local == n
        assert not any(v.any() for v in host(fin).values())
        before = w.snapshot()
        w.reset(layout2)
        got = host(fin)
        assert (got["final_count"] == 1).all()
        for f in ("vector_states", "view_maps", "lasers_raw", "is_collisions"):
            same(got[f], before[f], f)
        assert (got["view_maps"] != w.snapshot()["view_maps"]).any()
    finally:
        for x in (w, no_laser, no_views, shallow):
            x.close()
