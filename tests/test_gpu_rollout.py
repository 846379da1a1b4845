"""The rollout storage on the device (imgenv_rollout_enable / _begin / _gae, csrc/rollout.h: the last launch of every chain stores
the transition and the observation it led to, a reset chain first moves the rows it overwrites into a final list; the advantage
pass walks the result).  The storage kernel moves bytes and rounds one double, the pass is float32 in a fixed order, so every
comparison is exact: bit patterns, no tolerance.  Shapes are tests/test_gpu_final_obs.py's narrow_cfg unless a test says otherwise."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import rollout_model
from scenarios import random_actions, small_world
from test_gpu_final_obs import TABLE8, WRAPPERS, env_rows, fixed_actions, host, narrow_cfg, same

pytestmark = pytest.mark.gpu
SINGLE = ("sensor_maps", "vector_states", "lasers", "ped_vector_states", "ped_maps")
# case 1's stored fields and the member of the state handed out that each of them is
STATE_OF = {"stack_sensor_maps": "sensor_maps", "stack_vector_states": "vector_states", "stack_lasers": "lasers",
            "ped_vector_norm": "ped_vector_states", "ped_maps": "ped_maps"}
SCALARS = ("actions", "rewards", "dones", "is_clean", "dones_info", "final_idx", "final_slot", "final_row")


def ring(vec):
    """host copies of the ring, with the cursor and the count of final entries"""
    r = vec.rollout()
    n, resets = r.pop("n"), r.pop("resets")
    r = host(r)
    r.update(n=n, resets=resets, final_count=int(r["final_n"][resets & 1]))
    return r


def state_fields(state):
    import torch
    torch.cuda.synchronize()
    return {f: getattr(state, f).cpu().numpy().copy() for f in STATE_OF.values()}


# ---- 1. the library resets, with stacks, the wrappers and final_obs on the same handle; 7. the advantage pass on that rollout ----
@functools.lru_cache(maxsize=None)
def case1(device_reset):
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T, F = 5, 3, 2, 7, 64
    cfg = narrow_cfg(R, P, max_ped=10, wrappers=WRAPPERS, discrete_action=True, discrete_actions=TABLE8, image_batch=2, state_batch=3,
                     laser_batch=2)
    acts = np.random.default_rng(3).integers(0, len(TABLE8), (T, E * R)).astype(np.int64)
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=True, device_reset=device_reset, final_obs=True, stack=True,
                      wrappers=True, rollout=T, rollout_final=F)
    try:
        rec = {"first": state_fields(vec.reset()), "steps": [], "shapes": {k: (tuple(v.shape), str(v.dtype)) for k, v in vec.world.rollout.items()}}
        rec["live_shapes"] = {f: tuple(getattr(vec._state(), m).shape) for f, m in STATE_OF.items()}
        for t in range(T):
            state, rew, done, info = vec.step(acts[t])
            torch.cuda.synchronize()  # (recording what every step returned; the ring does not depend on it)
            rec["steps"].append({"state": state_fields(state), "final": state_fields(info["final_observation"]),
                                 "rewards": rew.cpu().numpy().copy(), "dones": done.cpu().numpy().copy(),
                                 "dones_info": info["dones_info"].cpu().numpy().copy(), "is_clean": info["is_clean"].cpu().numpy().copy(),
                                 "all_down": info["all_down"].cpu().numpy().astype(bool),
                                 "actions": vec.world.action_outputs["actions"].cpu().numpy().copy()})
        rec["ring"] = ring(vec)
        g = torch.Generator(device="cpu").manual_seed(11)
        values, fv = torch.randn((T + 1, E * R), generator=g).cuda(), torch.randn(F, generator=g).cuda()
        keep = torch.full((T, E * R), 7.0, device="cuda")
        adv, ret = vec.rollout_advantages(values, fv, 0.99, 0.95)
        adv0, ret0 = vec.world.rollout_gae(values, None, 0.5, 0.5, adv=keep.clone(), ret=keep.clone())
        rec["gae"] = host({"values": values, "final_values": fv, "adv": adv, "ret": ret, "adv0": adv0, "ret0": ret0})
        with pytest.raises(ValueError):
            vec.rollout_advantages(values[:-1], fv, 0.99, 0.95)
    finally:
        vec.close()
    return rec, (E, R, T, F)


@pytest.mark.parametrize("device_reset", [True, False], ids=["device_reset", "native_spawn"])
def test_ring_holds_what_every_step_handed_out(device_reset):
    rec, (E, R, T, F) = case1(device_reset)
    r, n = rec["ring"], E * R
    assert r["n"] == T
    assert {"obs_" + f for f in STATE_OF} | {"final_" + f for f in STATE_OF} | set(SCALARS) | {"final_n"} == set(rec["shapes"])
    for f in STATE_OF:  # what the state handed out consists of: the whole stacks, the normalised vector, ped_maps
        assert rec["shapes"]["obs_" + f][0] == (T + 1,) + rec["live_shapes"][f] and rec["shapes"]["final_" + f][0] == (F,) + rec["live_shapes"][f][1:]
    assert rec["shapes"]["obs_stack_lasers"] == ((T + 1, n, 2, 181), "torch.float64") and rec["shapes"]["final_ped_vector_norm"] == ((F, 71), "torch.float32")
    for f, member in STATE_OF.items():
        same(r["obs_" + f][0], rec["first"][member], "slot 0: %s" % f)
    restarted = np.zeros(E, bool)
    for t, s in enumerate(rec["steps"]):
        for f, member in STATE_OF.items():
            same(r["obs_" + f][t + 1], s["state"][member], "slot %d: %s" % (t + 1, f))
        same(r["rewards"][t], s["rewards"].astype(np.float32), "rewards %d" % t)
        same(r["actions"][t], s["actions"], "actions %d" % t)
        for f in ("dones", "dones_info", "is_clean"):
            same(r[f][t], s[f], "%s %d" % (f, t))
        idx = r["final_idx"][t + 1]
        assert ((idx >= 0) == s["all_down"]).all(), t
        assert (idx < F).all()
        for row in np.nonzero(idx >= 0)[0]:
            e = idx[row]
            assert r["final_slot"][e] == t + 1 and r["final_row"][e] == row, (t, row, e)
            for f, member in STATE_OF.items():
                same(r["final_" + f][e], s["final"][member][row], "step %d, row %d: final %s" % (t, row, f))
        restarted |= s["all_down"].reshape(E, R).all(axis=1)
    assert (r["final_idx"][0] == -1).all()
    assert restarted.all(), restarted  # time_max 5 < T: every env restarts inside the window
    assert r["final_count"] == int((r["final_idx"] >= 0).sum()) and sorted(r["final_idx"][r["final_idx"] >= 0]) == list(range(r["final_count"]))
    assert (r["dones_info"] == 10).any()  # (time-outs, for the pass below)


@pytest.mark.parametrize("device_reset", [True, False], ids=["device_reset", "native_spawn"])
def test_advantage_pass_equals_the_model(device_reset):
    rec, (E, R, T, F) = case1(device_reset)
    g = rec["gae"]
    adv, ret = rollout_model.gae(rec["ring"], g["values"], g["final_values"], 0.99, 0.95, F)
    same(g["adv"], adv, "adv")
    same(g["ret"], ret, "ret")
    assert (adv != 0).any()
    adv0, ret0 = rollout_model.gae(rec["ring"], g["values"], None, 0.5, 0.5, F)  # no final values
    same(g["adv0"], adv0, "adv without final_values")
    same(g["ret0"], ret0, "ret without final_values")
    assert (g["adv0"] != g["adv"]).any()


# ---- 2. the caller resets (Python spawn), one env in mid-episode; 3. a final list that overflows ----
def snapshot_chain(snap, actions):
    return {"kind": "step", "obs": {f: snap[f] for f in SINGLE}, "actions": actions, "rewards": snap["step_rewards"], "dones": snap["step_dones"],
            "is_clean": snap["step_is_clean"], "dones_info": snap["step_dones_info"]}


@pytest.mark.parametrize("F", [64, 4], ids=["F64", "F4"])
def test_caller_resets_against_the_model(F):
    """auto_reset=False, 7 steps: after each step the caller resets the finished envs (Python spawn, imgenv_reset_worlds), after
    step 2 env 1 as well -- a restart without done.  The whole ring equals the model's replay of the recorded chains.  F = 4: more
    restarts than entries; the kept entries and the ring are as with room for all, final_n counts them all, final_idx goes beyond F"""
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T = 5, 3, 2, 7
    vec = VecImageEnv(narrow_cfg(R, P), env_num=E, seed=9, auto_reset=False, rollout=T, rollout_final=F)
    try:
        assert set(vec.world.rollout) == {"obs_" + f for f in SINGLE} | {"final_" + f for f in SINGLE} | set(SCALARS) | {"final_n"}
        vec.reset()
        first = {f: vec.world.snapshot()[f] for f in SINGLE}
        acts, chains, undone = fixed_actions(T, E * R), [], 0
        for t in range(T):
            state, rew, done, info = vec.step(torch.as_tensor(acts[t], device="cuda"))
            snap = vec.world.snapshot()
            chains.append(snapshot_chain(snap, acts[t]))
            finished = torch.nonzero(info["all_down"].view(E, R).all(dim=1)).flatten().tolist()
            for envs in ([finished] if finished else []) + ([[1]] if t == 2 and 1 not in finished else []):
                vec.reset_envs(envs)
                rows = np.nonzero(env_rows(envs, E, R))[0].tolist()
                undone += int((snap["step_dones"][rows] == 0).sum())
                chains.append({"kind": "reset", "rows": rows, "obs": {f: vec.world.snapshot()[f] for f in SINGLE}})
        got, want = ring(vec), rollout_model.replay(T, F, first, chains)
    finally:
        vec.close()
    assert undone > 0  # (a restart without done)
    assert got["n"] == want["n"] == T and got["resets"] == want["resets"] and got["final_count"] == want["final_count"]
    for f in want:
        if f not in ("n", "resets", "final_count", "final_n"):
            same(got[f], want[f], f)
    restarts = int((want["final_idx"] >= 0).sum())
    assert restarts >= E * R
    if F == 4:
        assert want["final_count"] > F and (got["final_idx"] >= F).any() and (got["final_slot"] > 0).all()
    else:
        assert want["final_count"] <= F


# ---- 4. the full ring, and the next window ----
@pytest.mark.parametrize("mode", ["python_spawn", "native_spawn", "device_reset"])
def test_full_ring_refuses_the_step_and_begin_starts_over(mode):
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T = 5, 3, 2, 3
    kw = {"python_spawn": {}, "native_spawn": {"native_spawn": True}, "device_reset": {"device_reset": True}}[mode]
    vec = VecImageEnv(narrow_cfg(R, P), env_num=E, seed=9, rollout=T, rollout_final=8, **kw)
    try:
        acts = fixed_actions(T + 2, E * R)
        vec.reset()
        for t in range(T):
            vec.step(torch.as_tensor(acts[t], device="cuda"))
        before, out_before, launches = ring(vec), vec.world.snapshot(), vec.world.launches()
        assert before["n"] == T
        with pytest.raises(RuntimeError, match="rollout full: imgenv_rollout_begin"):
            vec.step(torch.as_tensor(acts[T], device="cuda"))
        with pytest.raises(RuntimeError, match="rollout full: imgenv_rollout_begin"):
            vec.world.step_begin(torch.as_tensor(acts[T], device="cuda"))
        after, out_after = ring(vec), vec.world.snapshot()
        for f in before:  # nothing was queued
            assert np.asarray(before[f]).tobytes() == np.asarray(after[f]).tobytes(), f
        for f in out_before:
            assert out_before[f].tobytes() == out_after[f].tobytes(), f
        vec.rollout_begin()
        now = ring(vec)
        assert now["n"] == 0 and now["resets"] == 0 and now["final_count"] == 0 and (now["final_n"] == 0).all()
        assert (now["final_idx"] == -1).all()
        for f in SINGLE:
            same(now["obs_" + f][0], before["obs_" + f][T], "slot 0 after begin: %s" % f)
            same(now["obs_" + f][1:], before["obs_" + f][1:], "the other slots: %s" % f)
        vec.step(torch.as_tensor(acts[T], device="cuda"))  # ... and the next window fills
        nxt = ring(vec)
        assert nxt["n"] == 1
        same(nxt["obs_vector_states"][0], before["obs_vector_states"][T], "slot 0 stays")
        assert (nxt["obs_vector_states"][1] != before["obs_vector_states"][1]).any()
        vec.rollout_begin()  # begin in mid-window: slot 1 -> slot 0
        same(ring(vec)["obs_vector_states"][0], nxt["obs_vector_states"][1], "begin in mid-window")
    finally:
        vec.close()


# ---- 5. a reset without a list through the grid-stride loop; 7. the advantage pass at 1200 rows ----
def test_imgenv_reset_keeps_1200_final_entries_and_the_pass_strides():
    """300 envs x 4 robots, no pedestrians, T = 2, as ONE imgenv_reset batch (no world list) behind two steps: 1200 final entries in
    row order, more chunks than ROLLOUT_MAX_BLOCKS x ROLLOUT_BLOCK lanes take in one pass (tests/test_gpu_final_obs.py's shape for
    the same cap); then the advantage pass over 1200 rows against the model"""
    import torch
    from img_env_amd import _cabi, worldgen
    from img_env_amd.vec_env import VecImageEnv
    E, R, T = 300, 4, 2
    n = E * R
    cfg = narrow_cfg(R, 0)
    grid = cfg["global_map"]["map_array"]
    vec = VecImageEnv(cfg, env_num=E, seed=9, auto_reset=False, rollout=T, rollout_final=n)
    try:
        ro = vec.world.rollout
        fields = [f for f in SINGLE if "obs_" + f in ro]

        def batch(seed):  # every world gets the same cast: the worlds are independent, and their robots are driven differently
            lay = worldgen.make_layout(grid, 0.125, R, 0, seed=seed, n_obstacles=3).as_batch()
            return dict(lay, robot_pose=np.tile(lay["robot_pose"], (E, 1)), robot_goal=np.tile(lay["robot_goal"], (E, 1)))
        row_bytes = [int(np.prod(ro["obs_" + f].shape[2:])) * ro["obs_" + f].element_size() for f in fields]
        chunks = sum(b // next(u for u in (16, 8, 4, 2, 1) if b % u == 0) for b in row_bytes)
        assert n * chunks > _cabi.ROLLOUT_MAX_BLOCKS * _cabi.ROLLOUT_BLOCK, (chunks, n * chunks)
        with pytest.raises(RuntimeError, match="before the first reset"):
            vec.rollout_begin()
        vec.world.reset(batch(11))
        vec.rollout_begin()
        first = vec.world.snapshot()
        acts = fixed_actions(T, n, seed=5)
        snaps = []
        for s in range(T):
            vec.world.step(torch.as_tensor(acts[s], device="cuda"))
            snaps.append(vec.world.snapshot())
        vec.world.reset(batch(12))
        after, got = vec.world.snapshot(), ring(vec)
        assert got["n"] == T and got["resets"] == 1 and got["final_count"] == n
        same(got["final_idx"][T], np.arange(n, dtype=np.int32), "final_idx")
        assert (got["final_idx"][:T] == -1).all()
        same(got["final_row"], np.arange(n, dtype=np.int32), "final_row")
        assert (got["final_slot"] == T).all()
        for f in fields:
            same(got["obs_" + f][0], first[f], "slot 0: %s" % f)
            same(got["obs_" + f][1], snaps[0][f], "slot 1: %s" % f)
            same(got["final_" + f], snaps[1][f], "final: %s" % f)
            same(got["obs_" + f][2], after[f], "slot 2: %s" % f)
        same(got["rewards"][1], snaps[1]["step_rewards"].astype(np.float32), "rewards")
        same(got["actions"], acts, "actions")
        g = torch.Generator(device="cpu").manual_seed(12)
        values, fv = torch.randn((T + 1, n), generator=g).cuda(), torch.randn(n, generator=g).cuda()
        adv, ret = vec.rollout_advantages(values, fv, 0.99, 0.95)
        h = host({"values": values, "fv": fv, "adv": adv, "ret": ret})
        want_adv, want_ret = rollout_model.gae(got, h["values"], h["fv"], 0.99, 0.95, n)
        same(h["adv"], want_adv, "adv")
        same(h["ret"], want_ret, "ret")
    finally:
        vec.close()


# ---- 6. nothing in the storage needs the host ----
def test_steps_queued_behind_a_busy_stream_fill_the_same_ring():
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T = 5, 3, 2, 7
    acts = fixed_actions(T, E * R)
    rings = []
    for synchronised in (False, True):
        vec = VecImageEnv(narrow_cfg(R, P), env_num=E, seed=9, device_reset=True, rollout=T, rollout_final=64)
        try:
            vec.reset()
            a = [torch.as_tensor(acts[t], device="cuda") for t in range(T)]
            torch.cuda.synchronize()
            if not synchronised:  # some tens of milliseconds of work in front of the steps on their stream
                x = torch.full((4096, 4096), 1e-4, device="cuda")
                for _ in range(24):
                    x = x @ x
            for t in range(T):
                vec.step(a[t])
                if synchronised:
                    torch.cuda.synchronize()
            rings.append(ring(vec))
        finally:
            vec.close()
    assert rings[0]["n"] == T and rings[0]["final_count"] > 0
    for f in rings[0]:
        assert np.asarray(rings[0][f]).tobytes() == np.asarray(rings[1][f]).tobytes(), f


# ---- 8. no cost when off, one launch per chain when on ----
@pytest.mark.parametrize("device_reset", [False, True], ids=["native_spawn", "device_reset"])
def test_the_feature_disturbs_nothing_and_costs_one_launch_per_chain(device_reset):
    """same cfg, seed and actions on a handle without the feature and on one with it, 6 auto-reset steps: every output byte equal
    on every step.  ``imgenv_step_launches`` after imgenv_step_autoreset_device covers the step's chain and the reset chain behind it:
    2 more; after imgenv_step_autoreset it covers the last chain alone, the step's or the reset's: 1 more.  Enabled but not begun: 0."""
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T = 5, 3, 2, 6
    cfg = narrow_cfg(R, P)
    acts = fixed_actions(T + 1, E * R)
    off, on = (VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=True, device_reset=device_reset, rollout=r) for r in (0, T + 1))
    try:
        assert off.world.rollout is None and off.rollout_horizon == 0
        with pytest.raises(RuntimeError, match="rollout=T"):
            off.rollout()
        off._reset()
        on._reset()  # (VecImageEnv.reset without its rollout_begin: enabled, not begun)
        assert on.world.launches() == off.world.launches() and on.world.rollout_cursor() == (-1, 0)
        a = torch.as_tensor(acts[T], device="cuda")
        off.step(a), on.step(a)
        assert on.world.launches() == off.world.launches() and on.world.rollout_cursor() == (-1, 0)
        assert not any(v.any() for v in host(on.world.rollout).values())
        on.rollout_begin()
        resets = 0
        for s in range(T):
            a = torch.as_tensor(acts[s], device="cuda")
            infos = [v.step(a)[3] for v in (off, on)]
            sa, sb = off.world.snapshot(), on.world.snapshot()
            assert set(sa) == set(sb)
            for f in sa:
                assert sa[f].tobytes() == sb[f].tobytes(), (s, f)
            assert on.world.launches() - off.world.launches() == (2 if device_reset else 1), s
            resets += 1 if device_reset else bool(infos[1]["reset_envs"])
            assert on.world.rollout_cursor() == (s + 1, resets)
        assert resets >= 1
        for v in (off, on):
            v.reset_envs([0, 3])
        assert on.world.launches() == off.world.launches() + 1
    finally:
        off.close()
        on.close()


# ---- 9. the entry points on a live handle ----
def test_enable_refuses_what_the_header_says_and_is_legal_at_any_time():
    from img_env_amd import _cabi
    from img_env_amd.world import World
    n = 6
    grid, params, layout = small_world(n, 3, seed=4)
    _, _, layout2 = small_world(n, 3, seed=5)
    w = World(dict(params, output_guard="copy"), grid)  # IMGENV_FLAG_FULL_REWRITE: the rows are taken from the working arena
    no_laser = World(dict(params, use_laser=0), grid)
    shallow = World(params, grid)
    try:
        o = _cabi.RolloutOut()
        assert w.lib.imgenv_rollout_outputs(w.h, C.byref(o)) == _cabi.ESTATE
        assert w.lib.imgenv_rollout_begin(w.h, None) == _cabi.ESTATE
        with pytest.raises(RuntimeError, match="enable_rollout"):
            w.rollout_cursor()
        with pytest.raises(RuntimeError, match="imgenv_stack_enable"):
            w.enable_rollout(4, 4, ["vector_states", "stacks"])
        with pytest.raises(RuntimeError, match="imgenv_obs_post_enable"):
            w.enable_rollout(4, 4, ["ped_vector_norm"])
        with pytest.raises(ValueError, match="unknown"):
            w.enable_rollout(4, 4, ["vector_state"])
        with pytest.raises(ValueError, match="horizon"):
            w.enable_rollout(0, 4)
        with pytest.raises(ValueError, match="final_capacity"):
            w.enable_rollout(4, 0)
        with pytest.raises(ValueError, match="2\\^31"):
            w.enable_rollout(2 ** 31 - 2, 4)
        with pytest.raises(ValueError, match="use_laser"):
            no_laser.enable_rollout(4, 4, ["lasers", "vector_states"])
        assert "obs_lasers" not in no_laser.enable_rollout(4, 4) and "obs_sensor_maps" in no_laser.rollout
        shallow.enable_stack(1, 1, 0)
        with pytest.raises(ValueError, match="deeper than 1"):
            shallow.enable_rollout(4, 4, ["stacks"])
        assert w.rollout is None
        # legal at any time: after a reset and a step
        rng = np.random.default_rng(0)
        ro = no_laser.rollout
        with pytest.raises(RuntimeError, match="before the first reset"):
            no_laser.rollout_begin()
        w.reset(layout)
        w.step(random_actions(rng, n))
        launches = w.launches()
        ro = w.enable_rollout(2, 3, ["vector_states", "lasers"])
        assert set(ro) == {"obs_vector_states", "obs_lasers", "final_vector_states", "final_lasers", "final_n"} | set(SCALARS)
        assert ro["obs_vector_states"].shape == (3, n) + tuple(w.out["vector_states"].shape[1:]) and ro["final_lasers"].shape[0] == 3
        assert all(t.data_ptr() % 256 == 0 for t in ro.values()) and w.launches() == launches
        assert w.enable_rollout(2, 3, ["lasers", "vector_states"]) is ro  # the same cfg: nothing changes
        for other in ((3, 3, ["lasers", "vector_states"]), (2, 4, ["lasers", "vector_states"]), (2, 3, ["lasers"])):
            with pytest.raises(ValueError, match="already"):
                w.enable_rollout(*other)
        assert w.lib.imgenv_rollout_outputs(w.h, C.byref(o)) == 0 and o.obs_vector_states == ro["obs_vector_states"].data_ptr()
        assert o.obs_sensor_maps is None and o.final_n == ro["final_n"].data_ptr() and (o.n_local, o.horizon, o.final_capacity, o.n) == (n, 2, 3, -1)
        import torch
        values = torch.zeros((3, n), device="cuda")
        with pytest.raises(RuntimeError, match="imgenv_rollout_begin"):
            w.rollout_gae(values, None, 0.9, 0.9)
        w.rollout_begin()
        before = w.snapshot()
        assert w.rollout_cursor() == (0, 0)
        got = host(ro)
        same(got["obs_vector_states"][0], before["vector_states"], "slot 0 holds the live observation")
        same(got["obs_lasers"][0], before["lasers"], "slot 0 holds the live observation")
        w.reset(layout2)  # a reset chain without a list on slot 0: six entries, three kept
        got = host(ro)
        assert w.rollout_cursor() == (0, 1) and got["final_n"].tolist() == [0, n]
        same(got["final_vector_states"], before["vector_states"][:3], "final entries")
        same(got["obs_vector_states"][0], w.snapshot()["vector_states"], "slot 0 holds the new episode's")
        assert got["final_idx"][0].tolist() == list(range(n))
        adv, ret = w.rollout_gae(values, None, 0.9, 0.9)  # no transition yet: nothing is written
        assert not host({"a": adv})["a"].any()
    finally:
        for x in (w, no_laser, shallow):
            x.close()
