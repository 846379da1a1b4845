"""The running normalisation on the device (imgenv_normalise_enable, csrc/normalise.h).  Every sum of the kernels is taken in a fixed
order that tests/normalise_model.py mirrors, and everything else is IEEE float64 arithmetic without contraction, so every comparison
is exact: bit patterns, no tolerance.  The model is fed from imgenv_out's raw arrays: what a step showed before the device-side reset
behind it overwrote the finished envs' rows comes from the final observations of the same handle (csrc/final_obs.h).

Three shapes reach every path: 1 env x 1 robot (one row, a reset without a list), 3 envs x 5 robots (listed reset chains, frozen
robots of a multi-robot env) and one tile of k_norm_part + 1 envs of one robot (two tiles merge, a grid of more than one workgroup).
Each runs 12 steps with imgenv_step_autoreset_device and time_max 5, so the device resets envs, plus one reset by the caller in
mid-episode, in three rollout windows of 4 steps, with a state stack of depth 3, final observations and the rollout ring."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import normalise_model as nm
import rollout_model
from test_gpu_final_obs import fixed_actions, host, narrow_cfg, same

pytestmark = pytest.mark.gpu
PAR = dict(obs=True, reward=True, gamma=0.97, clip_obs=2.5, clip_reward=1.5, eps=1e-6)  # (clips that bite)
D, K, T, STEPS = 5, 3, 4, 12
SHAPES = {"1x1": (1, 1), "3x5": (3, 5), "tile+1": (nm.tile_rows(D + 1) + 1, 1)}
LIVE = ("norm_vector_states", "norm_state_stack", "norm_rewards")
# imgenv_step_launches after each of 7 imgenv_step_autoreset_device calls on 3 envs x 5 robots x 2 pedestrians with a state stack and
# nothing else enabled, counted on the commit before this feature (the step's chain and the reset chain behind it)
PLAIN_LAUNCHES = [16] * 7


def make(E, R, normalise=PAR, **kw):
    from img_env_amd.vec_env import VecImageEnv
    cfg = narrow_cfg(R, 2, state_batch=K, image_batch=0, laser_batch=-1)
    return VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, stack=True, normalise=normalise, **kw)


def lib_state(vec):
    """host copies of the statistics and returns of the words in turn, and of the three normalised arrays"""
    w = vec.world
    sw, rw, _ = w.normalise_words()
    n = host(w.normalise)
    return {"stats": n["stats"][sw], "returns": n["returns"][rw], **{k: n[k] for k in LIVE}}


def model_state(m):
    s = m.stats()
    return {"stats": np.concatenate([[s["obs_count"], s["ret_count"], s["ret_mean"], s["ret_var"]], s["obs_mean"], s["obs_var"]]),
            "returns": s["returns"], "norm_vector_states": m.norm_vector_states, "norm_state_stack": m.norm_state_stack.reshape(m.R, -1),
            "norm_rewards": m.norm_rewards}


def raw(vec):
    """the raw arrays a chain has left, the final observations beside them"""
    snap = vec.world.snapshot()
    snap["stack"] = host({"s": vec.world.stack["vector_states"]})["s"]
    snap["final"] = host(vec.world.final_obs)
    return snap


@functools.lru_cache(maxsize=None)
def record(shape, run=0):
    """what the handle showed after every call, and the ring at the end of every window (``run``: a second, independent recording)"""
    import torch
    E, R = SHAPES[shape]
    vec = make(E, R, final_obs=True, rollout=T, rollout_final=2 * (T + 1) * E * R)
    try:
        acts = fixed_actions(STEPS, E * R)
        rec = {"calls": [], "rings": [], "fields": sorted(vec.world.rollout), "final_fields": sorted(vec.world.final_obs)}
        vec.reset()
        rec["calls"].append(("reset", raw(vec), lib_state(vec), None))
        for t in range(STEPS):
            if t and t % T == 0:
                vec.rollout_begin()
            state, rew, done, info = vec.step(torch.as_tensor(acts[t], device="cuda"))
            assert rew.data_ptr() == vec.world.normalise["norm_rewards"].data_ptr() and info["raw_rewards"].data_ptr() == vec.world.out["step_rewards"].data_ptr()
            assert state.vector_states.data_ptr() == vec.world.normalise["norm_state_stack"].data_ptr()
            assert info["raw_vector_states"].data_ptr() == vec.world.out["vector_states"].data_ptr()
            rec["calls"].append(("step", raw(vec), lib_state(vec), acts[t]))
            if t == 2:  # a caller's reset in mid-episode: env 1 (the only env of a handle of one: a chain without a list)
                env = min(1, E - 1)
                vec.reset_envs([env])
                rec["calls"].append(("caller_reset", raw(vec), lib_state(vec), env))
            if t % T == T - 1:
                r = vec.rollout()
                n, resets = r.pop("n"), r.pop("resets")
                r = host(r)
                r.update(n=n, resets=resets)
                g = torch.Generator(device="cpu").manual_seed(t)
                values, fv = torch.randn((T + 1, E * R), generator=g).cuda(), torch.randn(r["final_slot"].shape[0], generator=g).cuda()
                adv, ret = vec.rollout_advantages(values, fv, 0.99, 0.95)
                r.update(host({"values": values, "final_values": fv, "adv": adv, "ret": ret}))
                rec["rings"].append(r)
    finally:
        vec.close()
    return rec


def replay(shape):
    """the model over the recorded raw arrays: yields (call, what the library showed, the model) after every call"""
    E, R = SHAPES[shape]
    n = E * R
    m = nm.Normalise(n, D, K, **PAR)
    for kind, snap, lib, arg in record(shape)["calls"]:
        vs, stack = snap["vector_states"], snap["stack"].reshape(n, K, D)
        if kind == "reset":
            m.reset(np.arange(n), vs, stack)
        elif kind == "caller_reset":
            m.reset(np.arange(arg * R, (arg + 1) * R), vs, stack)
        else:
            down = snap["step_all_down"].astype(bool)
            fin = snap["final"]
            vs_step = np.where(down[:, None], fin["vector_states"], vs)
            stack_step = np.where(down[:, None, None], fin["stack_vector_states"].reshape(n, K, D), stack)
            m.step(vs_step, snap["step_rewards"], snap["step_is_clean"], snap["step_dones"], stack_step)
            if down.any():  # the device-side reset chain behind the step: the finished envs, ascending
                m.reset(np.flatnonzero(down), vs, stack)
        yield (kind, snap, lib, copy.deepcopy(model_state(m)))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_statistics_and_outputs_equal_the_model_after_every_chain(shape):
    resets = frozen = clipped = 0
    for q, (kind, snap, lib, want) in enumerate(replay(shape)):
        for name in want:
            same(lib[name], want[name], "%s, call %d (%s): %s" % (shape, q, kind, name))
        if kind == "step":
            resets += int(snap["step_all_down"].any())
            frozen += int((snap["step_is_clean"] == 0).sum())
            clipped += int((np.abs(lib["norm_vector_states"]) == np.float32(PAR["clip_obs"])).sum() + (np.abs(lib["norm_rewards"]) == PAR["clip_reward"]).sum())
    print("%s: %d calls with a device-side reset, %d frozen rows, %d clipped values" % (shape, resets, frozen, clipped))
    assert resets >= 1  # time_max 5 < 12 steps: the device reset envs (an env the caller reset at step 2 times out once, at step 7)
    assert lib["stats"][0] > STEPS / 2 and lib["stats"][1] > STEPS / 2  # the counts ran
    if shape != "1x1":
        assert frozen > 0 or SHAPES[shape][1] == 1  # (robots that finished before their env did)
        assert clipped > 0


@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_second_run_gives_identical_bits(shape):
    a, b = record(shape), record(shape, 1)
    assert a is not b and len(a["calls"]) == len(b["calls"])
    for (_, _, la, _), (_, _, lb, _) in zip(a["calls"], b["calls"]):
        for name in la:
            assert la[name].tobytes() == lb[name].tobytes(), name


@pytest.mark.parametrize("shape", list(SHAPES))
def test_ring_and_final_list_hold_the_normalised_arrays(shape):
    """rollout=4 with IMGENV_ROLLOUT_NORM_STATES | _NORM_REWARDS (VecImageEnv switches them on): every slot's state rows are the
    normalised arrays seen at that step, the ring's rewards norm_rewards, the final-list rows what was shown before the reset, the
    advantages the numpy GAE model's on those rewards; and with IMGENV_FINAL_NORM_STATES the captured rows are the pre-reset ones"""
    E, R = SHAPES[shape]
    rec = record(shape)
    assert {"obs_norm_vector_states", "obs_norm_state_stack", "final_norm_vector_states", "final_norm_state_stack"} <= set(rec["fields"])
    assert "obs_vector_states" not in rec["fields"] and {"norm_vector_states", "norm_state_stack"} <= set(rec["final_fields"])
    calls, at, moved = rec["calls"], 1, 0  # (calls[0] is the reset the first window begins behind)
    for w, r in enumerate(rec["rings"]):
        assert r["n"] == T
        for f in ("norm_vector_states", "norm_state_stack"):  # slot 0: what the handle showed when the window began
            same(r["obs_" + f][0], calls[at - 1][2][f], "window %d: slot 0 %s" % (w, f))
        slot = 0
        while at < len(calls):
            kind, snap, lib, arg = calls[at]
            if kind == "step":
                if slot == T:
                    break
                same(r["rewards"][slot], lib["norm_rewards"].astype(np.float32), "window %d: rewards %d" % (w, slot))
                # the envs the device reset behind this step: the final list and the final observations of the same handle hold the
                # normalised rows of before the reset (but for rows the caller reset once more at the same slot: the later entry stays)
                down = snap["step_all_down"].astype(bool)
                if at + 1 < len(calls) and calls[at + 1][0] == "caller_reset":
                    down[calls[at + 1][3] * R:(calls[at + 1][3] + 1) * R] = False
                idx = r["final_idx"][slot + 1]
                assert (idx[down] >= 0).all()
                for row in np.flatnonzero(down):
                    for f in ("norm_vector_states", "norm_state_stack"):
                        same(r["final_" + f][idx[row]], snap["final"][f][row], "window %d, slot %d, row %d: final %s" % (w, slot + 1, row, f))
                    moved += 1
                slot += 1
            else:  # the caller's reset: slot `slot` now shows the new episode, the final list what the step before showed
                rows = np.arange(arg * R, (arg + 1) * R)
                idx = r["final_idx"][slot]
                assert (idx[rows] >= 0).all()
                for row in rows:
                    for f in ("norm_vector_states", "norm_state_stack"):
                        same(r["final_" + f][idx[row]], calls[at - 1][2][f][row], "window %d: caller's reset, row %d: %s" % (w, row, f))
                        same(snap["final"][f][row], calls[at - 1][2][f][row], "final_obs at the caller's reset, row %d: %s" % (row, f))
                    moved += 1
            if not (kind == "step" and at + 1 < len(calls) and calls[at + 1][0] == "caller_reset"):  # (that reset rewrites the slot)
                for f in ("norm_vector_states", "norm_state_stack"):
                    same(r["obs_" + f][slot], lib[f], "window %d: slot %d %s" % (w, slot, f))
            at += 1
        adv, ret = rollout_model.gae(r, r["values"], r["final_values"], 0.99, 0.95, r["final_slot"].shape[0])
        same(r["adv"], adv, "window %d: adv" % w)
        same(r["ret"], ret, "window %d: ret" % w)
    assert moved >= 2 * R


def test_training_off_freezes_the_statistics_and_stats_move_to_a_fresh_handle():
    """evaluation: the statistics' and returns' bits stay while the outputs still follow the raw arrays; stats_get -> a fresh handle
    -> stats_set reproduces the first handle's outputs from then on"""
    import torch
    E, R = SHAPES["3x5"]
    acts = fixed_actions(8, E * R)
    a = make(E, R)
    try:
        a.reset()
        for t in range(4):
            a.step(torch.as_tensor(acts[t], device="cuda"))
        stats = a.normalise_stats()
        before = lib_state(a)
        same(stats["obs_mean"], before["stats"][4:4 + D], "stats_get: obs_mean")
        same(stats["returns"], before["returns"], "stats_get: returns")
        assert (stats["obs_count"], stats["ret_count"]) == (before["stats"][0], before["stats"][1]) and stats["obs_count"] > 4
        # a fresh handle of the same shape, the same episode history (the raw arrays do not depend on the feature): other statistics
        fresh = make(E, R)
        try:
            fresh.world.normalise_training(False)
            fresh.reset()
            for t in range(4):
                fresh.step(torch.as_tensor(acts[t], device="cuda"))
            assert lib_state(fresh)["stats"][0] == 1e-4  # (evaluation from the start: nothing moved)
            fresh.load_normalise_stats(stats)
            a.normalise_training(False)
            m = nm.Normalise(E * R, D, K, **PAR)
            m.load(stats)
            m.training = False
            for t in range(4, 8):
                a.step(torch.as_tensor(acts[t], device="cuda"))
                fresh.step(torch.as_tensor(acts[t], device="cuda"))
                la, lf, snap = lib_state(a), lib_state(fresh), raw_no_final(a)
                same(la["stats"], before["stats"], "training off, step %d: stats" % t)
                same(la["returns"], before["returns"], "training off, step %d: returns" % t)
                for name in LIVE + ("stats",):
                    same(lf[name], la[name], "fresh handle, step %d: %s" % (t, name))
                # the outputs follow the raw arrays: the rows no reset touched behind the step are the model's apply of this step
                live = ~snap["step_all_down"].astype(bool)
                m.step(snap["vector_states"], snap["step_rewards"], snap["step_is_clean"], snap["step_dones"], snap["stack"].reshape(E * R, K, D))
                same(la["norm_vector_states"][live], m.norm_vector_states[live], "training off, step %d: norm_vector_states" % t)
                same(la["norm_rewards"], m.norm_rewards, "training off, step %d: norm_rewards" % t)
            # training on again: the statistics move on from where they stood
            a.normalise_training(True)
            a.reset_envs([0])
            assert lib_state(a)["stats"][0] == before["stats"][0] + R
        finally:
            fresh.close()
    finally:
        a.close()


def raw_no_final(vec):
    snap = vec.world.snapshot()
    snap["stack"] = host({"s": vec.world.stack["vector_states"]})["s"]
    return snap


def test_refusals_and_launch_counts():
    """every IMGENV_EINVAL of the feature, and the launches: a handle without the feature launches what it always did and shows the
    same bytes; with it, imgenv_step_launches after imgenv_step_autoreset_device -- the step's chain and the reset chain behind it
    -- is 4 more in training (k_norm_part + k_norm_apply twice) and 2 more in evaluation"""
    import torch
    from img_env_amd import _cabi
    E, R = SHAPES["3x5"]
    plain, on = make(E, R, normalise=None), make(E, R)
    try:
        w, lib = plain.world, plain.world.lib
        for bits in (_cabi.ROLLOUT_NORM_STATES | 2, _cabi.ROLLOUT_NORM_REWARDS | 2):  # before imgenv_normalise_enable
            assert lib.imgenv_rollout_enable(w.h, C.byref(_cabi.make_rollout_cfg(4, 8, bits)), None) == _cabi.EINVAL
            assert b"imgenv_normalise_enable" in lib.imgenv_last_error()
        assert lib.imgenv_final_obs_enable(w.h, C.byref(_cabi.make_final_obs_cfg(_cabi.FINAL_NORM_STATES | 1)), None) == _cabi.EINVAL
        with pytest.raises(ValueError, match="imgenv_normalise_enable"):
            w.enable_rollout(4, 8, ["vector_states", "norm_rewards"])
        with pytest.raises(RuntimeError):
            w.normalise_stats()
        no = _cabi.NormaliseOut()
        assert lib.imgenv_normalise_outputs(w.h, C.byref(no)) == _cabi.ESTATE and lib.imgenv_normalise_training(w.h, 0, None) == _cabi.ESTATE
        for bad in (dict(clip_obs=0.0), dict(clip_obs=float("inf")), dict(clip_reward=-1.0), dict(clip_reward=float("nan")), dict(eps=0.0),
                    dict(eps=float("nan")), dict(gamma=-0.01), dict(gamma=1.01), dict(gamma=float("nan")), dict(obs=False, reward=False)):
            with pytest.raises(ValueError):
                w.enable_normalise(**dict(PAR, **bad))
        c = _cabi.make_normalise_cfg()
        c.struct_size -= 8
        assert lib.imgenv_normalise_enable(w.h, C.byref(c), None) == _cabi.EINVAL
        assert lib.imgenv_normalise_enable(None, C.byref(_cabi.make_normalise_cfg()), None) == _cabi.EINVAL
        with pytest.raises(ValueError, match="already"):  # enabling twice
            on.world.enable_normalise(**PAR)
        with pytest.raises(ValueError):
            on.world.enable_rollout(4, 8, ["norm_rewards"])  # (selects no field)
        stats = on.normalise_stats()
        for bad in (dict(obs_count=0.0), dict(ret_var=-1.0), dict(ret_mean=float("nan")), dict(obs_var=np.full(D, -1.0)), dict(obs_mean=np.zeros(D + 1))):
            with pytest.raises(ValueError):
                on.load_normalise_stats(dict(stats, **bad))
        rew_only = make(E, R, normalise=dict(PAR, obs=False))
        try:
            for call in (lambda: rew_only.world.enable_rollout(4, 8, ["vector_states", "norm_states"]), lambda: rew_only.world.enable_final_obs(["norm_states"])):
                with pytest.raises(ValueError):
                    call()
            assert "norm_vector_states" not in rew_only.world.normalise and rew_only.reset().vector_states.data_ptr() == rew_only.world.stack["vector_states"].data_ptr()
        finally:
            rew_only.close()
        # the launches and the raw bytes
        acts = fixed_actions(7, E * R)
        plain.reset()
        on.reset()
        more, plain_counts = set(), []
        for t in range(7):
            if t == 4:
                on.normalise_training(False)
            plain.step(torch.as_tensor(acts[t], device="cuda"))
            on.step(torch.as_tensor(acts[t], device="cuda"))
            more.add((t >= 4, on.world.launches() - plain.world.launches()))
            plain_counts.append(plain.world.launches())
            sp, so = plain.world.snapshot(), on.world.snapshot()
            for f in sp:
                assert sp[f].tobytes() == so[f].tobytes(), (t, f)
        assert more == {(False, 4), (True, 2)}
        print("imgenv_step_launches of the handle without the feature:", plain_counts)
        assert plain_counts == PLAIN_LAUNCHES  # what the commit before this feature launched for the same calls
    finally:
        plain.close()
        on.close()


def test_a_robot_shard_keeps_its_own_statistics_and_refuses_the_listed_chain():
    """a robot-sharded handle (rows 0 .. 1 of a 5-robot world) may enable the feature: its statistics are over its two local rows.
    The one listed chain such a handle could run, imgenv_step_autoreset_device, is IMGENV_EINVAL before anything is queued, and
    every statistic, return and output keeps its bits"""
    import torch
    from img_env_amd import _cabi, config, spawn
    from img_env_amd.world import World
    cfg = narrow_cfg(5, 2)
    params, grid = config.params_from_cfg(cfg), config.load_map(cfg)
    layout = spawn.EnvPos(cfg, seed=9).reset(max(grid.shape[-2:]) * float(cfg["global_map"]["resolution"]))
    w = World(dict(params, robot_begin=0, robot_end=2), grid)
    try:
        assert w.n_local == 2
        w.enable_normalise(**PAR)
        w.reset(layout)
        sw, rw, _ = w.normalise_words()
        before = host(w.normalise)
        snap = w.snapshot()
        m = nm.Normalise(2, D, 0, **PAR)
        m.reset(np.arange(2), snap["vector_states"])
        want = model_state(m)
        same(before["stats"][sw], want["stats"], "shard: the statistics of the two local rows")
        same(before["norm_vector_states"], want["norm_vector_states"], "shard: norm_vector_states")
        assert before["stats"][sw][0] == 1e-4 + 2
        sc = spawn.make_spawn_cfg(cfg)
        acts = torch.zeros((2, 3), dtype=torch.float32, device="cuda")
        rc = w.lib.imgenv_step_autoreset_device(w.h, C.c_void_p(acts.data_ptr()), C.byref(sc[0]), C.c_uint64(1), None)
        assert rc == _cabi.EINVAL and b"needs all robots of every world" in w.lib.imgenv_last_error()
        assert w.normalise_words()[:2] == (sw, rw)
        after = host(w.normalise)
        for name in before:
            assert before[name].tobytes() == after[name].tobytes(), name
    finally:
        w.close()


def test_minibatches_carry_the_normalised_fields():
    """VecImageEnv(normalise=..., rollout=T, minibatch=B): every gathered row of mb_norm_vector_states / mb_norm_state_stack is the
    ring row that mb_index names, zeros behind the valid list; two buffers, a batch that does not divide the valid count"""
    import torch
    E, R = SHAPES["3x5"]
    B = 7
    vec = make(E, R, rollout=T, rollout_final=64, minibatch=B, minibatch_buffers=2)
    try:
        assert {"mb_norm_vector_states", "mb_norm_state_stack"} <= set(vec.world.minibatch)
        assert vec.world.minibatch["mb_norm_state_stack"].shape == (2, B, K * D)
        assert "mb_vector_states" not in vec.world.minibatch
        acts = fixed_actions(T, E * R)
        vec.reset()
        for t in range(T):
            vec.step(torch.as_tensor(acts[t], device="cuda"))
        ring = host({k: v for k, v in vec.world.rollout.items() if k.startswith("obs_norm") or k == "is_clean"})
        adv = torch.arange(T * E * R, dtype=torch.float32, device="cuda").view(T, E * R)
        seen, weightless = [], 0
        for mb in vec.rollout_minibatches({"adv": adv}, seed=5):
            got = host({k: mb[k] for k in ("mb_norm_vector_states", "mb_norm_state_stack", "mb_index", "mb_weight", "adv")})
            for i, k in enumerate(got["mb_index"]):
                for f in ("norm_vector_states", "norm_state_stack"):
                    rows = ring["obs_" + f].reshape((T + 1) * E * R, -1)
                    same(got["mb_" + f][i], rows[k] if k >= 0 else np.zeros_like(rows[0]), "slot %d (k = %d): %s" % (i, k, f))
                assert got["adv"][i] == (k if k >= 0 else 0)
                weightless += int(k < 0)
            seen += [int(k) for k in got["mb_index"] if k >= 0]
        assert sorted(seen) == np.flatnonzero(ring["is_clean"].reshape(-1)).tolist() and weightless > 0
        assert np.abs(ring["obs_norm_vector_states"][1:T + 1]).max() > 0
        from img_env_amd import _cabi  # IMGENV_ROLLOUT_NORM_REWARDS names no field of a minibatch
        bad = _cabi.make_minibatch_cfg(B, 2, _cabi.ROLLOUT_NORM_REWARDS | _cabi.ROLLOUT_NORM_STATES)
        assert vec.world.lib.imgenv_rollout_minibatch_enable(vec.world.h, C.byref(bad), None) == _cabi.EINVAL
        assert b"fields" in vec.world.lib.imgenv_last_error()
    finally:
        vec.close()
