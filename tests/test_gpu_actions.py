"""Action decoding (imgenv_actions_*, csrc/actions.h) and observation post-processing (imgenv_obs_post_*, csrc/obs_post.h) on the
device against the numpy models of tests/action_model.py, which tests/test_action_model.py holds to the reference's own
recordings and lines.  Both kernels only compare, convert, select, subtract and divide without contraction, so every array is
compared bit for bit, after every call."""
import copy
import ctypes as C

import numpy as np
import pytest

from action_model import CLIP, TABLE, ActionModel, close_to_human, decode, ped_norm, table_rows
from episode_model import EpisodeModel
from scenarios import random_actions, small_world
from stack_model import bits
from test_gpu_episodes import device_arrays, env_rows, episode_cfg, same_arrays, step_inputs

pytestmark = pytest.mark.gpu
TABLE8 = [[0.0, -0.9], [0.0, 0.3], [0.2, -0.6], [0.2, 0.0], [0.4, 0.6], [0.6, -0.3], [0.6, 0.0, 1], [0.6, 0.9]]  # the fixtures' table
CLIP3 = [[0, 0.6], [-0.9, 0.9], [-0.6, 0.6]]  # 10obs_5ped_baseline.yaml
WRAPPERS = ["VelActionWrapper", "TimeLimitWrapper", "SensorsPaperRewardWrapper", "InfoLogWrapper", "MultiRobotCleanWrapper",
            "StatePedVectorWrapper"]


def same(got, want, where):
    g, w = np.asarray(got), np.asarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (where, g.dtype, w.dtype, g.shape, w.shape)
    eq = (g == w) if g.dtype.itemsize == 1 else (bits(g) == bits(w))  # (uint8 flags have no bit pattern to hide behind)
    if not eq.all():
        at = np.argwhere(~eq)[0]
        raise AssertionError("%s differs at %s: got %r, want %r (%d of %d)" % (where, at.tolist(), g[tuple(at)], w[tuple(at)],
                                                                                 (~eq).sum(), eq.size))


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def raw_policy(vector_states, discrete, scale=1.6):
    """turn towards the goal and drive (vector_states[:, :2] is the goal in the robot's frame), as the raw output of a policy:
    the index of the nearest row of TABLE8, or (v, w) stretched so that part of it lies outside the clip range"""
    vs = np.asarray(vector_states, np.float64)
    ang = np.arctan2(vs[:, 1], vs[:, 0])
    v = np.where(np.abs(ang) < 0.7, 0.6, 0.1)
    w = np.clip(2.0 * ang, -0.9, 0.9)
    if discrete:
        t = table_rows(TABLE8).astype(np.float64)
        return np.argmin((t[None, :, 0] - v[:, None]) ** 2 + (t[None, :, 1] - w[:, None]) ** 2, axis=1).astype(np.int64)
    return np.stack([v * scale - 0.2, w * scale], 1)


# ---- 1. the decode alone ----
@pytest.mark.parametrize("R", [3, 70, 257])
def test_decode_every_dtype_mode_and_width_with_bad_rows_at_the_edges(R):
    """pedestrian-free handles below a wavefront, across one and across a block; int32 / int64 indices and float32 / float64 rows,
    TABLE and CLIP mode, 2 and 3 columns; bad rows (index -1 / n_table / far out, NaN, +-inf) in the first lane, the first
    wavefront's last lane, the last (partial) wavefront's first lane and the last row -- n_bad exact after every decode; then one
    step on the decoded rows: nothing non-finite reaches it"""
    import torch
    from img_env_amd.world import World
    grid, params, layout = small_world(R, 0, seed=11, grid_size=480, clearance=0.7)
    bad_rows = sorted({0, min(63, R - 1), (R - 1) // 64 * 64, R - 1})
    rng = np.random.default_rng(R)
    for mode, n_cols in ((TABLE, 2), (TABLE, 3), (CLIP, 2), (CLIP, 3)):
        w = World(params, grid)
        try:
            out = w.enable_actions(discrete_actions=TABLE8, act_dim=n_cols) if mode == TABLE else \
                w.enable_actions(continuous_actions=CLIP3, act_dim=n_cols)
            assert out["actions"].shape == (R, 3) and out["speeds"].shape == (R, 2) and out["n_bad"].shape == (1,)
            w.reset(layout)
            m = ActionModel(R, mode, table=TABLE8 if mode == TABLE else None, clip=CLIP3 if mode == CLIP else None, n_cols=n_cols)
            raws = []
            if mode == TABLE:
                for dt, far in ((np.int32, 2 ** 31 - 1), (np.int64, -2 ** 40)):
                    idx = rng.integers(0, len(TABLE8), R).astype(dt)
                    idx[bad_rows] = [(-1, len(TABLE8), far, len(TABLE8))[q % 4] for q in range(len(bad_rows))]
                    raws.append(idx)
            for dt in (np.float32, np.float64):
                x = rng.uniform(-1.5, 1.5, (R, n_cols)).astype(dt)
                x[bad_rows, rng.integers(0, n_cols, len(bad_rows))] = [(np.nan, np.inf, -np.inf, np.nan)[q % 4] for q in range(len(bad_rows))]
                raws.append(x)
            for k, raw in enumerate(raws):
                # (numpy and torch inputs alike)
                got = w.decode_actions(torch.as_tensor(raw, device="cuda") if k % 2 else raw)
                assert got is out["actions"]
                want = m.decode(raw)
                where = "R %d mode %d cols %d %s" % (R, mode, n_cols, raw.dtype)
                same(host(out["actions"]), want, where + " actions")
                same(host(out["speeds"]), m.speeds, where + " speeds")
                assert int(host(out["n_bad"])[0]) == m.n_bad == (k + 1) * len(bad_rows), where
                assert (want[bad_rows] == 0).all() and (m.speeds == want[:, :2]).all()
            w.step(out["actions"])
            snap = w.snapshot()
            for f in ("robot_pose", "vector_states", "lasers", "rewards", "step_ds"):
                assert np.isfinite(snap[f]).all(), (where, f)
            same(host(out["actions"]), m.actions, where + " after the step")
        finally:
            w.close()


# ---- 2. VecImageEnv(wrappers=True) in its three reset modes ----
@pytest.mark.parametrize("discrete", [True, False], ids=["discrete", "continuous"])
@pytest.mark.parametrize("mode", ["host_reset", "native_spawn", "device_reset"])
def test_vec_env_decodes_what_the_policy_emits(mode, discrete):
    """16 envs of 3 robots and 2 pedestrians, time limit 10, 30 steps of a goal-seeking policy given as raw output: indices of the
    nearest table row, or float rows partly outside the clip range.  ``actions`` and ``speeds`` equal the model after every step;
    the model takes that step's dones and the envs that restarted.  Masked rows, restarts and (continuous) clipped values must
    occur.  The episode statistics kept beside it equal tests/episode_model.py fed the DECODED actions."""
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, steps = 16, 3, 2, 30
    cfg = episode_cfg(R, P, discrete_action=discrete, discrete_actions=TABLE8)
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=mode != "host_reset", device_reset=mode == "device_reset",
                      episode_stats=True, wrappers=True)
    try:
        w = vec.world
        m = ActionModel(E * R, TABLE if discrete else CLIP, table=TABLE8 if discrete else None, clip=cfg["continuous_actions"])
        ep = EpisodeModel(E * R, cfg["control_hz"])
        state = vec.reset()
        ep.reset(np.ones(E * R, bool), np.zeros(E * R, np.int32))
        restarts = clipped = 0
        for s in range(steps):
            raw = raw_policy(host(state.vector_states), discrete)
            if mode == "native_spawn":  # (device tensors and host arrays, float32 and float64)
                raw = torch.as_tensor(raw if discrete else raw.astype(np.float32), device="cuda")
            state, rew, done, info = vec.step(raw)
            raw = host(raw) if isinstance(raw, torch.Tensor) else raw
            want = m.decode(raw)
            if not discrete:
                clipped += int((want[:, :2] != raw.astype(np.float32)).sum())
            same(host(w.action_outputs["actions"]), want, "%s step %d actions" % (mode, s))
            same(host(info["speeds"]), m.speeds, "%s step %d speeds" % (mode, s))
            assert info["speeds"] is w.action_outputs["speeds"]
            got = step_inputs(w)
            assert np.array_equal(got["step_is_clean"].astype(bool), m.is_clean), s  # the mask IS the step's is_clean
            m.step_done(host(done))
            all_down = host(info["all_down"]).astype(bool)
            rows = all_down if mode == "device_reset" else env_rows(info["reset_envs"], E, R)
            assert np.array_equal(rows, all_down), s
            m.reset(rows)
            restarts += int(rows.sum()) // R
            ep.step(want, got["step_is_clean"], got["step_rewards"])
            ep.reset(rows, got["step_dones_info"])
            same_arrays(device_arrays(w), ep.arrays(), "%s step %d statistics" % (mode, s))
            same(host(info["bool_get_close_to_human"]), close_to_human(host(w.out["ped_min_dists"])), "close %d" % s)
        print("%s %s: masked rows %d, restarts %d, clipped %d, bad %d" % (mode, "discrete" if discrete else "continuous",
                                                                          m.masked_rows, restarts, clipped, m.n_bad))
        assert m.masked_rows > 0 and restarts > 0 and (discrete or clipped > 0)
        assert int(host(w.action_outputs["n_bad"])[0]) == 0
        assert ep.episodes.sum() > 0
    finally:
        vec.close()


# ---- 3. the normalised pedestrian vectors and close_to_human ----
def check_post(vec, where):
    w = vec.world
    raw = host(w.out["ped_vector_states"])
    same(host(w.obs_post["ped_vector_norm"]), ped_norm(raw, vec.cfg["max_ped"]), where + " ped_vector_norm")
    close = host(w.obs_post["close_to_human"])
    same(close, close_to_human(host(w.out["ped_min_dists"])), where + " close_to_human")
    return raw, close


@pytest.mark.parametrize("stack", [False, True], ids=["frames", "stacks"])
def test_normalised_ped_vectors_and_close_to_human_follow_every_chain(stack):
    """16 envs of 3 robots and 2 pedestrians with max_ped 10 (eight pedestrians of padding per row): after the reset, after every
    step (device-side resets among them) and after a caller's reset of 2 of the 16 envs, whose other rows stay as they were"""
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P = 16, 3, 2
    cfg = episode_cfg(R, P, max_ped=10, wrappers=WRAPPERS, discrete_action=True, discrete_actions=TABLE8,
                      **(dict(image_batch=2, state_batch=3, laser_batch=2) if stack else {}))
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, stack=stack, wrappers=True)
    try:
        w = vec.world
        assert w.obs_post["ped_vector_norm"].shape == (E * R, 71) and w.obs_post["close_to_human"].shape == (E * R,)
        state = vec.reset()
        assert state.ped_vector_states is w.obs_post["ped_vector_norm"]
        raw, close = check_post(vec, "reset")
        assert (raw[:, 0] == P).all() and (raw[:, 1 + 7 * P:] == 0).all()
        seen = set(close.tolist())
        changed = 0
        for s in range(24):
            state, _, _, info = vec.step(raw_policy(host(state.vector_states), True))
            raw, close = check_post(vec, "step %d" % s)
            assert info["bool_get_close_to_human"] is w.obs_post["close_to_human"]
            seen |= set(close.tolist())
            changed += int((host(w.obs_post["ped_vector_norm"]) != raw).any(axis=1).sum())
        assert seen == {0, 1} and changed > 0, (seen, changed)
        before = host(w.obs_post["ped_vector_norm"]).copy(), host(w.obs_post["close_to_human"]).copy()
        vec.reset_envs([3, 7])
        check_post(vec, "reset of 2 envs")
        others = ~env_rows([3, 7], E, R)
        same(host(w.obs_post["ped_vector_norm"])[others], before[0][others], "rows of the other envs")
        same(host(w.obs_post["close_to_human"])[others], before[1][others], "rows of the other envs")
        assert (host(w.obs_post["ped_vector_norm"])[~others] != before[0][~others]).any()
        vec.step(raw_policy(host(w.out["vector_states"]), True))
        check_post(vec, "step after it")
    finally:
        vec.close()


def test_a_handle_without_pedestrians_copies_its_rows():
    """count 0: nothing to normalise, ped_vector_norm is the raw row; close_to_human is not offered without pedestrians"""
    from img_env_amd.world import World
    grid, params, layout = small_world(5, 0, seed=4)
    w = World(params, grid)
    try:
        with pytest.raises(ValueError, match="pedestrians"):
            w.enable_obs_post(ped_norm=True, close=True)
        post = w.enable_obs_post()
        assert set(post) == {"ped_vector_norm"} and w.enable_obs_post() is post
        with pytest.raises(ValueError, match="another cfg"):
            w.enable_obs_post(std=(6.0, 6.0, 0.6, 0.9, 0.5, 0.5, 5.0))
        w.reset(layout)
        w.step(random_actions(np.random.default_rng(0), 5))
        raw = host(w.out["ped_vector_states"])
        assert (raw[:, 0] == 0).all()
        same(host(post["ped_vector_norm"]), raw, "count 0")
        same(host(post["ped_vector_norm"]), ped_norm(raw, (raw.shape[1] - 1) // 7), "count 0, the model")
    finally:
        w.close()


# ---- 4. disabled is invisible ----
@pytest.mark.parametrize("flags", [4, 512], ids=["stamped_layer", "counting_layer"])
@pytest.mark.parametrize("device_reset", [False, True], ids=["native_spawn", "device_reset"])
def test_a_handle_that_enables_nothing_computes_and_launches_as_before(device_reset, flags):
    """same cfg and seed on a handle that never touches the new calls, fed the decoded rows, and on one that decodes indices and
    post-processes: every byte of every imgenv_out array equal on every step; imgenv_step_launches differs by one per chain
    (k_obs_post) plus one per decode.  After imgenv_step_autoreset_device the count covers the step's and the reset chain: 3.
    After imgenv_step_autoreset it covers the last chain alone -- the step's with its decode, 2, or the reset chain's, 1 -- and
    both kinds must occur."""
    from img_env_amd.vec_env import VecImageEnv
    E, R, P = 16, 3, 2
    cfg = episode_cfg(R, P, max_ped=4, wrappers=WRAPPERS, discrete_action=True, discrete_actions=TABLE8, flags=flags)
    plain = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=True, device_reset=device_reset)
    full = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=True, device_reset=device_reset, wrappers=True)
    try:
        assert plain.world.action_outputs is None and plain.world.obs_post is None
        assert full.world.layer_mode()["layer"] == plain.world.layer_mode()["layer"] == {4: "stamped", 512: "counting"}[flags]
        for v in (plain, full):
            v.reset()
        assert full.world.launches() == plain.world.launches() + 1
        extra, with_reset = set(), set()
        for s in range(24):
            raw = raw_policy(host(plain.world.out["vector_states"]), True)
            info_f = full.step(raw)[3]
            info_p = plain.step(full.world.action_outputs["actions"].clone())[3]
            assert "speeds" not in info_p and "bool_get_close_to_human" not in info_p and "speeds" in info_f
            if not device_reset:
                assert info_p["reset_envs"] == info_f["reset_envs"], s
                with_reset.add(len(info_p["reset_envs"]) > 0)
            sa, sb = plain.world.snapshot(), full.world.snapshot()
            assert set(sa) == set(sb)
            for f in sa:
                assert sa[f].tobytes() == sb[f].tobytes(), (s, f)
            extra.add(full.world.launches() - plain.world.launches())
        assert extra == ({3} if device_reset else {1, 2}), extra
        assert device_reset or with_reset == {False, True}, with_reset
    finally:
        plain.close()
        full.close()


# ---- 5. stream order ----
def test_decode_and_step_are_ordered_on_the_stream_without_any_synchronisation():
    """20 rounds of: a torch op on the stream writes the raw actions, decode, imgenv_step_autoreset_device -- queued back to back
    behind a stream kept busy by large matrix products, clones of what each round left taken on the same stream; against a twin
    that synchronises after every call"""
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, rounds = 32, 3, 2, 20
    cfg = episode_cfg(R, P, time_max=5, max_ped=4, wrappers=WRAPPERS, discrete_action=True, discrete_actions=TABLE8)
    run = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, wrappers=True)
    twin = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, wrappers=True)
    try:
        g = torch.Generator(device="cuda").manual_seed(3)
        all_raw = torch.randint(0, len(TABLE8), (rounds, E * R), generator=g, device="cuda")
        names = ("actions", "speeds", "norm", "close", "pose", "all_down")

        def kept(v):
            w = v.world
            return dict(zip(names, (t.clone() for t in (w.action_outputs["actions"], w.action_outputs["speeds"], w.obs_post["ped_vector_norm"],
                                                        w.obs_post["close_to_human"], w.out["robot_pose"], w.out["step_all_down"]))))

        def play(v, sync):
            raw = torch.zeros(E * R, dtype=torch.int64, device="cuda")
            v.reset()
            frames = []
            for s in range(rounds):
                torch.add(all_raw[s], 0, out=raw)  # the policy's last op, on the stream
                if sync:
                    torch.cuda.synchronize()
                v.step(raw)
                if sync:
                    torch.cuda.synchronize()
                frames.append(kept(v))
            return frames
        want = play(twin, True)
        torch.cuda.synchronize()
        busy = torch.randn(4096, 4096, device="cuda")
        for q in range(20):
            busy = (busy @ busy).clamp_(-1, 1)
        got = play(run, False)
        torch.cuda.synchronize()
        for s in range(rounds):
            for k in names:
                same(got[s][k].cpu().numpy(), want[s][k].cpu().numpy(), "round %d %s" % (s, k))
        assert sum(int(f["all_down"].sum()) for f in want) >= E  # restarts in between
    finally:
        run.close()
        twin.close()


# ---- 6. robot shards ----
def test_shards_decode_and_post_process_their_local_rows():
    """two handles owning halves of one 24-robot world with 10 pedestrians (step_begin, the exchange by hand, step_end) against the
    whole-world handle: the local rows of actions, speeds, ped_vector_norm and close_to_human"""
    import torch
    from img_env_amd.world import World
    n, n_peds = 24, 10
    grid, params, layout = small_world(n, n_peds, seed=31, grid_size=320, clearance=0.8, time_max=3)  # (done after four steps)
    _, _, layout2 = small_world(n, n_peds, seed=32, grid_size=320, clearance=0.8, time_max=3)
    bounds = [0, n // 2, n]
    full = World(params, grid)
    ranks = [World(dict(params, robot_begin=bounds[r], robot_end=bounds[r + 1]), grid) for r in range(2)]
    try:
        for w in [full] + ranks:
            w.enable_actions(discrete_actions=TABLE8)
            w.enable_obs_post()
        assert ranks[1].action_outputs["actions"].shape == (n // 2, 3) and ranks[1].obs_post["ped_vector_norm"].shape[0] == n // 2
        m = ActionModel(n, TABLE, table=TABLE8)

        def exchange():
            torch.cuda.synchronize()
            for r, w in enumerate(ranks):
                for q, o in enumerate(ranks):
                    if q != r:
                        w.records[bounds[q]:bounds[q + 1]].copy_(o.records[bounds[q]:bounds[q + 1]])

        def compare(where):
            for name, of in (("actions", "action_outputs"), ("speeds", "action_outputs"), ("ped_vector_norm", "obs_post"),
                             ("close_to_human", "obs_post")):
                whole = host(getattr(full, of)[name])
                same(np.concatenate([host(getattr(w, of)[name]) for w in ranks]), whole, "%s %s (shards)" % (where, name))
            raw = host(full.out["ped_vector_states"])
            same(host(full.obs_post["ped_vector_norm"]), ped_norm(raw, (raw.shape[1] - 1) // 7), where + " norm")
        rng = np.random.default_rng(5)
        for lay, k in ((layout, 8), (layout2, 6)):
            for w in [full] + ranks:
                w.reset(lay)
            m.reset(np.ones(n, bool))
            compare("reset")
            for s in range(k):
                raw = rng.integers(-1, len(TABLE8) + 1, n)  # (bad indices among them)
                a = full.decode_actions(raw)
                full.step(a)
                for r, w in enumerate(ranks):
                    w.step_begin(w.decode_actions(raw[bounds[r]:bounds[r + 1]].astype(np.int32)))
                exchange()
                for w in ranks:
                    w.step_end()
                want = m.decode(raw)
                same(host(full.action_outputs["actions"]), want, "actions %d" % s)
                same(host(full.action_outputs["speeds"]), m.speeds, "speeds %d" % s)
                m.step_done(host(full.out["step_dones"]))
                compare("step %d" % s)
        assert int(host(full.action_outputs["n_bad"])[0]) == m.n_bad > 0
        assert sum(int(host(w.action_outputs["n_bad"])[0]) for w in ranks) == m.n_bad
        assert m.masked_rows > 0
    finally:
        full.close()
        for w in ranks:
            w.close()


# ---- 7. refusals that need a handle ----
def test_refusals_that_need_a_handle():
    import torch
    from img_env_amd import _cabi
    from img_env_amd.world import World
    grid, params, layout = small_world(4, 2, seed=4)
    w = World(params, grid)
    c = World(params, grid)
    try:
        raw = torch.zeros(4, dtype=torch.int64, device="cuda")
        ao = _cabi.ActionsOut()
        assert w.lib.imgenv_actions_decode(w.h, C.c_void_p(raw.data_ptr()), _cabi.RAW_I64, None) == _cabi.ESTATE  # before enable
        assert w.lib.imgenv_actions_outputs(w.h, C.byref(ao)) == _cabi.ESTATE
        assert w.lib.imgenv_obs_post_outputs(w.h, C.byref(_cabi.ObsPostOut())) == _cabi.ESTATE
        with pytest.raises(RuntimeError):
            w.decode_actions(raw)
        first = w.enable_actions(discrete_actions=TABLE8)
        assert w.lib.imgenv_actions_decode(w.h, C.c_void_p(raw.data_ptr()), _cabi.RAW_I64, None) == _cabi.ESTATE  # before the first reset
        assert b"reset" in w.lib.imgenv_last_error()
        assert w.enable_actions(discrete_actions=TABLE8) is first  # the same cfg again: nothing changes
        for other in (dict(discrete_actions=TABLE8[:7]), dict(discrete_actions=TABLE8, act_dim=3), dict(continuous_actions=CLIP3),
                      dict(discrete_actions=[r[:2] for r in TABLE8])):
            with pytest.raises(ValueError, match="another cfg"):
                w.enable_actions(**other)
        assert w.lib.imgenv_actions_outputs(w.h, C.byref(ao)) == 0 and ao.n_local == 4
        for name, t in first.items():
            assert getattr(ao, name) == t.data_ptr(), name
        w.reset(layout)
        assert w.decode_actions(raw) is first["actions"]
        assert w.lib.imgenv_actions_decode(w.h, C.c_void_p(raw.data_ptr() + 4), _cabi.RAW_I64, None) == _cabi.EINVAL  # misaligned
        assert w.lib.imgenv_actions_decode(w.h, C.c_void_p(raw.data_ptr()), 4, None) == _cabi.EINVAL
        assert w.lib.imgenv_actions_decode(w.h, None, _cabi.RAW_I64, None) == _cabi.EINVAL
        with pytest.raises(ValueError):
            w.decode_actions(np.zeros(5, np.int64))  # one index per robot
        with pytest.raises(ValueError):
            w.decode_actions(np.zeros((4, 3), np.float32))  # act_dim is 2
        # CLIP mode takes no indices
        c.enable_actions(continuous_actions=CLIP3)
        c.reset(layout)
        with pytest.raises(ValueError, match="CLIP"):
            c.decode_actions(raw)
        with pytest.raises(ValueError, match="CLIP"):
            c.decode_actions(np.zeros(4, np.int32))
        c.decode_actions(np.zeros((4, 2), np.float64))
        with pytest.raises(ValueError, match="another cfg"):
            c.enable_actions(continuous_actions=[[0, 0.6], [-0.9, 0.8]])
        c.enable_actions(continuous_actions=[[0, 0.6], [-0.9, 0.9], [-1, 1]])  # (a range beyond act_dim is not part of the cfg)
        torch.cuda.synchronize()
    finally:
        w.close()
        c.close()


# ---- the probe's torch variant is the same computation ----
@pytest.mark.parametrize("kind", ["table", "clip"])
def test_the_probes_torch_wrappers_hand_out_the_same(kind):
    """tools/vec_env_probe.py --wrappers-compare measures the library against the same results kept with torch ops around a plain
    VecImageEnv: both must hand out the same actions, speeds, normalised vectors and close_to_human, or the comparison compares
    nothing"""
    import os
    import sys
    import torch
    from img_env_amd.vec_env import VecImageEnv
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from vec_env_probe import TABLE28, TorchWrappers
    E, R, P = 8, 3, 2
    cfg = episode_cfg(R, P, max_ped=10, wrappers=WRAPPERS, discrete_action=kind == "table", discrete_actions=TABLE28)
    lib = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, wrappers=True)
    ref = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True)
    try:
        tw = TorchWrappers(ref)
        lib.reset()
        ref.reset()
        g = torch.Generator(device="cuda").manual_seed(2)
        for s in range(16):
            if kind == "table":
                raw = torch.randint(0, len(TABLE28), (E * R,), generator=g, device="cuda")
            else:
                raw = torch.rand(E * R, 2, generator=g, device="cuda") * 3.0 - 1.5
            state, _, _, info = lib.step(raw)
            a = tw.action(raw)
            _, _, _, info_ref = ref.step(a)
            speeds, norm, close = tw.after(a, info_ref)
            same(host(lib.world.action_outputs["actions"]), host(a), "actions %d" % s)
            assert (host(info["speeds"]) == host(speeds)).all(), s  # (by value: the torch mask multiplies, -0.0 for a masked w < 0)
            same(host(state.ped_vector_states), host(norm), "norm %d" % s)
            assert (host(info["bool_get_close_to_human"]).astype(bool) == host(close)).all(), s
    finally:
        lib.close()
        ref.close()
