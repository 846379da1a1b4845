"""The policy head (imgenv_policy_*, csrc/policy.h) on the device against tests/policy_model.py: the categorical draw inside the
float64 model's CDF interval, log-probability and entropy within bounds derived from the float32 format (<= 2 ulp per expf, half
an ulp per addition of at most A partial sums <= s, one multiplication: margin = (A + 8) 2^-23), the Gaussian sample within the
angle's error, everything that is IEEE arithmetic bit for bit, bad rows, reproducibility, the rollout window's columns and the
opt-in guarantee.  Tiny worlds from the generators; every test prints its measured maxima as fractions of the bounds.

The Gaussian entropy's "2^-21 relative" is relative to the magnitudes of the numbers summed (policy_model.entropy_scale).  The
issue's equal-logits check ("wherever u 4096 is farther than margin 4096 from an integer") excludes every row, margin(4096) * 4096
being 2; with equal logits the arithmetic is exact, so the index is checked to BE floor(u 4096) on every row."""
import copy

import numpy as np
import pytest

import policy_model as pm
from action_model import CLIP, TABLE, ActionModel, decode, table_rows
from scenarios import small_world
from stack_model import bits
from test_gpu_episodes import episode_cfg

pytestmark = pytest.mark.gpu
F32 = np.float32
TABLE8 = [[0.0, -0.9], [0.0, 0.3], [0.2, -0.6], [0.2, 0.0], [0.4, 0.6], [0.6, -0.3], [0.6, 0.0, 1], [0.6, 0.9]]
CLIP3 = [[0, 0.6], [-0.9, 0.9], [-0.6, 0.6]]
ROWS = (1, 63, 65, 257)
WIDTHS = (1, 2, 3, 8, 16, 17, 64, 65, 257, 1025, 4096)
SCALES = (0.0, 1.0, 8.0, 30.0)
SEED = (0x1234 << 32) | 0x9abcdef1
_worlds = {}


def tiny_world(R):
    """(grid, params, layout) of R robots without pedestrians, made once per size"""
    if R not in _worlds:
        _worlds[R] = small_world(R, 0, seed=11, grid_size=480, clearance=0.7)
    return _worlds[R]


def table_of(A):
    rng = np.random.default_rng(A)
    return np.stack([rng.uniform(0, 0.6, A), rng.uniform(-0.9, 0.9, A), rng.integers(0, 2, A)], axis=1).astype(F32).tolist()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def same(got, want, where):
    g, w = np.asarray(got), np.asarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (where, g.dtype, w.dtype, g.shape, w.shape)
    eq = (g == w) if g.dtype.itemsize == 1 else (bits(g) == bits(w))
    assert eq.all(), "%s differs at %s (%d of %d)" % (where, np.argwhere(~eq)[0].tolist(), (~eq).sum(), eq.size)


def uniforms(R, draw, seed=SEED, begin=0):
    return pm.u01(pm.draw_block(np.arange(R, dtype=np.uint64) + np.uint64(begin), draw, seed)[:, 0])


def categorical_world(R, A, seed=SEED):
    from img_env_amd.world import World
    grid, params, layout = tiny_world(R)
    w = World(params, grid)
    table = table_of(A)
    w.enable_actions(discrete_actions=table, act_dim=3)
    w.enable_policy("categorical", seed)
    w.reset(layout)
    return w, table


# ---- 1. categorical: the draw, log-probability and entropy against the float64 model; 2. the decode bit for bit ----
@pytest.mark.parametrize("R", ROWS)
def test_categorical_against_the_model(R):
    worst = dict(interval=0.0, logp=0.0, entropy=0.0)
    rng = np.random.default_rng(R)
    rows = np.arange(R)
    for A in WIDTHS:
        w, table = categorical_world(R, A)
        try:
            mg, model = pm.margin(A), ActionModel(R, TABLE, table=table, n_cols=3)
            for draw, scale in enumerate(SCALES):
                l = pm.make_logits(rng, R, A, scale)
                acts = w.policy_sample(l, draw=draw)
                assert acts is w.action_outputs["actions"]
                k, logp, ent = host(w.policy["index"]), host(w.policy["logp"]), host(w.policy["entropy"])
                u, ref = uniforms(R, draw), pm.categorical_truth(l)
                where = "R %d A %d scale %g" % (R, A, scale)
                assert k.dtype == np.int32 and (k >= 0).all() and (k < A).all(), where
                F, p = ref["cdf"], ref["p"]
                below = np.where(k > 0, F[rows, np.maximum(k - 1, 0)], 0.0)
                worst["interval"] = max(worst["interval"], float(np.maximum(below - u, u - F[rows, k]).max() / mg))
                lp, H = ref["logp"][rows, k], ref["entropy"]
                e_lp = np.abs(logp - lp) / (2.0 ** -22 * (1 + np.abs(lp)) + mg)
                e_H = np.abs(ent - H) / (2.0 ** -22 * (1 + H) + mg * (1 + np.log(A)))
                worst["logp"], worst["entropy"] = max(worst["logp"], float(e_lp.max())), max(worst["entropy"], float(e_H.max()))
                assert (below - mg <= u).all() and (u <= F[rows, k] + mg).all() and (p[rows, k] > 0).all(), where  # no row excluded
                assert (e_lp <= 1).all() and (e_H <= 1).all(), (where, e_lp.max(), e_H.max())
                # the decode of the kernel's own index, bit for bit
                same(host(acts), model.decode(k), where + " actions")
                same(host(w.action_outputs["speeds"]), model.speeds, where + " speeds")
                # the mode: the lowest index of the maximum, exact; its log-probability within the same bound
                w.policy_sample(l, draw=draw, deterministic=True)
                kd = host(w.policy["index"])
                same(kd, np.argmax(l, axis=1).astype(np.int32), where + " mode")
                assert (np.abs(host(w.policy["logp"]) - ref["logp"][rows, kd]) <= 2.0 ** -22 * (1 + np.abs(ref["logp"][rows, kd])) + mg).all()
                same(host(w.policy["entropy"]), ent, where + " entropy of the mode call")
            assert int(host(w.action_outputs["n_bad"])[0]) == 0
        finally:
            w.close()
    print("categorical R %d: worst fraction of the bound: interval %.3f, logp %.3f, entropy %.3f" % (R, worst["interval"], worst["logp"], worst["entropy"]))


def test_equal_logits_pin_the_generators_high_bits():
    R, A = 257, 4096
    w, _ = categorical_world(R, A)
    try:
        seen = set()
        for draw in (0, 1, (7 << 32) | 5):
            w.policy_sample(np.zeros((R, A), F32), draw=draw)
            k, x = host(w.policy["index"]), uniforms(R, draw).astype(np.float64) * A
            same(k, np.floor(x).astype(np.int32), "draw %d" % draw)
            same(host(w.policy["logp"]), np.full(R, -np.log(F32(4096)), F32), "logp")
            seen |= set(k.tolist())
        assert len(seen) > 600
    finally:
        w.close()


# ---- 3. Gaussian ----
@pytest.mark.parametrize("C", (2, 3))
def test_gaussian_against_the_model(C):
    from img_env_amd.world import World
    R = 257
    grid, params, layout = tiny_world(R)
    w = World(params, grid)
    try:
        w.enable_actions(continuous_actions=CLIP3, act_dim=C)
        pol = w.enable_policy("gaussian", SEED)
        assert pol["raw"].shape == (R, C) and "index" not in pol and "pol_raw" not in pol
        w.reset(layout)
        rng = np.random.default_rng(C)
        g = np.arange(R)
        worst = dict(z=0.0, raw=0.0, logp=0.0, entropy=0.0)
        zero = np.zeros((R, C), F32)
        for draw in range(8):  # mean 0, log_std 0: raw is z
            w.policy_sample(zero, log_std=np.zeros(C, F32), draw=draw)
            zt = pm.normals(g, draw, SEED, C, truth=True)
            e = np.abs(host(w.policy["raw"]) - zt) / (2.0 ** -18 * (1 + np.abs(zt)))
            worst["z"] = max(worst["z"], float(e.max()))
            assert (e <= 1).all(), (draw, e.max())
        model = ActionModel(R, CLIP, clip=CLIP3, n_cols=C)
        for draw, per_row in ((20, False), (21, True), (22, False), (23, True)):
            mu = (rng.standard_normal((R, C)) * 0.5).astype(F32)
            ls = rng.uniform(-5, 1, (R, C) if per_row else (C,)).astype(F32)
            acts = w.policy_sample(mu, log_std=ls, draw=draw)
            raw, logp, ent = host(w.policy["raw"]), host(w.policy["logp"]), host(w.policy["entropy"])
            zt = pm.normals(g, draw, SEED, C, truth=True)
            ref = pm.gaussian_truth(mu, ls, zt)
            sigma = np.exp(np.broadcast_to(ls.astype(np.float64).reshape(-1, C), (R, C)))
            e_raw = np.abs(raw - ref["raw"]) / (sigma * 2.0 ** -18 * (1 + np.abs(zt)) + 2.0 ** -22 * (1 + np.abs(mu)))
            e_lp = np.abs(logp - ref["logp"]) / ((np.abs(zt) * 2.0 ** -18 * (1 + np.abs(zt))).sum(axis=1) + 2.0 ** -21 * (1 + np.abs(ref["logp"])))
            e_H = np.abs(ent - ref["entropy"]) / (2.0 ** -21 * pm.entropy_scale(ls, R, C))
            for key, e in (("raw", e_raw), ("logp", e_lp), ("entropy", e_H)):
                worst[key] = max(worst[key], float(e.max()))
            assert (e_raw <= 1).all() and (e_lp <= 1).all() and (e_H <= 1).all(), (draw, e_raw.max(), e_lp.max(), e_H.max())
            # actions: the CLIP rule on the kernel's own raw, bit for bit; the clip must bite somewhere
            want = model.decode(raw)
            same(host(acts), want, "draw %d actions" % draw)
            same(host(w.action_outputs["speeds"]), model.speeds, "draw %d speeds" % draw)
            assert (want[:, :C] != raw).any()
            # the mode is the mean, bit for bit
            w.policy_sample(mu, log_std=ls, draw=draw, deterministic=True)
            same(host(w.policy["raw"]), mu + F32(0), "mode")
            same(host(w.policy["entropy"]), ent, "entropy of the mode call")
        assert int(host(w.action_outputs["n_bad"])[0]) == 0
        print("gaussian C %d: worst fraction of the bound: z %.3f, raw %.3f, logp %.3f, entropy %.3f" % (C, worst["z"], worst["raw"], worst["logp"], worst["entropy"]))
    finally:
        w.close()


# ---- 4. bad rows ----
@pytest.mark.parametrize("A", (3, 17, 300))
def test_bad_categorical_rows_and_their_neighbours(A):
    R = 257
    w, table = categorical_world(R, A)
    try:
        rng = np.random.default_rng(A)
        l = pm.make_logits(rng, R, A, 1.0)
        clean = l.copy()
        bad = [0, 1, 63, 64, 130, R - 1]
        l[0, A - 1] = np.nan
        l[1, 0] = np.inf
        l[63, :] = -np.inf
        l[64, A // 2] = np.nan
        l[130, :] = -np.inf
        l[R - 1, 0] = np.inf
        w.policy_sample(clean, draw=3)
        k0, lp0, H0, a0 = (host(t) for t in (w.policy["index"], w.policy["logp"], w.policy["entropy"], w.action_outputs["actions"]))
        w.policy_sample(l, draw=3)
        k, lp, H, a = (host(t) for t in (w.policy["index"], w.policy["logp"], w.policy["entropy"], w.action_outputs["actions"]))
        assert (k[bad] == -1).all() and (lp[bad] == 0).all() and (H[bad] == 0).all() and (a[bad] == 0).all()
        assert (host(w.action_outputs["speeds"])[bad] == 0).all()
        ok = np.setdiff1d(np.arange(R), bad)  # the neighbours in the same group and wavefront: as without the bad rows
        same(k[ok], k0[ok], "index")
        same(lp[ok], lp0[ok], "logp")
        same(H[ok], H0[ok], "entropy")
        same(a[ok], a0[ok], "actions")
        assert int(host(w.action_outputs["n_bad"])[0]) == len(bad)
        w.policy_sample(l, draw=4, deterministic=True)
        assert int(host(w.action_outputs["n_bad"])[0]) == 2 * len(bad) and (host(w.policy["index"])[bad] == -1).all()
    finally:
        w.close()


def test_bad_gaussian_rows_and_their_neighbours():
    from img_env_amd.world import World
    R, C = 130, 3
    grid, params, layout = small_world(R, 0, seed=11, grid_size=480, clearance=0.7)
    w = World(params, grid)
    try:
        w.enable_actions(continuous_actions=CLIP3, act_dim=C)
        w.enable_policy("gaussian", SEED)
        w.reset(layout)
        rng = np.random.default_rng(1)
        mu, ls = rng.standard_normal((R, C)).astype(F32), rng.uniform(-2, 0, (R, C)).astype(F32)
        w.policy_sample(mu, log_std=ls, draw=1)
        raw0, lp0 = host(w.policy["raw"]), host(w.policy["logp"])
        bad = [0, 63, 64, R - 1]
        mu2, ls2 = mu.copy(), ls.copy()
        mu2[0, 1] = np.nan
        mu2[63, 2] = np.inf
        ls2[64, 0] = 100.0
        ls2[R - 1, 2] = np.nan
        w.policy_sample(mu2, log_std=ls2, draw=1)
        raw, lp, H, a = (host(t) for t in (w.policy["raw"], w.policy["logp"], w.policy["entropy"], w.action_outputs["actions"]))
        assert (raw[bad] == 0).all() and (lp[bad] == 0).all() and (H[bad] == 0).all() and (a[bad] == 0).all()
        ok = np.setdiff1d(np.arange(R), bad)
        same(raw[ok], raw0[ok], "raw")
        same(lp[ok], lp0[ok], "logp")
        assert int(host(w.action_outputs["n_bad"])[0]) == len(bad)
    finally:
        w.close()


# ---- 5. reproducibility ----
def test_same_seed_and_draw_same_bits():
    R, A = 65, 17
    rng = np.random.default_rng(0)
    l = pm.make_logits(rng, R, A, 1.0)
    l[1] = l[0]  # two robots with equal logits draw different u

    def run(seed, draw):
        w, _ = categorical_world(R, A, seed)
        try:
            w.policy_sample(l, draw=draw)
            return [host(t) for t in (w.policy["index"], w.policy["logp"], w.policy["entropy"], w.action_outputs["actions"], w.action_outputs["speeds"])]
        finally:
            w.close()
    a, b, other_draw, other_seed = run(SEED, 5), run(SEED, 5), run(SEED, 6), run(SEED + 1, 5)
    for x, y in zip(a, b):
        same(x, y, "same seed and draw")
    assert (a[0] != other_draw[0]).any() and (a[0] != other_seed[0]).any()
    same(a[2], other_draw[2], "the entropy does not depend on the draw")
    u = uniforms(R, 5)
    assert u[0] != u[1]
    w, _ = categorical_world(R, A)
    try:
        pairs = []
        for draw in range(16):
            w.policy_sample(l, draw=draw)
            pairs.append(host(w.policy["index"])[:2].tolist())
        assert any(k0 != k1 for k0, k1 in pairs)
    finally:
        w.close()


def test_enable_and_sample_refusals():
    from img_env_amd.world import World
    grid, params, layout = tiny_world(1)
    w = World(params, grid)
    try:
        with pytest.raises(RuntimeError):
            w.enable_policy("categorical", 1)  # before enable_actions
        w.enable_actions(discrete_actions=TABLE8)
        with pytest.raises(ValueError):
            w.enable_policy("gaussian", 1)  # TABLE mode serves the categorical head
        with pytest.raises(RuntimeError):
            w.enable_policy("categorical", 1, store=True)  # before enable_rollout
        pol = w.enable_policy("categorical", 1)
        assert w.enable_policy("categorical", 1) is pol and set(pol) == {"index", "logp", "entropy"}
        with pytest.raises(ValueError):
            w.enable_policy("categorical", 2)  # another cfg
        with pytest.raises(RuntimeError):
            w.policy_sample(np.zeros((1, 8), F32))  # before the first reset
        w.reset(layout)
        with pytest.raises(ValueError):
            w.policy_sample(np.zeros((1, 7), F32))
        with pytest.raises(RuntimeError):
            w.policy_value(np.zeros(1, F32))  # a head without STORE
        w.step(w.policy_sample(np.zeros((1, 8), F32)))
        with_head = w.launches()
        w.step(w.decode_actions(np.zeros(1, np.int64)))
        assert w.launches() == with_head  # one launch in front of the step, either way
    finally:
        w.close()


# ---- 6. the window ----
def logits_for(state_vs, rng):
    """a goal-seeking preference over TABLE8 plus noise, one action masked"""
    vs = np.asarray(state_vs, np.float64)
    ang = np.arctan2(vs[:, 1], vs[:, 0])
    t = table_rows(TABLE8).astype(np.float64)
    v, wz = np.where(np.abs(ang) < 0.7, 0.6, 0.1), np.clip(2.0 * ang, -0.9, 0.9)
    l = -8.0 * ((t[None, :, 0] - v[:, None]) ** 2 + (t[None, :, 1] - wz[:, None]) ** 2) + rng.standard_normal((len(vs), len(t)))
    l[:, 6] = -np.inf
    return l.astype(F32)


def test_the_window_keeps_what_was_handed_out():
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T, B = 16, 3, 2, 3, 32
    cfg = episode_cfg(R, P, discrete_action=True, discrete_actions=TABLE8)
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, wrappers=True, rollout=T, minibatch=B, policy=dict(seed=SEED))
    try:
        n = E * R
        rng = np.random.default_rng(3)
        state = vec.reset()
        for window in range(2):
            handed, vals = [], []
            for t in range(T):
                l = logits_for(host(state.vector_states), rng)
                v = torch.as_tensor(rng.standard_normal(n).astype(F32), device="cuda")
                draw = vec.policy_draw
                state, rew, done, info = vec.policy_step(logits=torch.as_tensor(l, device="cuda"), values=v)
                assert vec.policy_draw == draw + 1 and set(info["policy"]) == {"actions", "index", "logp", "entropy"}
                k = host(info["policy"]["index"])
                assert (k != 6).all() and (k >= 0).all()
                same(host(info["policy"]["actions"]), decode(k, TABLE, table_rows(TABLE8))[0], "actions")
                handed.append((k, host(info["policy"]["logp"])))
                vals.append(host(v))
            boot = torch.as_tensor(rng.standard_normal(n).astype(F32), device="cuda")
            vec.policy_value(boot)
            ro = vec.rollout()
            assert ro["n"] == T and ro["pol_raw"].shape == (1, T, n) and ro["pol_logp"].shape == (T, n) and ro["pol_value"].shape == (T + 1, n)
            for t in range(T):
                same(host(ro["pol_raw"])[0, t], handed[t][0].astype(F32), "window %d pol_raw[%d]" % (window, t))
                same(host(ro["pol_logp"])[t], handed[t][1], "pol_logp[%d]" % t)
                same(host(ro["pol_value"])[t], vals[t], "pol_value[%d]" % t)
                same(host(ro["actions"])[t], decode(handed[t][0], TABLE, table_rows(TABLE8))[0], "ring actions[%d]" % t)
            same(host(ro["pol_value"])[T], host(boot), "the bootstrap value")
            assembled = torch.as_tensor(np.stack(vals + [host(boot)]), device="cuda")
            adv, ret = vec.rollout_advantages(ro["pol_value"])
            adv2, ret2 = vec.rollout_advantages(assembled)
            same(host(adv), host(adv2), "advantages")
            same(host(ret), host(ret2), "returns")
            flat_lp, flat_k = host(ro["pol_logp"]).ravel(), host(ro["pol_raw"])[0].ravel()
            gathered = 0
            for mb in vec.rollout_minibatches({"logp": ro["pol_logp"], "act": ro["pol_raw"][0]}, seed=5 + window):
                idx, wt = host(mb["mb_index"]), host(mb["mb_weight"])
                take = wt > 0
                same(host(mb["logp"])[take], flat_lp[idx[take]], "gathered logp")
                same(host(mb["act"])[take], flat_k[idx[take]], "gathered act")
                gathered += int(take.sum())
            assert gathered == int((host(ro["is_clean"]) != 0).sum()) > 0
            # the window is full: a storing sample raises and queues nothing; an evaluation call does not touch it
            l = torch.zeros((n, 8), device="cuda")
            with pytest.raises(RuntimeError):
                vec.policy_sample(logits=l)
            before = host(ro["pol_logp"])
            vec.policy_sample(logits=l, store=False)
            same(host(vec.rollout()["pol_logp"]), before, "NO_STORE")
            vec.rollout_begin()
            assert vec.rollout()["n"] == 0  # ... and the next window's slot 0 is written again
    finally:
        vec.close()


def test_speeds_of_frozen_robots_are_masked_and_host_resets_store_too():
    """auto_reset=False and a time limit of 10: robots end their episodes one by one and every one has by step 10; the policy head
    masks their speeds with the is_clean of before the step, as the decode does"""
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P = 4, 3, 2
    cfg = episode_cfg(R, P, discrete_action=True, discrete_actions=TABLE8)
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, auto_reset=False, wrappers=True, policy=dict(seed=1))
    try:
        n = E * R
        rng = np.random.default_rng(4)
        m = ActionModel(n, TABLE, table=TABLE8)
        state = vec.reset()
        for s in range(12):
            l = logits_for(host(state.vector_states), rng)
            state, rew, done, info = vec.policy_step(logits=l)
            m.decode(host(info["policy"]["index"]))
            same(host(info["policy"]["actions"]), m.actions, "step %d actions" % s)
            same(host(info["speeds"]), m.speeds, "step %d speeds" % s)
            m.step_done(host(done))
        assert m.masked_rows >= n and not m.is_clean.any()
    finally:
        vec.close()


# ---- 7. opt-in ----
def test_the_feature_disturbs_nothing():
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P = 16, 3, 2
    cfg = episode_cfg(R, P, discrete_action=True, discrete_actions=TABLE8)
    off, on = (VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, wrappers=True, policy=p) for p in (None, dict(seed=3)))
    try:
        assert off.world.policy is None
        with pytest.raises(RuntimeError):
            off.policy_sample(logits=np.zeros((E * R, 8), F32))
        rng = np.random.default_rng(8)
        s_off, s_on = off.reset(), on.reset()
        for step in range(5):
            same(host(s_on.vector_states), host(s_off.vector_states), "step %d state" % step)
            l = logits_for(host(s_off.vector_states), rng)
            k = np.argmax(l, axis=1)
            s_off, r_off, d_off, i_off = off.step(k)
            s_on, r_on, d_on, i_on = on.policy_step(logits=l, deterministic=True)
            same(host(i_on["policy"]["index"]), k.astype(np.int32), "step %d index" % step)
            assert off.world.launches() == on.world.launches()
            for name in ("vector_states", "sensor_maps", "lasers", "ped_maps", "rewards", "dones", "step_rewards", "step_dones_info"):
                same(host(on.world.out[name]), host(off.world.out[name]), "step %d %s" % (step, name))
            same(host(r_on), host(r_off), "rewards")
            same(host(d_on), host(d_off), "dones")
            same(host(i_on["speeds"]), host(i_off["speeds"]), "speeds")
    finally:
        off.close()
        on.close()
    with pytest.raises(ValueError):
        VecImageEnv(copy.deepcopy(cfg), env_num=2, seed=9, policy=dict(seed=3))  # needs wrappers=True
