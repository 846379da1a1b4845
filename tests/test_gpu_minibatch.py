"""The rollout minibatches on the device (imgenv_rollout_minibatch_enable, imgenv_rollout_index / _stats / _shuffle / _minibatch,
csrc/minibatch.h) against tests/minibatch_model.py.  The index, the shuffle and the gather move integers and bytes, the
normalisation is two float32 roundings: those comparisons are exact.  The statistics are held to the final roundings (see
test_statistics).  Shapes and helpers are tests/test_gpu_rollout.py's."""
import copy
import ctypes as C
import functools
import math

import numpy as np
import pytest

import minibatch_model as mm
from scenarios import small_world
from test_gpu_final_obs import TABLE8, WRAPPERS, fixed_actions, host, narrow_cfg, same

pytestmark = pytest.mark.gpu
STALE = "rollout changed since imgenv_rollout_index"
RING_SCALARS = ("actions", "rewards", "dones", "dones_info")
SEEDS = (0x0123456789ABCDEF, 7)


def obs_fields(ring):
    return {k[4:]: v for k, v in ring.items() if k.startswith("obs_")}


def model_minibatch(ring, order, j, B, fields, scalars=(), normalise=None, norm=None):
    return mm.gather(order, j, B, {f: ring["obs_" + f] for f in fields}, {k: ring[k] for k in RING_SCALARS}, scalars, normalise, norm)


def compare_minibatch(got, want, n_scalars, where):
    assert set(want) <= set(got), (where, set(want) - set(got))
    for name, w in want.items():
        g = got[name][:n_scalars] if name == "mb_scalars" else got[name]
        same(g, w, "%s: %s" % (where, name))


def caller_scalars(T, R, seed):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randn((T, R), generator=g).cuda(), torch.randn((T, R), generator=g).cuda(), torch.randn((T + 1, R), generator=g).cuda()]


# ---- 1. 90 transitions: a tail of 10 flags inside one tile; device_reset, stacks and wrappers on ----
@functools.lru_cache(maxsize=None)
def case90():
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T, B = 5, 3, 2, 6, 32
    cfg = narrow_cfg(R, P, max_ped=10, wrappers=WRAPPERS, discrete_action=True, discrete_actions=TABLE8, image_batch=2, state_batch=3, laser_batch=2)
    acts = np.random.default_rng(3).integers(0, len(TABLE8), (T, E * R)).astype(np.int64)
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=True, device_reset=True, stack=True, wrappers=True, rollout=T,
                      rollout_final=64, minibatch=B, minibatch_buffers=2)
    try:
        w = vec.world
        rec = {"shapes": {k: (tuple(v.shape), str(v.dtype), v.data_ptr()) for k, v in w.minibatch.items()},
               "ring_shapes": {k: (tuple(v.shape), str(v.dtype)) for k, v in w.rollout.items()}}
        vec.reset()
        for t in range(T):
            vec.step(acts[t])
        rec["ring"] = host(w.rollout)
        w.rollout_index()
        rec["valid_count"] = w.rollout_valid_count()
        rec["index"] = host({k: w.minibatch[k] for k in ("valid", "valid_n")})
        sc = caller_scalars(T, E * R, 5)
        norm = torch.tensor([0.25, 2.0], device="cuda")
        rec["scalars"] = [s.cpu().numpy() for s in sc]
        rec["orders"], rec["mbs"] = [], []
        for seed in SEEDS:
            w.rollout_shuffle(seed)
            rec["orders"].append(host({"order": w.minibatch["order"]})["order"])
        for j in range(4):  # three minibatches cover 90 slots; the fourth lies behind T R
            rec["mbs"].append(host(w.rollout_minibatch(j, j % 2, sc, normalise=0, norm=norm)))
        # through the vectorised env: the library's own norm, the scalars under the caller's names
        names = dict(zip(("adv", "logp", "values"), sc))
        rec["epoch"] = [host(mb) for mb in vec.rollout_minibatches(names, SEEDS[0], normalise="adv")]
        rec["epoch_norm"] = host({"norm": w.minibatch["norm"]})["norm"]
        rec["ring_after"] = host(w.rollout)
        with pytest.raises(ValueError):
            w.rollout_minibatch(0, 0, [sc[0][:-1]])
        with pytest.raises(ValueError):
            w.rollout_minibatch(0, 2, sc)  # buffer 2 of 2
        with pytest.raises(ValueError):
            w.rollout_stats(sc[2])  # [T + 1, R]
    finally:
        vec.close()
    return rec, (E, R, T, B)


def test_index_equals_flatnonzero_and_order_equals_the_model():
    rec, (E, R, T, B) = case90()
    valid = mm.valid_list(rec["ring"]["is_clean"], T)
    V = len(valid)
    print("valid_n", V, "of", T * E * R)
    assert int(rec["index"]["valid_n"][0]) == V == rec["valid_count"]
    same(rec["index"]["valid"][:V], valid, "valid")
    assert 0 < V <= T * E * R
    for seed, order in zip(SEEDS, rec["orders"]):
        same(order, mm.order_list(valid, T * E * R, seed), "order under seed %x" % seed)
    assert (rec["orders"][0] != rec["orders"][1]).any()
    sh = rec["shapes"]
    assert sh["valid"][:2] == ((T * E * R,), "torch.int32") and sh["order"][:2] == ((T * E * R,), "torch.int32") and sh["norm"][:2] == ((2,), "torch.float32")
    assert all(ptr % 256 == 0 for _, _, ptr in sh.values())
    for name, (shape, dtype) in rec["ring_shapes"].items():  # [buffers, B, row...] with the ring's row shapes and types
        if name.startswith("obs_"):
            assert sh["mb_" + name[4:]][:2] == ((2, B) + shape[2:], dtype), name
    assert sh["mb_scalars"][0] == (2, 6, B) and sh["mb_actions"][0] == (2, B, 3) and sh["mb_dones"][:2] == ((2, B), "torch.uint8")


def test_every_minibatch_equals_the_model():
    rec, (E, R, T, B) = case90()
    ring, order = rec["ring"], rec["orders"][1]  # (the last shuffle: SEEDS[1])
    fields = list(obs_fields(ring))
    assert set(fields) == {"stack_sensor_maps", "stack_vector_states", "stack_lasers", "ped_vector_norm", "ped_maps"}
    V = int(rec["index"]["valid_n"][0])
    for j, got in enumerate(rec["mbs"]):
        want = model_minibatch(ring, order, j, B, fields, rec["scalars"], 0, np.array([0.25, 2.0], np.float32))
        compare_minibatch(got, want, 3, "minibatch %d" % j)
    last = rec["mbs"][V // B] if V % B else None
    if last is not None:  # the last minibatch with a transition in it: its tail is empty
        k = V % B
        assert (last["mb_index"][:k] >= 0).all() and (last["mb_index"][k:] == -1).all() and (last["mb_weight"][k:] == 0).all()
        assert not last["mb_ped_maps"][k:].any() and not last["mb_scalars"][:, k:].any() and last["mb_weight"][:k].tolist() == [1.0] * k
    assert (rec["mbs"][3]["mb_index"] == -1).all() and not rec["mbs"][3]["mb_weight"].any()  # behind T R
    seen = np.concatenate([m["mb_index"] for m in rec["mbs"]])
    assert sorted(seen[seen >= 0].tolist()) == rec["index"]["valid"][:V].tolist()  # every transition that counts, once


def test_an_epoch_through_the_vectorised_env_and_the_ring_stays():
    rec, (E, R, T, B) = case90()
    ring = rec["ring"]
    valid = mm.valid_list(ring["is_clean"], T)
    order = mm.order_list(valid, T * E * R, SEEDS[0])
    assert len(rec["epoch"]) == -(-T * E * R // B)
    norm = rec["epoch_norm"]
    for j, got in enumerate(rec["epoch"]):
        want = model_minibatch(ring, order, j, B, list(obs_fields(ring)), rec["scalars"], 0, norm)
        sc = want.pop("mb_scalars")
        assert "mb_scalars" not in got
        for s, name in enumerate(("adv", "logp", "values")):
            same(got[name], sc[s], "epoch minibatch %d: %s" % (j, name))
        compare_minibatch(got, want, 0, "epoch minibatch %d" % j)
    for f in ring:
        assert ring[f].tobytes() == rec["ring_after"][f].tobytes(), f


# ---- 2. 4800 transitions: two tiles; vector_states and sensor_maps only; 5. the statistics ----
@functools.lru_cache(maxsize=None)
def case4800():
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T, B = 40, 3, 2, 40, 100
    vec = VecImageEnv(narrow_cfg(R, P), env_num=E, seed=9, device_reset=True, rollout=T, rollout_final=64, rollout_fields=["vector_states", "sensor_maps"],
                      minibatch=B)
    try:
        w = vec.world
        acts = fixed_actions(T, E * R)
        vec.reset()
        for t in range(T):
            vec.step(torch.as_tensor(acts[t], device="cuda"))
        rec = {"ring": host(w.rollout)}
        w.rollout_index()
        w.rollout_shuffle(SEEDS[1])
        rec["index"] = host({k: w.minibatch[k] for k in ("valid", "valid_n", "order")})
        sc = caller_scalars(T, E * R, 6)
        rec["scalars"] = [s.cpu().numpy() for s in sc]
        rec["mbs"] = {j: host(w.rollout_minibatch(j, 0, sc[:1])) for j in (0, 47)}
        g = torch.Generator(device="cpu").manual_seed(8)
        x = (1.0 + torch.randn((T, E * R), generator=g)).cuda()
        out_a, out_b = torch.zeros(2, device="cuda"), torch.full((2,), 9.0, device="cuda")
        assert w.rollout_stats(x, 1e-8, out=out_a) is out_a
        w.rollout_stats(x, 1e-8, out=out_b)
        own = w.rollout_stats(x, 1e-8)
        assert own is w.minibatch["norm"]
        rec["stats"] = host({"x": x, "a": out_a, "b": out_b, "own": own})
    finally:
        vec.close()
    return rec, (E, R, T, B)


def test_two_tiles_index_order_and_minibatches():
    rec, (E, R, T, B) = case4800()
    TR = T * E * R
    assert TR == 4800 > 4096
    valid = mm.valid_list(rec["ring"]["is_clean"], T)
    V = len(valid)
    print("valid_n", V, "of", TR)
    assert int(rec["index"]["valid_n"][0]) == V and 0 < V
    assert (valid >= 4096).any()  # (the second tile contributes)
    same(rec["index"]["valid"][:V], valid, "valid")
    order = mm.order_list(valid, TR, SEEDS[1])
    same(rec["index"]["order"], order, "order")
    assert set(obs_fields(rec["ring"])) == {"vector_states", "sensor_maps"}
    for j, got in rec["mbs"].items():
        assert "mb_ped_maps" not in got
        compare_minibatch(got, model_minibatch(rec["ring"], order, j, B, ["vector_states", "sensor_maps"], rec["scalars"][:1]), 1, "minibatch %d" % j)


def test_statistics():
    """x = 1 + standard normal: |mean| >= 0.5 mean|x|, nothing cancels.  The float64 accumulation error is at most
    (V + 2) 2^-53 sum|x| / V, orders of magnitude below a float32 ulp, so the bars are the final roundings: norm[0] within 1 float32
    ulp of float32(fsum mean), norm[1] within 2 ulp of the float64 value; two calls give identical bits."""
    rec, (E, R, T, B) = case4800()
    s = rec["stats"]
    valid = mm.valid_list(rec["ring"]["is_clean"], T)
    v = s["x"].reshape(-1)[valid].astype(np.float64)
    V = len(v)
    assert V > 4096  # more than one tile of partial sums
    assert s["a"].tobytes() == s["b"].tobytes() == s["own"].tobytes()
    mean = math.fsum(v) / V
    assert abs(mean) >= 0.5 * float(np.abs(v).mean())
    var = float(np.mean((v - mean) ** 2))  # the population variance
    inv = 1.0 / math.sqrt(var + 1e-8)
    err0 = abs(float(s["a"][0]) - float(np.float32(mean))) / float(np.spacing(np.float32(mean)))
    err1 = abs(float(s["a"][1]) - inv) / float(np.spacing(np.float32(inv)))
    print("V", V, "norm", s["a"], "ulps", err0, err1, "model", mm.stats(s["x"], valid, T * E * R, 1e-8))
    assert err0 <= 1.0 and err1 <= 2.0
    assert (V + 2) * 2.0 ** -53 * float(np.abs(v).sum()) / V < 1e-3 * float(np.spacing(np.float32(mean)))


# ---- 3. a gather that strides: ped_maps at B = 256; 4. valid_n < B and valid_n == 0 ----
def test_ped_maps_at_256_slots_strides_and_a_window_of_frozen_robots_is_all_weight_zero():
    """5 envs x 3 robots, auto_reset=False, windows of 3 steps, time_max 5.  ped_maps alone is 1728 chunks a row: 256 slots are
    more chunks than ROLLOUT_MAX_BLOCKS x ROLLOUT_BLOCK lanes take in one pass.  The first window (steps 1-3) has 45 transitions, most of
    them clean: valid_n < B.  By step 5 every robot has timed out, so the third window (steps 7-9) holds frozen robots only: valid_n = 0,
    the statistics are (0, 1), the order is all -1 and the minibatch all zeros with weight 0."""
    import torch
    from img_env_amd import _cabi
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T, B = 5, 3, 2, 3, 256
    vec = VecImageEnv(narrow_cfg(R, P), env_num=E, seed=9, auto_reset=False, rollout=T, rollout_final=8)
    try:
        w = vec.world
        assert w.minibatch is None
        with pytest.raises(RuntimeError, match="minibatch=B"):
            vec.rollout_minibatches({}, 1)
        with pytest.raises(ValueError, match="rollout stores"):
            w.enable_minibatch(B, 1, ["ped_maps", "ped_vector_norm"])
        mb_views = w.enable_minibatch(B, 1, ["ped_maps"])
        assert w.enable_minibatch(B, 1, ["ped_maps"]) is mb_views
        for other in ((B + 1, 1, ["ped_maps"]), (B, 2, ["ped_maps"]), (B, 1, None)):
            with pytest.raises(ValueError, match="already"):
                w.enable_minibatch(*other)
        assert {k for k in mb_views if k.startswith("mb_")} == {"mb_ped_maps"} | set(_cabi.MB_SCALARS)
        chunks = int(np.prod(mb_views["mb_ped_maps"].shape[2:])) * 4 // 16
        assert chunks == 1728 and B * chunks > _cabi.ROLLOUT_MAX_BLOCKS * _cabi.ROLLOUT_BLOCK
        acts = fixed_actions(3 * T, E * R)
        x = torch.ones((T, E * R), device="cuda")
        vec.reset()
        for window in range(3):
            if window:
                vec.rollout_begin()
            for t in range(T):
                vec.step(torch.as_tensor(acts[window * T + t], device="cuda"))
            if window == 1:
                continue
            ring = host(w.rollout)
            w.rollout_index()
            norm = w.rollout_stats(x, 0.0)
            w.rollout_shuffle(3)
            got = host(w.rollout_minibatch(0, 0, [x], normalise=0))
            idx = host({k: w.minibatch[k] for k in ("valid", "valid_n", "order", "norm")})
            valid = mm.valid_list(ring["is_clean"], T)
            V = len(valid)
            print("window", window, "valid_n", V)
            assert int(idx["valid_n"][0]) == V == w.rollout_valid_count() and V < B
            order = mm.order_list(valid, T * E * R, 3)
            same(idx["order"], order, "order")
            assert idx["norm"].tolist() == ([1.0, 1.0] if V else [0.0, 1.0])  # x == 1: var + eps == 0
            compare_minibatch(got, model_minibatch(ring, order, 0, B, ["ped_maps"], [x.cpu().numpy()], 0, idx["norm"]), 1, "window %d" % window)
            assert (got["mb_weight"][V:] == 0).all() and not got["mb_ped_maps"][V:].any()
            if window == 0:
                assert V > 0 and got["mb_ped_maps"][:V].any()
            else:
                assert V == 0 and (idx["order"] == -1).all() and not got["mb_weight"].any() and (got["mb_index"] == -1).all()
    finally:
        vec.close()


# ---- 6. the stale generation ----
def test_a_chain_behind_the_index_makes_it_stale():
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T = 5, 3, 2, 6
    vec = VecImageEnv(narrow_cfg(R, P), env_num=E, seed=9, auto_reset=False, rollout=T, rollout_final=64, minibatch=16)
    try:
        w = vec.world
        acts = fixed_actions(T, E * R)
        x = torch.ones((T, E * R), device="cuda")
        step = iter(torch.as_tensor(a, device="cuda") for a in acts)

        def all_stale():
            for call in (lambda: w.rollout_shuffle(1), lambda: w.rollout_stats(x), lambda: w.rollout_minibatch(0, 0, [x])):
                with pytest.raises(RuntimeError, match=STALE):
                    call()

        def all_work():
            w.rollout_index()
            w.rollout_stats(x)
            w.rollout_shuffle(1)
            w.rollout_minibatch(0, 0, [x])
        with pytest.raises(RuntimeError, match="imgenv_rollout_begin"):
            w.rollout_index()  # before the first window
        vec.reset()
        with pytest.raises(RuntimeError, match="no transition"):
            w.rollout_index()
        with pytest.raises(RuntimeError, match="before imgenv_rollout_index"):
            w.rollout_shuffle(1)
        vec.step(next(step))
        vec.step(next(step))
        w.rollout_index()
        with pytest.raises(RuntimeError, match="before imgenv_rollout_shuffle"):
            w.rollout_minibatch(0, 0, [x])
        all_work()
        before = host(w.minibatch)
        vec.step(next(step))
        all_stale()
        after = host(w.minibatch)
        for f in before:  # nothing was queued
            assert before[f].tobytes() == after[f].tobytes(), f
        all_work()
        vec.reset_envs([0])
        all_stale()
        all_work()
        vec.rollout_begin()
        all_stale()
        with pytest.raises(RuntimeError, match="no transition"):
            w.rollout_index()
        vec.step(next(step))
        all_work()
        assert w.rollout_valid_count() == int(host(w.rollout)["is_clean"][:1].astype(bool).sum())
    finally:
        vec.close()


# ---- 7. the feature disturbs nothing ----
def test_the_feature_disturbs_nothing():
    """twin handles with and without minibatch=B through 6 auto-reset steps: every output byte and every chain's launch count equal;
    the ring is byte-equal after an epoch of gathers"""
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T, B = 5, 3, 2, 6, 32
    cfg = narrow_cfg(R, P)
    acts = fixed_actions(T, E * R)
    off, on = (VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=True, device_reset=True, rollout=T, minibatch=b) for b in (0, B))
    try:
        assert off.world.minibatch is None and off.minibatch_batch == 0 and on.world.minibatch is not None
        with pytest.raises(RuntimeError, match="minibatch=B"):
            off.rollout_minibatches({}, 1)
        with pytest.raises(ValueError, match="rollout=T"):
            VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, minibatch=B)
        off.reset(), on.reset()
        assert on.world.launches() == off.world.launches()
        for s in range(T):
            a = torch.as_tensor(acts[s], device="cuda")
            off.step(a), on.step(a)
            sa, sb = off.world.snapshot(), on.world.snapshot()
            assert set(sa) == set(sb)
            for f in sa:
                assert sa[f].tobytes() == sb[f].tobytes(), (s, f)
            assert on.world.launches() == off.world.launches(), s
        ring_off, ring_on = host(off.world.rollout), host(on.world.rollout)
        launches = on.world.launches()
        adv = torch.randn((T, E * R), device="cuda")
        n = sum(1 for _ in on.rollout_minibatches({"adv": adv}, 5, normalise="adv"))
        assert n == -(-T * E * R // B) and on.world.launches() == launches  # (the chain's count is the chain's)
        ring_after = host(on.world.rollout)
        for f in ring_off:
            assert ring_off[f].tobytes() == ring_on[f].tobytes() == ring_after[f].tobytes(), f
        assert on.world.rollout_cursor() == off.world.rollout_cursor()
    finally:
        off.close()
        on.close()


# ---- 8. nothing needs the host ----
def test_index_and_gathers_queued_behind_a_busy_stream_equal_a_synchronised_twin():
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T, B = 5, 3, 2, 6, 32
    acts = fixed_actions(T, E * R)
    runs = []
    for synchronised in (False, True):
        vec = VecImageEnv(narrow_cfg(R, P), env_num=E, seed=9, device_reset=True, rollout=T, rollout_final=64, minibatch=B, minibatch_buffers=2)
        try:
            vec.reset()
            a = [torch.as_tensor(acts[t], device="cuda") for t in range(T)]
            adv = torch.arange(T * E * R, dtype=torch.float32, device="cuda").view(T, E * R)
            torch.cuda.synchronize()
            if not synchronised:  # some tens of milliseconds of work in front of the steps on their stream
                x = torch.full((4096, 4096), 1e-4, device="cuda")
                for _ in range(24):
                    x = x @ x
            for t in range(T):
                vec.step(a[t])
                if synchronised:
                    torch.cuda.synchronize()
            kept = []
            for mb in vec.rollout_minibatches({"adv": adv}, 11, normalise="adv"):
                kept.append({k: v.clone() for k, v in mb.items()})  # (stream-ordered copies: the buffers alternate)
                if synchronised:
                    torch.cuda.synchronize()
            kept.append({k: vec.world.minibatch[k].clone() for k in ("valid", "valid_n", "order", "norm")})
            runs.append([host(m) for m in kept])
        finally:
            vec.close()
    assert len(runs[0]) == len(runs[1]) == -(-T * E * R // B) + 1
    assert int(runs[0][-1]["valid_n"][0]) > 0
    for m0, m1 in zip(*runs):
        assert set(m0) == set(m1)
        for f in m0:
            assert m0[f].tobytes() == m1[f].tobytes(), f


# ---- 9. the enable call on a live handle ----
def test_enable_needs_the_rollout_and_reports_every_pointer():
    from img_env_amd import _cabi
    from img_env_amd.world import World
    grid, params, layout = small_world(6, 3, seed=4)
    w = World(params, grid)
    try:
        o = _cabi.MinibatchOut()
        assert w.lib.imgenv_rollout_minibatch_outputs(w.h, C.byref(o)) == _cabi.ESTATE
        assert w.lib.imgenv_rollout_index(w.h, None) == _cabi.ESTATE
        with pytest.raises(RuntimeError, match="imgenv_rollout_enable"):
            w.enable_minibatch(8)
        with pytest.raises(RuntimeError, match="enable_minibatch"):
            w.rollout_index()
        assert w.minibatch is None
        w.enable_rollout(4, 4, ["vector_states", "lasers"])
        with pytest.raises(ValueError, match="rollout stores"):
            w.enable_minibatch(8, 1, ["sensor_maps"])
        launches = w.launches()
        mb = w.enable_minibatch(8, 3, None)  # 0: every field of the rollout
        assert w.launches() == launches
        assert {k for k in mb if k.startswith("mb_")} == {"mb_vector_states", "mb_lasers"} | set(_cabi.MB_SCALARS)
        assert mb["mb_lasers"].shape == (3, 8) + tuple(w.out["lasers"].shape[1:]) and mb["mb_lasers"].dtype == w.out["lasers"].dtype
        assert w.lib.imgenv_rollout_minibatch_outputs(w.h, C.byref(o)) == 0
        assert (o.n_local, o.horizon, o.batch, o.buffers, o.fields) == (6, 4, 8, 3, 2 | 4)
        for name in _cabi.MB_ARRAYS:
            assert getattr(o, name) and getattr(o, name) % 256 == 0, name
        for b in range(4):
            for name, _ in _cabi.MinibatchBuffer._fields_:
                ptr = getattr(o.buf[b], name)
                want = b < 3 and name not in ("mb_sensor_maps", "mb_ped_vector_states", "mb_ped_maps", "mb_ped_vector_norm", "mb_stack_sensor_maps",
                                              "mb_stack_vector_states", "mb_stack_lasers")
                assert bool(ptr) == want and (not ptr or ptr % 256 == 0), (b, name)
            if b < 3:
                assert o.buf[b].mb_lasers == mb["mb_lasers"][b].data_ptr() and mb["mb_lasers"][b].is_contiguous()
    finally:
        w.close()
