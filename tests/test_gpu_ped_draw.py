"""Pedestrian maps drawn from pedestrian vectors on the device (imgenv_ped_maps_draw, IMGENV_ROLLOUT_PED_MAPS_DRAWN,
csrc/ped_draw.h).  The oracle is the map k_obs wrote beside the vector, which the existing ``ped_maps`` field stores, and
tests/ped_draw_model.py for rows k_obs never writes.  The kernel moves words and compares float64 values computed in the model's
order: every comparison is bit for bit."""
import copy

import numpy as np
import pytest

import minibatch_model as mm
import ped_draw_model as pdm
from scenarios import small_world
from test_gpu_final_obs import fixed_actions, host, narrow_cfg, same

pytestmark = pytest.mark.gpu


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# (seed 15: of the seeds 0 .. 39 the one whose device-side placements put most pedestrians within 3 m of a robot in these six steps
# -- 32 of the 105 stored maps and 4 of the 15 final ones hold a disc; seed 9, the neighbouring files' choice, shows none)
def steps(vec, acts):
    import torch
    for a in acts:
        vec.step(torch.as_tensor(a, device="cuda"))


# ---- 1. the maps k_obs stored beside the vectors ----
@pytest.mark.parametrize("size", [48, 40, 96])
def test_drawn_from_the_stored_vectors_equals_the_stored_maps(size):
    """5 envs x 3 robots x 2 pedestrians, device_reset, 6 steps with time_max 5: every row of all 7 slots and of the final list.
    48 and 96: cells of 0.125 and 0.0625 m, the ped_inv_res form; 40: 0.15 m, the floor division."""
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T = 5, 3, 2, 6
    vec = VecImageEnv(narrow_cfg(R, P, max_ped=10, ped_image_size=[size, size]), env_num=E, seed=15, device_reset=True, rollout=T,
                      rollout_fields=["ped_vector_states", "ped_maps"])
    try:
        w = vec.world
        vec.reset()
        steps(vec, fixed_actions(T, E * R))
        ring = w.rollout
        PV = ring["obs_ped_vector_states"].shape[-1]
        assert PV == 71 and tuple(ring["obs_ped_maps"].shape) == (T + 1, E * R, 3, size, size)
        drawn = w.draw_ped_maps(ring["obs_ped_vector_states"].view(-1, PV))
        drawn_final = w.draw_ped_maps(ring["final_ped_vector_states"])
        got = host({"obs": drawn, "final": drawn_final})
        kept = host(ring)
        assert got["obs"].shape == ((T + 1) * E * R, 3, size, size)
        same(got["obs"], kept["obs_ped_maps"].reshape(got["obs"].shape), "slots")
        same(got["final"], kept["final_ped_maps"], "final list")
        n_final = int(kept["final_n"][vec.rollout()["resets"] & 1])
        filled = int(words(kept["obs_ped_maps"]).reshape(len(got["obs"]), -1).any(axis=1).sum())
        print("size", size, "maps with a pedestrian:", filled, "of", len(got["obs"]), "final entries:", n_final)
        assert filled > 0 and n_final > 0 and words(kept["final_ped_maps"][:n_final]).any()
    finally:
        vec.close()


# ---- 2. synthetic rows against the model ----
@pytest.mark.parametrize("size", [48, 40])
def test_synthetic_rows_equal_the_model(size):
    """PV = 1 + 7 * 80: 80 pedestrians in one row are more than one wavefront's 64 lanes (test_rows_of_300_pedestrians has more than
    the workgroup's 256).  The rows are
    ped_draw_model.synthetic_rows: no pedestrian, one disc, discs cut by every edge and corner, positions at exactly +-3 and one
    float32 beyond, overlapping discs in both rank orders, 80 on a few cells, counts above the cap / negative / not finite /
    fractional, positions that are not finite, -0.0f and NaN velocities.  Then index lists with -1 and repeats: one map, 300, and
    more than two passes of a full grid."""
    import torch
    from img_env_amd import _cabi
    from img_env_amd.world import World
    grid, params, _ = small_world(3, 2, seed=4, max_ped=80, ped_image_size=(size, size))
    w = World(params, grid)
    try:
        vectors, names = pdm.synthetic_rows(1 + 7 * 80)
        geo = pdm.geometry(size, size, params["ped_image_r"])
        want = pdm.draw(vectors, geo)
        dev = torch.as_tensor(vectors, device="cuda")
        launches = w.launches()
        got = host({"m": w.draw_ped_maps(dev)})["m"]
        for i, name in enumerate(names):
            same(got[i], want[i], name)
        assert words(want).any()
        for n in (1, 300, 2 * _cabi.PED_DRAW_MAX_BLOCKS + 5):
            rows = pdm.synthetic_index(len(vectors), n, seed=n)
            out = torch.full((n, 3, size, size), float("nan"), device="cuda")  # (every cell is written)
            assert w.draw_ped_maps(dev, torch.as_tensor(rows, device="cuda"), out) is out
            same(host({"m": out})["m"], pdm.draw(vectors, geo, rows), "%d indexed rows" % n)
        import ctypes as C
        assert w.draw_ped_maps(dev[:0]).shape == (0, 3, size, size)
        before = out.clone()
        assert w.lib.imgenv_ped_maps_draw(w.h, C.c_void_p(dev.data_ptr()), None, 0, C.c_void_p(out.data_ptr()), None) == 0  # n == 0: nothing is launched
        assert w.lib.imgenv_ped_maps_draw(w.h, C.c_void_p(dev.data_ptr()), None, -1, C.c_void_p(out.data_ptr()), None) == _cabi.EINVAL
        assert w.lib.imgenv_ped_maps_draw(w.h, None, None, 1, C.c_void_p(out.data_ptr()), None) == _cabi.EINVAL
        assert w.lib.imgenv_ped_maps_draw(w.h, C.c_void_p(dev.data_ptr()), None, 1, None, None) == _cabi.EINVAL
        assert torch.equal(before.view(torch.int32), out.view(torch.int32))
        assert w.launches() == launches  # (the chain's count is the chain's)
        for bad in (dev[:, :-1], dev.double(), dev.cpu(), dev.t()):
            with pytest.raises(ValueError, match="ped_vectors"):
                w.draw_ped_maps(bad)
        with pytest.raises(ValueError, match="rows"):
            w.draw_ped_maps(dev, torch.zeros(4, dtype=torch.int64, device="cuda"))
        with pytest.raises(ValueError, match="out"):
            w.draw_ped_maps(dev, None, torch.zeros((len(vectors), 3, size, size + 1), device="cuda"))
    finally:
        w.close()


def test_rows_of_300_pedestrians_take_further_rounds_of_the_lanes():
    """PV = 1 + 7 * 300: k_ped_draw's 256 lanes take a pedestrian each, so pedestrians 256 .. 299 are a second round.  300 spread and
    300 piled, counts of 256 and 257, and a row whose only pedestrian inside the box is the 300th (and the same row counted to 299:
    all zeros), in both floor forms."""
    import torch
    from img_env_amd import _cabi
    from img_env_amd.world import World
    assert _cabi.PED_DRAW_BLOCK == 256
    vectors, names = pdm.crowded_rows(1 + 7 * 300)
    for size in (48, 40):
        grid, params, _ = small_world(3, 2, seed=4, max_ped=300, ped_image_size=(size, size))
        w = World(params, grid)
        try:
            geo = pdm.geometry(size, size, params["ped_image_r"])
            want = pdm.draw(vectors, geo)
            got = host({"m": w.draw_ped_maps(torch.as_tensor(vectors, device="cuda"))})["m"]
            for i, name in enumerate(names):
                same(got[i], want[i], "%d: %s" % (size, name))
            assert words(want[names.index("the 300th alone in the box")]).any() and not words(want[names.index("the 300th not counted")]).any()
        finally:
            w.close()


# ---- 3. twin handles: one stores the maps, one draws them ----
def test_twin_minibatches_and_the_smaller_ring():
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T, B = 5, 3, 2, 6, 32
    cfg = narrow_cfg(R, P, max_ped=10)
    acts = fixed_actions(T, E * R)
    stored, drawn = (VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=15, device_reset=True, rollout=T, rollout_final=64, minibatch=B, minibatch_buffers=2,
                                 rollout_draw_ped_maps=d) for d in (False, True))
    try:
        ws, wd = stored.world, drawn.world
        Hp, Wp = ws.rollout["obs_ped_maps"].shape[-2:]
        assert set(ws.rollout) - set(wd.rollout) == {"obs_ped_maps", "final_ped_maps"} and set(wd.rollout) <= set(ws.rollout)
        assert "obs_ped_vector_states" in wd.rollout and wd.rollout_draws_ped_maps and not ws.rollout_draws_ped_maps
        nbytes = [sum(t.numel() * t.element_size() for t in w.rollout.values()) for w in (ws, wd)]
        assert nbytes[0] - nbytes[1] == ((T + 1) * E * R + 64) * 3 * Hp * Wp * 4
        assert set(ws.minibatch) == set(wd.minibatch) and "mb_ped_maps" in wd.minibatch
        assert wd.minibatch["mb_ped_maps"].shape == ws.minibatch["mb_ped_maps"].shape == (2, B, 3, Hp, Wp)
        for vec in (stored, drawn):
            vec.reset()
            steps(vec, acts)
        ring_s, ring_d = host(ws.rollout), host(wd.rollout)
        for f in ring_d:
            same(ring_d[f], ring_s[f], "ring " + f)
        adv = torch.randn((T, E * R), generator=torch.Generator().manual_seed(1)).cuda()
        epochs = []
        for w in (ws, wd):
            w.rollout_index()
            w.rollout_stats(adv)
            w.rollout_shuffle(11)
            epochs.append([host(w.rollout_minibatch(j, j % 2, [adv], normalise=0)) for j in range(4)])  # (the fourth lies behind T R)
        V = ws.rollout_valid_count()
        assert 0 < V == wd.rollout_valid_count() < 3 * B
        for j, (ms, md) in enumerate(zip(*epochs)):
            assert set(ms) == set(md)
            for f in ms:
                same(md[f], ms[f], "minibatch %d %s" % (j, f))
        assert words(epochs[1][0]["mb_ped_maps"]).any()
        assert not epochs[1][3]["mb_weight"].any() and not words(epochs[1][3]["mb_ped_maps"]).any()  # all slots behind the valid list
        tail = epochs[1][2]["mb_weight"] == 0
        assert tail.any() and not words(epochs[1][2]["mb_ped_maps"][tail]).any()  # weight-0 slots of a mixed minibatch
        # through the vectorised env's epoch as well
        for ms, md in zip(*[[host(mb) for mb in vec.rollout_minibatches({"adv": adv}, 5, normalise="adv")] for vec in (stored, drawn)]):
            for f in ms:
                same(md[f], ms[f], "epoch " + f)
        # what a trainer needs for the value of the window's last state and of the time-outs
        maps = host({str(t): drawn.rollout_ped_maps(t) for t in range(T + 1)})
        for t in range(T + 1):
            same(maps[str(t)], ring_s["obs_ped_maps"][t], "slot %d" % t)
        same(host({"f": drawn.rollout_final_ped_maps()})["f"], ring_s["final_ped_maps"], "final list")
        with pytest.raises(ValueError):
            drawn.rollout_ped_maps(T + 1)
        with pytest.raises(RuntimeError, match="rollout_draw_ped_maps"):
            stored.rollout_ped_maps(0)
        ring_after = host(wd.rollout)
        for f in ring_d:  # (drawing reads the ring)
            assert ring_after[f].tobytes() == ring_d[f].tobytes(), f
    finally:
        stored.close()
        drawn.close()


# ---- 4. a draw that strides over its grid's share of a minibatch: 256 slots; valid_n < B and valid_n == 0 ----
def test_ped_maps_at_256_slots_drawn_and_a_window_of_frozen_robots_is_all_zero():
    """test_gpu_minibatch.py's striding case with the maps drawn: the minibatch selects ``ped_maps_drawn`` alone -- no field is copied,
    the gather writes the scalars only.  Windows of 3 steps, auto_reset=False, time_max 5: the third window holds frozen robots
    only, valid_n = 0, the order is all -1 and every drawn map is zero."""
    import torch
    from img_env_amd import _cabi
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T, B = 5, 3, 2, 3, 256
    stored, drawn = (VecImageEnv(narrow_cfg(R, P), env_num=E, seed=9, auto_reset=False, rollout=T, rollout_final=8, rollout_draw_ped_maps=d)
                     for d in (False, True))
    try:
        ws, wd = stored.world, drawn.world
        with pytest.raises(ValueError, match="rollout stores"):
            wd.enable_minibatch(B, 1, ["ped_maps"])
        with pytest.raises(ValueError, match="rollout stores"):
            ws.enable_minibatch(B, 1, ["ped_maps_drawn"])
        views = wd.enable_minibatch(B, 1, ["ped_maps_drawn"])
        ws.enable_minibatch(B, 1, ["ped_maps"])
        assert {k for k in views if k.startswith("mb_")} == {"mb_ped_maps"} | set(_cabi.MB_SCALARS)
        acts = fixed_actions(3 * T, E * R)
        x = torch.ones((T, E * R), device="cuda")
        for vec in (stored, drawn):
            vec.reset()
        for window in range(3):
            for vec in (stored, drawn):
                if window:
                    vec.rollout_begin()
                steps(vec, acts[window * T:(window + 1) * T])
            if window == 1:
                continue
            got = []
            for w in (ws, wd):
                w.rollout_index()
                w.rollout_stats(x, 0.0)
                w.rollout_shuffle(3)
                got.append(host(w.rollout_minibatch(0, 0, [x], normalise=0)))
            ring = host(ws.rollout)
            V = len(mm.valid_list(ring["is_clean"], T))
            order = host({"order": wd.minibatch["order"]})["order"]
            print("window", window, "valid_n", V)
            assert V == wd.rollout_valid_count() < B
            for f in got[0]:
                same(got[1][f], got[0][f], "window %d %s" % (window, f))
            flat = ring["obs_ped_maps"].reshape((-1,) + ring["obs_ped_maps"].shape[2:])
            for i in range(B):  # and against the ring itself
                k = int(order[i]) if i < len(order) else -1
                same(got[1]["mb_ped_maps"][i], flat[k] if k >= 0 else np.zeros_like(flat[0]), "slot %d" % i)
            assert not words(got[1]["mb_ped_maps"][V:]).any()
            if window == 0:
                assert V > 0 and words(got[1]["mb_ped_maps"][:V]).any()
            else:
                assert V == 0 and (order == -1).all() and not got[1]["mb_weight"].any() and (got[1]["mb_index"] == -1).all()
    finally:
        stored.close()
        drawn.close()


# ---- 5. refusals and neutrality ----
def test_refused_combinations_leave_the_handle_usable():
    import torch
    from img_env_amd.world import World
    grid, params, layout = small_world(4, 2, seed=4)
    w = World(params, grid)
    try:
        with pytest.raises(ValueError, match="excludes IMGENV_ROLLOUT_PED_MAPS"):
            w.enable_rollout(4, 4, ["ped_vector_states", "ped_maps", "ped_maps_drawn"])
        assert w.rollout is None
        with pytest.raises(ValueError, match="needs IMGENV_ROLLOUT_PED_VECTOR_STATES"):
            w.enable_rollout(4, 4, ["sensor_maps", "ped_maps_drawn"])
        with pytest.raises(ValueError, match="fields 512"):
            w.enable_rollout(4, 4, ["ped_maps_drawn"])
        assert w.rollout is None and not w.rollout_draws_ped_maps
        ring = w.enable_rollout(4, 4, ["ped_vector_states", "ped_maps_drawn"])
        assert set(k for k in ring if k.startswith(("obs_", "final_")) and k != "final_idx" and k != "final_slot" and k != "final_row" and k != "final_n") == \
            {"obs_ped_vector_states", "final_ped_vector_states"}
        with pytest.raises(ValueError, match="already"):
            w.enable_rollout(4, 4, ["ped_vector_states", "ped_maps"])
        mb = w.enable_minibatch(8, 1, None)  # 0: all of the rollout's -- the vector, and the maps drawn from it
        assert "mb_ped_maps" in mb and "mb_ped_vector_states" in mb
        w.reset(layout)
        w.rollout_begin()
        w.step(np.zeros((4, 3), np.float32))
        live = host({k: w.out[k] for k in ("ped_vector_states", "ped_maps")})
        same(host({"m": w.draw_ped_maps(w.out["ped_vector_states"])})["m"], live["ped_maps"], "the live observation")
        same(host({"m": w.draw_ped_maps(w.rollout["obs_ped_vector_states"][1])})["m"], live["ped_maps"], "slot 1")
        w.rollout_index()
        w.rollout_shuffle(1)
        got = host(w.rollout_minibatch(0, 0))
        for i, k in enumerate(got["mb_index"]):
            same(got["mb_ped_maps"][i], live["ped_maps"][k] if k >= 0 else np.zeros_like(live["ped_maps"][0]), "slot %d" % i)
        assert (got["mb_index"] >= 0).sum() == 4
    finally:
        w.close()
    grid, params, layout = small_world(3, 0, seed=4)
    w = World(params, grid)
    try:
        vectors = torch.zeros((3, w.out["ped_vector_states"].shape[1]), device="cuda")
        with pytest.raises(ValueError, match="without pedestrians"):
            w.draw_ped_maps(vectors)
        w.reset(layout)  # (still usable)
        w.step(np.zeros((3, 3), np.float32))
    finally:
        w.close()


def test_the_feature_disturbs_nothing():
    """four handles through a reset and 5 auto-reset steps: a plain one and one whose caller draws maps between the steps; one that
    stores ped_maps and one that draws them.  Within each pair every output byte and every chain's launch count are equal --
    k_rollout does not see the bit, a draw is no launch of a chain -- and the pairs differ by the rollout's one launch per chain."""
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T = 5, 3, 2, 5
    cfg = narrow_cfg(R, P, max_ped=10)
    acts = fixed_actions(T, E * R)
    kinds = [dict(), dict(), dict(rollout=T), dict(rollout=T, rollout_draw_ped_maps=True)]
    vecs = [VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=True, device_reset=True, **k) for k in kinds]
    try:
        with pytest.raises(ValueError, match="rollout=T"):
            VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, rollout_draw_ped_maps=True)
        for vec in vecs:
            vec.reset()
        base = [vec.world.launches() for vec in vecs]
        assert base[0] == base[1] and base[2] == base[3]
        for s in range(T):
            a = torch.as_tensor(acts[s], device="cuda")
            for vec in vecs:
                vec.step(a)
            vecs[1].world.draw_ped_maps(vecs[1].world.out["ped_vector_states"])
            vecs[3].rollout_ped_maps(s + 1)
            snaps = [vec.world.snapshot() for vec in vecs]
            for other in snaps[1:]:
                assert set(other) == set(snaps[0])
                for f in other:
                    assert other[f].tobytes() == snaps[0][f].tobytes(), (s, f)
            n = [vec.world.launches() for vec in vecs]
            assert n[0] == n[1] and n[2] == n[3], (s, n)
    finally:
        for vec in vecs:
            vec.close()


def test_draws_queued_behind_a_busy_stream_equal_a_synchronised_twin():
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T, B = 5, 3, 2, 6, 32
    acts = fixed_actions(T, E * R)
    runs = []
    for synchronised in (False, True):
        vec = VecImageEnv(narrow_cfg(R, P, max_ped=10), env_num=E, seed=15, device_reset=True, rollout=T, rollout_final=64, minibatch=B, minibatch_buffers=2,
                          rollout_draw_ped_maps=True)
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
            kept = [{"last": vec.rollout_ped_maps(T), "final": vec.rollout_final_ped_maps()}]
            for mb in vec.rollout_minibatches({"adv": adv}, 11, normalise="adv"):
                kept.append({k: v.clone() for k, v in mb.items()})  # (stream-ordered copies: the buffers alternate)
                if synchronised:
                    torch.cuda.synchronize()
            runs.append([host(m) for m in kept])
        finally:
            vec.close()
    assert len(runs[0]) == len(runs[1]) == -(-T * E * R // B) + 1
    assert words(runs[0][1]["mb_ped_maps"]).any()
    for m0, m1 in zip(*runs):
        assert set(m0) == set(m1)
        for f in m0:
            assert m0[f].tobytes() == m1[f].tobytes(), f
