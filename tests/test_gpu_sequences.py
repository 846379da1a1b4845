"""The sequence minibatches on the device (imgenv_rollout_seq_enable, imgenv_rollout_seq_index / _seq_shuffle / _seq_minibatch,
csrc/sequences.h) against tests/seq_model.py.  Everything moves integers and bytes, the normalisation is two float32 roundings:
every comparison is exact.  Shapes and helpers are tests/test_gpu_minibatch.py's."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import seq_model as sm
from scenarios import small_world
from test_gpu_episodes import episode_cfg
from test_gpu_final_obs import TABLE8, WRAPPERS, fixed_actions, host, narrow_cfg, same

pytestmark = pytest.mark.gpu
STALE = "rollout changed since imgenv_rollout_seq_index"
RING_SCALARS = ("actions", "rewards", "dones", "dones_info")
SEEDS = (0x0123456789ABCDEF, 7)
NORM = np.array([0.25, 2.0], np.float32)


def obs_fields(ring):
    return {k[4:]: v for k, v in ring.items() if k.startswith("obs_")}


def model_minibatch(ring, order, j, Bs, L, n, R, fields, scalars=(), normalise=None, norm=None, states=()):
    return sm.gather(order, j, Bs, L, n, R, {f: ring["obs_" + f] for f in fields}, {k: ring[k] for k in RING_SCALARS}, ring["is_clean"],
                     ring["final_idx"], scalars, normalise, norm, states)


def compare_minibatch(got, want, n_scalars, where):
    assert set(want) <= set(got), (where, set(want) - set(got))
    for name, w in want.items():
        g = got[name][:n_scalars] if name == "mb_scalars" else got[name]
        same(g, w, "%s: %s" % (where, name))


def caller_arrays(T, R, seed):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    scalars = [torch.randn((T, R), generator=g).cuda(), torch.randn((T, R), generator=g).cuda(), torch.randn((T + 1, R), generator=g).cuda()]
    states = [torch.randn((T + 1, R, 8), generator=g).cuda(), torch.randn((T + 1, R, 8), generator=g).cuda()]
    return scalars, states


# ---- 1. 6 rows x 15 steps, L = 4: the last chunk has 3 steps; device_reset, stacks and wrappers on ----
@functools.lru_cache(maxsize=None)
def case15():
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T, L, Bs = 3, 2, 2, 15, 4, 4
    cfg = narrow_cfg(R, P, max_ped=10, wrappers=WRAPPERS, discrete_action=True, discrete_actions=TABLE8, image_batch=2, state_batch=3, laser_batch=2)
    acts = np.random.default_rng(3).integers(0, len(TABLE8), (T, E * R)).astype(np.int64)
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=True, device_reset=True, stack=True, wrappers=True, rollout=T,
                      rollout_final=128, sequences=dict(length=L, batch=Bs, buffers=2, state_bytes=(32, 32)))
    try:
        w = vec.world
        assert w.minibatch is None  # the sequences do not need the minibatches
        rec = {"shapes": {k: (tuple(v.shape), str(v.dtype), v.data_ptr()) for k, v in w.sequences.items()},
               "ring_shapes": {k: (tuple(v.shape), str(v.dtype)) for k, v in w.rollout.items()}, "all_down": []}
        vec.reset()
        for t in range(T):
            _, _, _, info = vec.step(acts[t])
            rec["all_down"].append(info["all_down"].cpu().numpy().copy())
        # the window must hold a sequence with no clean step, one with an unclean step inside and an mb_first in mid-chunk: the time
        # limit of 5 steps gives the last (every reset lands on t = 5 or 10, l = 1 or 2); the first two are written where the seed's
        # robots stayed clean
        clean = w.rollout["is_clean"]
        clean[0:4, 0] = 0   # q = 0: wholly unclean
        clean[4, 1] = 1     # q = 7 (c = 1, row 1): t = 4 counts, t = 5 does not
        clean[5, 1] = 0
        rec["ring"] = host(w.rollout)
        w.rollout_seq_index()
        rec["count"] = w.rollout_seq_count()
        rec["index"] = host({k: w.sequences[k] for k in ("seq_flag", "seq_valid", "seq_valid_n")})
        sc, st = caller_arrays(T, E * R, 5)
        norm = torch.tensor(NORM, device="cuda")
        rec["scalars"], rec["states"] = [s.cpu().numpy() for s in sc], [s.cpu().numpy() for s in st]
        rec["orders"], rec["mbs"] = [], []
        for seed in SEEDS:
            w.rollout_seq_shuffle(seed)
            rec["orders"].append(host({"o": w.sequences["seq_order"]})["o"])
        for j in range(7):  # six minibatches cover the 24 sequences; the seventh lies behind C_max R
            rec["mbs"].append(host(w.rollout_seq_minibatch(j, j % 2, sc, normalise=0, norm=norm, states=st)))
        names = dict(zip(("adv", "logp", "values"), sc))
        rec["epoch"] = [host(mb) for mb in vec.rollout_sequences(names, SEEDS[0], states=st)]
        rec["rows"] = {k: tuple(v.shape) for k, v in vec.sequence_rows(next(iter(vec.rollout_sequences(names, SEEDS[0], states=st)))).items()}
        rec["ring_after"] = host(w.rollout)
        with pytest.raises(ValueError, match="minibatch >= 1"):
            vec.rollout_sequences(names, 1, states=st, normalise="adv")
        with pytest.raises(ValueError):
            w.rollout_seq_minibatch(0, 0, [sc[0][:-1]], states=st)
        with pytest.raises(ValueError):
            w.rollout_seq_minibatch(0, 2, sc, states=st)  # buffer 2 of 2
        with pytest.raises(ValueError, match="norm"):
            w.rollout_seq_minibatch(0, 0, sc, normalise=0, states=st)  # no norm
        with pytest.raises(ValueError, match="state arrays"):
            w.rollout_seq_minibatch(0, 0, sc, states=st[:1])
        with pytest.raises(ValueError, match="32 bytes"):
            w.rollout_seq_minibatch(0, 0, sc, states=[st[0], st[1][:, :, :4].contiguous()])
        with pytest.raises(ValueError, match="aligned"):
            off = torch.zeros((T + 1) * E * R * 8 + 1, device="cuda")[1:].view(T + 1, E * R, 8)
            w.rollout_seq_minibatch(0, 0, sc, states=[st[0], off])
    finally:
        vec.close()
    return rec, (E, R, T, L, Bs)


def test_flags_index_and_order_equal_the_model():
    rec, (E, R, T, L, Bs) = case15()
    RR, S = E * R, -(-T // L) * E * R
    assert S == 24 and T % L == 3
    ring = rec["ring"]
    flags = sm.flags(ring["is_clean"], T, L)
    same(rec["index"]["seq_flag"], flags, "seq_flag")
    valid = sm.valid_list(ring["is_clean"], T, L)
    Vs = len(valid)
    print("seq_valid_n", Vs, "of", S)
    assert int(rec["index"]["seq_valid_n"][0]) == Vs == rec["count"] and 0 < Vs < S
    same(rec["index"]["seq_valid"][:Vs], valid, "seq_valid")
    for seed, order in zip(SEEDS, rec["orders"]):
        same(order, sm.order_list(valid, S, seed), "seq_order under seed %x" % seed)
    assert (rec["orders"][0] != rec["orders"][1]).any()
    sh = rec["shapes"]
    assert sh["seq_valid"][:2] == ((S,), "torch.int32") and sh["seq_order"][:2] == ((S,), "torch.int32") and sh["seq_flag"][:2] == ((S,), "torch.uint8")
    assert all(ptr % 256 == 0 for _, _, ptr in sh.values())
    for name, (shape, dtype) in rec["ring_shapes"].items():  # [buffers, L, Bs, row...] with the ring's row shapes and types
        if name.startswith("obs_"):
            assert sh["mb_" + name[4:]][:2] == ((2, L, Bs) + shape[2:], dtype), name
    assert sh["mb_scalars"][0] == (2, 6, L, Bs) and sh["mb_actions"][0] == (2, L, Bs, 3) and sh["mb_first"][:2] == ((2, L, Bs), "torch.uint8")
    assert sh["mb_seq"][:2] == ((2, Bs), "torch.int32") and sh["mb_seq_state0"][:2] == ((2, Bs, 32), "torch.uint8") and "mb_seq_state1" in sh
    # the device-side reset: slot t + 1 of a row was rewritten exactly where all_down was set after step t
    for t in range(T - 1):
        same(ring["final_idx"][t + 1] >= 0, rec["all_down"][t].astype(bool), "final_idx of slot %d" % (t + 1))
    assert np.any(ring["final_idx"][1:T] >= 0)
    assert RR == 6


def test_every_sequence_minibatch_equals_the_model():
    rec, (E, R, T, L, Bs) = case15()
    RR, S = E * R, -(-T // L) * E * R
    ring, order = rec["ring"], rec["orders"][1]  # (the last shuffle: SEEDS[1])
    fields = list(obs_fields(ring))
    assert set(fields) == {"stack_sensor_maps", "stack_vector_states", "stack_lasers", "ped_vector_norm", "ped_maps"}
    Vs = int(rec["index"]["seq_valid_n"][0])
    for j, got in enumerate(rec["mbs"]):
        want = model_minibatch(ring, order, j, Bs, L, T, RR, fields, rec["scalars"], 0, NORM, rec["states"])
        compare_minibatch(got, want, 3, "sequence minibatch %d" % j)
        assert set(got) == set(want), set(got) ^ set(want)
    # the window holds all three: a sequence with no clean step, one with an unclean step inside, an mb_first in mid-chunk
    flags = rec["index"]["seq_flag"]
    assert (flags == 0).any(), "no sequence without a clean step"
    seen = [m for m in rec["mbs"]]
    inside = any(((m["mb_index"] >= 0) & (m["mb_weight"] == 0)).any() for m in seen)
    assert inside, "no gathered sequence with an unclean step inside"
    assert any(m["mb_first"][1:].any() for m in seen), "no mb_first in mid-chunk"
    # mb_first against all_down of the step before
    for m in seen:
        k = m["mb_index"]
        t, row = k // RR, k % RR
        for l, i in zip(*np.nonzero(k >= 0)):
            want = bool(rec["all_down"][t[l, i] - 1][row[l, i]]) if t[l, i] > 0 else False
            assert bool(m["mb_first"][l, i]) == want, (l, i, k[l, i])
    # the last chunk has three steps; slots behind the valid list and the minibatch behind C_max R are empty
    short = [(m["mb_seq"][i], m["mb_seq_len"][i]) for m in seen for i in range(Bs) if m["mb_seq"][i] >= (T // L) * RR]
    assert short and all(n == 3 for _, n in short)
    gathered = np.concatenate([m["mb_seq"] for m in seen])
    assert sorted(gathered[gathered >= 0].tolist()) == rec["index"]["seq_valid"][:Vs].tolist()  # every sequence that counts, once
    last = seen[6]
    assert (last["mb_seq"] == -1).all() and (last["mb_index"] == -1).all() and not last["mb_weight"].any() and not last["mb_seq_state0"].any()
    assert not last["mb_ped_maps"].any() and not last["mb_seq_len"].any()


def test_an_epoch_through_the_vectorised_env_and_the_ring_stays():
    rec, (E, R, T, L, Bs) = case15()
    RR, S = E * R, -(-T // L) * E * R
    ring = rec["ring"]
    order = sm.order_list(sm.valid_list(ring["is_clean"], T, L), S, SEEDS[0])
    assert len(rec["epoch"]) == -(-S // Bs) == 6
    for j, got in enumerate(rec["epoch"]):
        want = model_minibatch(ring, order, j, Bs, L, T, RR, list(obs_fields(ring)), rec["scalars"], None, None, rec["states"])
        sc = want.pop("mb_scalars")
        assert "mb_scalars" not in got
        for s, name in enumerate(("adv", "logp", "values")):
            same(got[name], sc[s], "epoch minibatch %d: %s" % (j, name))
        compare_minibatch(got, want, 0, "epoch minibatch %d" % j)
    for f in ring:
        assert ring[f].tobytes() == rec["ring_after"][f].tobytes(), f
    rows = rec["rows"]
    assert rows["adv"] == (L * Bs,) and rows["mb_actions"] == (L * Bs, 3) and rows["mb_seq"] == (Bs,) and rows["mb_seq_state0"] == (Bs, 32)
    assert rows["mb_ped_maps"][0] == L * Bs and len(rows["mb_ped_maps"]) == 4


# ---- 2. the caller's resets: mb_first for reset_envs in mid-episode and at n = 0 ----
def test_mb_first_marks_a_callers_reset_in_mid_episode_and_at_slot_0():
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T, L = 3, 2, 2, 6, 4
    vec = VecImageEnv(narrow_cfg(R, P), env_num=E, seed=9, auto_reset=False, rollout=T, rollout_final=32, rollout_fields=["vector_states"],
                      sequences=dict(length=L, batch=E * R * 2))
    try:
        w = vec.world
        acts = fixed_actions(T, E * R)
        vec.reset()
        vec.reset_envs([1])          # at n = 0: rows 2, 3 start over at slot 0
        for t in range(3):
            vec.step(torch.as_tensor(acts[t], device="cuda"))
        vec.reset_envs([0])          # in mid-episode: rows 0, 1 start over at slot 3 (l = 3 of chunk 0)
        for t in range(3, T):
            vec.step(torch.as_tensor(acts[t], device="cuda"))
        w.rollout["is_clean"][:] = 1  # (every sequence is gathered)
        ring = host(w.rollout)
        w.rollout_seq_index()
        w.rollout_seq_shuffle(5)
        got = host(w.rollout_seq_minibatch(0))
        assert w.rollout_seq_count() == 2 * E * R
        want = np.zeros((T, E * R), bool)
        want[0, 2:4] = True
        want[3, 0:2] = True
        same(ring["final_idx"][:T] >= 0, want, "final_idx")
        k = got["mb_index"]
        assert (k >= 0).sum() == T * E * R
        first = np.zeros(T * E * R, bool)
        first[k[k >= 0]] = got["mb_first"][k >= 0].astype(bool)
        same(first.reshape(T, E * R), want, "mb_first")
        order = sm.order_list(sm.valid_list(ring["is_clean"], T, L), 2 * E * R, 5)
        compare_minibatch(got, model_minibatch(ring, order, 0, 2 * E * R, L, T, E * R, ["vector_states"]), 0, "minibatch")
    finally:
        vec.close()


# ---- 3. 4800 sequences: two tiles; one small field ----
def test_two_tiles_of_sequences():
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T, L, Bs = 400, 3, 2, 8, 2, 100
    vec = VecImageEnv(narrow_cfg(R, P), env_num=E, seed=9, device_reset=True, rollout=T, rollout_final=64, rollout_fields=["vector_states"],
                      sequences=dict(length=L, batch=Bs, state_bytes=(4,)))
    try:
        w = vec.world
        acts = fixed_actions(T, E * R)
        vec.reset()
        for t in range(T):
            vec.step(torch.as_tensor(acts[t], device="cuda"))
        ring = host(w.rollout)
        S = (T // L) * E * R
        assert S == 4800 > 4096
        w.rollout_seq_index()
        w.rollout_seq_shuffle(SEEDS[1])
        idx = host({k: w.sequences[k] for k in ("seq_flag", "seq_valid", "seq_valid_n", "seq_order")})
        valid = sm.valid_list(ring["is_clean"], T, L)
        Vs = len(valid)
        print("seq_valid_n", Vs, "of", S)
        assert int(idx["seq_valid_n"][0]) == Vs and (valid >= 4096).any()  # (the second tile contributes)
        same(idx["seq_valid"][:Vs], valid, "seq_valid")
        order = sm.order_list(valid, S, SEEDS[1])
        same(idx["seq_order"], order, "seq_order")
        x = torch.arange((T + 1) * E * R, dtype=torch.float32, device="cuda").view(T + 1, E * R)
        for j in (0, 47):
            got = host(w.rollout_seq_minibatch(j, 0, [x], states=[x]))
            want = model_minibatch(ring, order, j, Bs, L, T, E * R, ["vector_states"], [x.cpu().numpy()], None, None, [x.cpu().numpy()])
            compare_minibatch(got, want, 1, "minibatch %d" % j)
    finally:
        vec.close()


# ---- 4. a gather that strides: ped_maps at L = 4, Bs = 64, stored and drawn; 5. Vs < Bs and Vs = 0 ----
def test_ped_maps_stride_stored_and_drawn_and_a_window_of_frozen_robots():
    """5 envs x 3 robots, auto_reset=False, windows of 4 steps, time_max 5.  ped_maps alone is 1728 chunks a row: 4 x 64 steps are
    442 368 chunks, more than ROLLOUT_MAX_BLOCKS x ROLLOUT_BLOCK lanes take in one pass.  The first window has 15 sequences: Vs < Bs.
    By step 5 every robot has timed out, so the third window holds frozen robots only: Vs = 0, the order all -1, the minibatch all zeros."""
    import torch
    from img_env_amd import _cabi
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T, L, Bs = 5, 3, 2, 4, 4, 64
    stored = VecImageEnv(narrow_cfg(R, P), env_num=E, seed=9, auto_reset=False, rollout=T, rollout_final=8, rollout_fields=["ped_maps"],
                         sequences=dict(length=L, batch=Bs))
    drawn = VecImageEnv(narrow_cfg(R, P), env_num=E, seed=9, auto_reset=False, rollout=T, rollout_final=8, rollout_draw_ped_maps=True,
                        rollout_fields=["ped_vector_states", "ped_maps_drawn"], sequences=dict(length=L, batch=Bs))
    try:
        assert stored.world.rollout_draws_ped_maps is False and drawn.world.rollout_draws_ped_maps is True
        assert {k for k in stored.world.sequences if k.startswith("mb_")} == {"mb_ped_maps"} | set(_cabi.SEQ_SCALARS[:-1])
        assert "mb_ped_vector_states" in drawn.world.sequences and "obs_ped_maps" not in drawn.world.rollout
        chunks = int(np.prod(stored.world.sequences["mb_ped_maps"].shape[3:])) * 4 // 16
        assert chunks == 1728 and L * Bs * chunks == 442368 > _cabi.ROLLOUT_MAX_BLOCKS * _cabi.ROLLOUT_BLOCK
        acts = fixed_actions(3 * T, E * R)
        x = torch.ones((T, E * R), device="cuda")
        norm = torch.tensor(NORM, device="cuda")
        stored.reset(), drawn.reset()
        for window in range(3):
            if window:
                stored.rollout_begin(), drawn.rollout_begin()
            for t in range(T):
                a = torch.as_tensor(acts[window * T + t], device="cuda")
                stored.step(a), drawn.step(a)
            if window == 1:
                continue
            got = []
            for vec in (stored, drawn):
                w = vec.world
                w.rollout_seq_index()
                w.rollout_seq_shuffle(3)
                got.append(host(w.rollout_seq_minibatch(0, 0, [x], normalise=0, norm=norm)))
            ring = host(stored.world.rollout)
            idx = host({k: stored.world.sequences[k] for k in ("seq_valid_n", "seq_order")})
            valid = sm.valid_list(ring["is_clean"], T, L)
            Vs = len(valid)
            print("window", window, "seq_valid_n", Vs)
            assert int(idx["seq_valid_n"][0]) == Vs == stored.world.rollout_seq_count() and Vs < Bs
            order = sm.order_list(valid, E * R, 3)
            same(idx["seq_order"], order, "seq_order")
            compare_minibatch(got[0], model_minibatch(ring, order, 0, Bs, L, T, E * R, ["ped_maps"], [x.cpu().numpy()], 0, NORM), 1, "window %d" % window)
            for name in got[0]:  # stored and drawn: equal to each other
                same(got[1][name], got[0][name], "drawn against stored: %s" % name)
            assert not got[0]["mb_ped_maps"][:, Vs:].any() and (got[0]["mb_weight"][:, Vs:] == 0).all()
            if window == 0:
                assert Vs > 0 and got[0]["mb_ped_maps"][:, :Vs].any()
            else:
                assert Vs == 0 and (idx["seq_order"] == -1).all() and not got[0]["mb_weight"].any() and (got[0]["mb_index"] == -1).all()
                assert (got[0]["mb_seq"] == -1).all() and not got[1]["mb_ped_maps"].any()
    finally:
        stored.close()
        drawn.close()


# ---- 6. the stale generation ----
def test_a_chain_behind_the_sequence_index_makes_it_stale():
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T = 5, 3, 2, 6
    vec = VecImageEnv(narrow_cfg(R, P), env_num=E, seed=9, auto_reset=False, rollout=T, rollout_final=64, rollout_fields=["vector_states"],
                      sequences=dict(length=2, batch=16))
    try:
        w = vec.world
        acts = fixed_actions(T, E * R)
        x = torch.ones((T, E * R), device="cuda")
        step = iter(torch.as_tensor(a, device="cuda") for a in acts)

        def all_stale():
            for call in (lambda: w.rollout_seq_shuffle(1), lambda: w.rollout_seq_minibatch(0, 0, [x])):
                with pytest.raises(RuntimeError, match=STALE):
                    call()

        def all_work():
            w.rollout_seq_index()
            w.rollout_seq_shuffle(1)
            w.rollout_seq_minibatch(0, 0, [x])
        with pytest.raises(RuntimeError, match="imgenv_rollout_begin"):
            w.rollout_seq_index()  # before the first window
        vec.reset()
        with pytest.raises(RuntimeError, match="no transition"):
            w.rollout_seq_index()
        with pytest.raises(RuntimeError, match="before imgenv_rollout_seq_index"):
            w.rollout_seq_shuffle(1)
        vec.step(next(step))
        vec.step(next(step))
        w.rollout_seq_index()
        with pytest.raises(RuntimeError, match="before imgenv_rollout_seq_shuffle"):
            w.rollout_seq_minibatch(0, 0, [x])
        all_work()
        before = host(w.sequences)
        vec.step(next(step))
        all_stale()
        after = host(w.sequences)
        for f in before:  # nothing was queued
            assert before[f].tobytes() == after[f].tobytes(), f
        all_work()
        vec.reset_envs([0])
        all_stale()
        all_work()
        vec.rollout_begin()
        all_stale()
        with pytest.raises(RuntimeError, match="no transition"):
            w.rollout_seq_index()
        vec.step(next(step))
        all_work()
        assert w.rollout_seq_count() == int(host(w.rollout)["is_clean"][:1].astype(bool).sum())  # one step: a sequence per transition
    finally:
        vec.close()


# ---- 7. the feature disturbs nothing ----
def test_the_feature_disturbs_nothing():
    """twin handles with and without sequences= through 6 auto-reset steps: every output byte and every chain's launch count equal;
    the ring is byte-equal after an epoch of gathers"""
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T = 5, 3, 2, 6
    cfg = narrow_cfg(R, P)
    acts = fixed_actions(T, E * R)
    off, on = (VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=True, device_reset=True, rollout=T, sequences=s)
               for s in (None, dict(length=4, batch=4)))
    try:
        assert off.world.sequences is None and off.sequences is None and on.world.sequences is not None
        with pytest.raises(RuntimeError, match="sequences="):
            off.rollout_sequences({}, 1)
        with pytest.raises(ValueError, match="rollout=T"):
            VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, sequences=dict(length=4, batch=4))
        with pytest.raises(ValueError, match="sequences:"):
            VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, rollout=T, sequences=dict(length=4))
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
        n = sum(1 for _ in on.rollout_sequences({"adv": adv}, 5))
        assert n == -(-2 * E * R // 4) and on.world.launches() == launches  # (the chain's count is the chain's)
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
    E, R, P, T, L, Bs = 5, 3, 2, 6, 4, 8
    acts = fixed_actions(T, E * R)
    runs = []
    for synchronised in (False, True):
        vec = VecImageEnv(narrow_cfg(R, P), env_num=E, seed=9, device_reset=True, rollout=T, rollout_final=64, minibatch=8,
                          sequences=dict(length=L, batch=Bs, buffers=2, state_bytes=(4,)))
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
            for mb in vec.rollout_sequences({"adv": adv}, 11, states=[adv], normalise="adv"):  # (the statistics are the minibatches')
                kept.append({k: v.clone() for k, v in mb.items()})  # (stream-ordered copies: the buffers alternate)
                if synchronised:
                    torch.cuda.synchronize()
            kept.append({k: vec.world.sequences[k].clone() for k in ("seq_flag", "seq_valid", "seq_valid_n", "seq_order")})
            kept.append({"norm": vec.world.minibatch["norm"].clone()})
            runs.append([host(m) for m in kept])
        finally:
            vec.close()
    assert len(runs[0]) == len(runs[1]) == -(-2 * E * R // Bs) + 2
    assert int(runs[0][-2]["seq_valid_n"][0]) > 0
    adv_seen = np.concatenate([m["adv"][m["mb_index"] >= 0] for m in runs[0][:-2]])
    assert adv_seen.size and abs(float(adv_seen.mean())) < 2.0  # (normalised with the library's statistics)
    for m0, m1 in zip(*runs):
        assert set(m0) == set(m1)
        for f in m0:
            assert m0[f].tobytes() == m1[f].tobytes(), f


# ---- 9. PPO's loss of a flattened sequence minibatch ----
def test_policy_loss_of_sequence_rows_equals_the_loss_of_the_same_rows_as_a_plain_dict():
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T, B, L, Bs = 4, 2, 2, 4, 4, 2, 3
    cfg = episode_cfg(R, P, discrete_action=True, discrete_actions=TABLE8)
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, wrappers=True, rollout=T, minibatch=B, policy=dict(seed=5, loss=True),
                      sequences=dict(length=L, batch=Bs))
    try:
        assert L * Bs > B  # the loss's max_rows is max(B, L Bs)
        torch.manual_seed(0)
        s = vec.reset()
        net = torch.nn.Linear(s.vector_states.shape[1], 9).to("cuda")
        for step in range(T):
            with torch.no_grad():
                y = net(s.vector_states.to(torch.float32))
            s, _, _, _ = vec.policy_step(logits=y[:, :8].contiguous(), values=y[:, 8].contiguous())
        with torch.no_grad():
            vec.policy_value(net(s.vector_states.to(torch.float32))[:, 8].contiguous())
        ro = vec.rollout()
        adv, ret = vec.rollout_advantages(ro["pol_value"])
        scalars = dict(action=ro["pol_raw"][0], old_logp=ro["pol_logp"], old_value=ro["pol_value"], adv=adv, ret=ret)
        seen = 0
        for mb in vec.rollout_sequences(scalars, seed=3):
            rows = vec.sequence_rows(mb)
            assert rows["mb_vector_states"].shape[0] == L * Bs and rows["mb_vector_states"].data_ptr() == mb["mb_vector_states"].data_ptr()
            with torch.no_grad():
                y = net(rows["mb_vector_states"].to(torch.float32))
            logits, values = y[:, :8].contiguous().requires_grad_(), y[:, 8].contiguous().requires_grad_()
            loss, info = vec.policy_loss(rows, logits=logits, values=values, clip=0.2, clip_vf=0.2)
            first = {k: v.clone() for k, v in dict(info, loss_value=loss.detach()).items()}
            plain = {k: v.clone() for k, v in rows.items()}
            assert all(v.shape[0] == L * Bs for k, v in plain.items() if not k.startswith("mb_seq"))
            loss2, info2 = vec.policy_loss(plain, logits=logits, values=values, clip=0.2, clip_vf=0.2)
            second = dict(info2, loss_value=loss2.detach())
            for k in first:
                assert torch.equal(first[k], second[k]), k
            assert int(info2["n_bad"].item()) == 0 and float(info2["weight_sum"].item()) == float(rows["mb_weight"].sum().item())
            seen += float(rows["mb_weight"].sum().item()) > 0
        assert seen >= 1
    finally:
        vec.close()


# ---- 10. the enable call on a live handle ----
def test_enable_needs_the_rollout_and_reports_every_pointer():
    from img_env_amd import _cabi
    from img_env_amd.world import World
    grid, params, layout = small_world(6, 3, seed=4)
    w = World(params, grid)
    try:
        o = _cabi.SeqOut()
        assert w.lib.imgenv_rollout_seq_outputs(w.h, C.byref(o)) == _cabi.ESTATE
        assert w.lib.imgenv_rollout_seq_index(w.h, None) == _cabi.ESTATE
        with pytest.raises(RuntimeError, match="imgenv_rollout_enable"):
            w.enable_sequences(2, 8)
        with pytest.raises(RuntimeError, match="enable_sequences"):
            w.rollout_seq_index()
        assert w.sequences is None
        w.enable_rollout(4, 4, ["vector_states", "lasers"])
        with pytest.raises(ValueError, match="rollout stores"):
            w.enable_sequences(2, 8, 1, ["sensor_maps"])
        with pytest.raises(ValueError, match="horizon 4"):
            w.enable_sequences(5, 8)
        with pytest.raises(ValueError, match="state_bytes"):
            w.enable_sequences(2, 8, 1, None, (6,))
        launches = w.launches()
        sq = w.enable_sequences(3, 8, 3, None, (0, 24))  # 0: every field of the rollout; the second state array alone
        assert w.launches() == launches and w.minibatch is None
        assert w.enable_sequences(3, 8, 3, None, (0, 24)) is sq
        for other in ((2, 8, 3, None, (0, 24)), (3, 9, 3, None, (0, 24)), (3, 8, 2, None, (0, 24)), (3, 8, 3, ["lasers"], (0, 24)), (3, 8, 3, None, (24,))):
            with pytest.raises(ValueError, match="already"):
                w.enable_sequences(*other)
        assert {k for k in sq if k.startswith("mb_")} == {"mb_vector_states", "mb_lasers", "mb_seq_state1"} | set(_cabi.SEQ_SCALARS[:-1])
        assert sq["mb_lasers"].shape == (3, 3, 8) + tuple(w.out["lasers"].shape[1:]) and sq["mb_lasers"].dtype == w.out["lasers"].dtype
        assert w.lib.imgenv_rollout_seq_outputs(w.h, C.byref(o)) == 0
        assert (o.n_local, o.horizon, o.length, o.batch, o.buffers, o.fields, o.max_sequences, list(o.state_bytes)) == (6, 4, 3, 8, 3, 2 | 4, 12, [0, 24])
        for name in _cabi.SEQ_ARRAYS:
            assert getattr(o, name) and getattr(o, name) % 256 == 0, name
        for b in range(4):
            for name, _ in _cabi.SeqBuffer._fields_[:-1]:
                ptr = getattr(o.buf[b], name)
                want = b < 3 and name in ("mb_vector_states", "mb_lasers") + _cabi.SEQ_SCALARS[:-1]
                assert bool(ptr) == want and (not ptr or ptr % 256 == 0), (b, name)
            assert not o.buf[b].mb_seq_state[0] and bool(o.buf[b].mb_seq_state[1]) == (b < 3)
            if b < 3:
                assert o.buf[b].mb_lasers == sq["mb_lasers"][b].data_ptr() and sq["mb_lasers"][b].is_contiguous()
    finally:
        w.close()
