"""The last entries of full field tables on the device: one handle with every row-copy feature on and every field selected, so that
k_final_obs walks 17 fields and k_rollout / k_rollout_gather all 11 of their tables (csrc/field_rows.h: the walk is written once
and generated per table size).  The kernels only move bytes: every comparison is exact, no tolerance.

2 worlds x 2 robots with 1 pedestrian each, 181 beams, the 48 x 48 view of the sister suites (tests/test_gpu_final_obs.py's
narrow_cfg: the smallest view those suites run); stacks of depth (3, 3, 2), the normalised pedestrian vector, running normalisation
of observations and reward; final observations of every bit and the normalised states, a rollout of every bit and both
normalisation bits with T = 3 and F = 4, minibatches of 4 with 2 buffers.  Three steps, a host reset of world 1, then one index,
one shuffle and one gather.  The live arrays and stacks are read back right after the chain that wrote them; every ring slot,
final-list entry, final-observation row and minibatch row of every field equals the live rows it was copied from."""
import numpy as np
import pytest

from img_env_amd import _cabi
from test_gpu_final_obs import TABLE8, WRAPPERS, host, narrow_cfg, same

pytestmark = pytest.mark.gpu
E, R, P, T, F, B, NB = 2, 2, 1, 3, 4, 4, 2
OUT_FIELDS = tuple(list(_cabi.FINAL_BITS)[:11])
STACKS = ("stack_sensor_maps", "stack_vector_states", "stack_lasers")
NORMS = ("norm_vector_states", "norm_state_stack")
FINAL_FIELDS = OUT_FIELDS + STACKS + ("ped_vector_norm",) + NORMS                 # k_final_obs' table: 17 fields
RING_FIELDS = tuple(_cabi.ROLLOUT_FIELDS) + tuple(_cabi.ROLLOUT_NORM_FIELDS)      # k_rollout's and k_rollout_gather's: 11


def live(w):
    """every source array a field is copied from, on the host, as the chain in hand left it"""
    src = {f: w.out[f] for f in OUT_FIELDS}
    src.update({"stack_" + name: t for name, t in w.stack.items()})
    src["ped_vector_norm"] = w.obs_post["ped_vector_norm"]
    src.update({f: w.normalise[f] for f in NORMS})
    return host(src)


@pytest.fixture(scope="module")
def rec():
    """the run, once for the module (a failure in it is not run again for the next test)"""
    from img_env_amd.vec_env import VecImageEnv
    cfg = narrow_cfg(R, P, wrappers=WRAPPERS, discrete_action=True, discrete_actions=TABLE8, image_batch=3, state_batch=3, laser_batch=2,
                     keep_view_maps=True)
    vec = VecImageEnv(cfg, env_num=E, seed=9, auto_reset=False, stack=True, wrappers=True, normalise=dict(obs=True, reward=True))
    try:
        w = vec.world
        assert w.stack_depths == (3, 3, 2) and "ped_vector_norm" in w.obs_post
        w.enable_final_obs(list(_cabi.FINAL_BITS) + ["norm_states"])
        w.enable_rollout(T, F, list(_cabi.ROLLOUT_BITS) + ["norm_states", "norm_rewards"])
        w.enable_minibatch(B, NB)
        acts = np.random.default_rng(4).integers(0, len(TABLE8), (T, E * R)).astype(np.int64)
        vec.reset()
        w.rollout_begin()
        rec = {"live": [live(w)]}
        for t in range(T):
            vec.step(acts[t])
            rec["live"].append(live(w))
        vec.reset_envs([1])
        rec["after"] = live(w)
        rec["ring"], rec["final"] = host(w.rollout), host(w.final_obs)
        rec["cursor"] = w.rollout_cursor()
        w.rollout_index()
        w.rollout_shuffle(11)
        rec["mb"] = host(w.rollout_minibatch(0, 1))
        rec["order"] = host({"order": w.minibatch["order"], "valid_n": w.minibatch["valid_n"]})
    finally:
        vec.close()
    return rec


def test_every_field_of_the_full_tables_is_there(rec):
    assert set(FINAL_FIELDS) | {"final_count"} == set(rec["final"]) and len(FINAL_FIELDS) == 17
    assert {"obs_" + f for f in RING_FIELDS} <= set(rec["ring"]) and {"final_" + f for f in RING_FIELDS} <= set(rec["ring"]) and len(RING_FIELDS) == 11
    assert {"mb_" + f for f in RING_FIELDS} <= set(rec["mb"])
    assert set(FINAL_FIELDS) == set(rec["live"][0])
    for f in FINAL_FIELDS:  # (a copy that moved nothing would pass on arrays of zeros)
        # (the flags may all be clear, and no pedestrian need be in sight)
        assert rec["live"][T][f].any() or f in ("is_collisions", "is_arrives", "ped_maps", "ped_vector_states", "ped_vector_norm"), f


def test_final_observation_rows_equal_the_live_rows_before_the_reset(rec):
    before, fin = rec["live"][T], rec["final"]
    assert fin["final_count"].tolist() == [0, 0, 1, 1]  # world 1's rows, once; the handle's first reset captures nothing
    for f in FINAL_FIELDS:
        same(fin[f][R:], before[f][R:], "final observation: %s" % f)
        assert not fin[f][:R].any(), f


def test_ring_slots_and_final_list_equal_the_live_rows(rec):
    ring, lv = rec["ring"], rec["live"]
    assert rec["cursor"] == (T, 1)
    for f in RING_FIELDS:
        for s in range(T):
            same(ring["obs_" + f][s], lv[s][f], "slot %d: %s" % (s, f))
        # the reset chain rewrote world 1's rows of slot T and moved what they held into the final list, in row order
        same(ring["obs_" + f][T][:R], lv[T][f][:R], "slot %d, world 0: %s" % (T, f))
        same(ring["obs_" + f][T][R:], rec["after"][f][R:], "slot %d, world 1: %s" % (T, f))
        same(ring["final_" + f][:R], lv[T][f][R:], "final list: %s" % f)
        assert not ring["final_" + f][R:].any(), f
    assert ring["final_idx"][T].tolist() == [-1, -1, 0, 1] and (ring["final_idx"][:T] == -1).all()
    assert ring["final_slot"][:R].tolist() == [T, T] and ring["final_row"][:R].tolist() == [R, R + 1] and int(ring["final_n"][1]) == R


def test_minibatch_rows_equal_the_ring_rows_they_index(rec):
    ring, mb = rec["ring"], rec["mb"]
    V = int(rec["order"]["valid_n"][0])
    index = mb["mb_index"]
    same(index, rec["order"]["order"][:B], "mb_index")
    assert V >= 1 and index[0] >= 0
    for f in RING_FIELDS:
        flat = ring["obs_" + f].reshape((-1,) + ring["obs_" + f].shape[2:])  # k = t * R_local + row
        for i, k in enumerate(index.tolist()):
            if k >= 0:
                same(mb["mb_" + f][i], flat[k], "minibatch slot %d = transition %d: %s" % (i, k, f))
            else:
                assert not mb["mb_" + f][i].any(), (f, i)
