"""The enable protocol of the eleven optional features on a live handle (csrc/feature_plan.h decides, csrc/imgenv_hip.hip allocates):
calls out of order change nothing, a repeated call hands back the same bytes, another cfg is refused with the stored one's text,
the features cost the chain the launches they cost before the state records existed, and each minibatch buffer's destination
pointers address that buffer.

The smallest handle that has every array (tests/test_gpu_field_tables_full.py's): 2 worlds x 2 robots with 1 pedestrian each, 181
beams, stacks of depth (2, 2, 2); rollout_horizon 2, final_capacity 2, minibatches of 2 with 2 buffers, a loss of 2 rows."""
import ctypes as C

import numpy as np
import pytest

from img_env_amd import _cabi
from test_gpu_final_obs import TABLE8, WRAPPERS, fixed_actions, host, narrow_cfg, same

pytestmark = pytest.mark.gpu
E, R, P, T, F, B, NB, ROWS = 2, 2, 1, 2, 2, 2, 2, 2
NOT_CALLED = "%s was not called"
ROLL_FIELDS = _cabi.ROLLOUT_ALL | _cabi.ROLLOUT_NORM_STATES | _cabi.ROLLOUT_NORM_REWARDS
FINAL_FIELDS = _cabi.FINAL_ALL | _cabi.FINAL_NORM_STATES


def make_vec():
    from img_env_amd.vec_env import VecImageEnv
    cfg = narrow_cfg(R, P, wrappers=WRAPPERS, discrete_action=True, discrete_actions=TABLE8, image_batch=2, state_batch=2, laser_batch=2,
                     keep_view_maps=True)
    return VecImageEnv(cfg, env_num=E, seed=9, auto_reset=False), cfg


@pytest.fixture
def vec():
    v, cfg = make_vec()
    v.yaml = cfg
    try:
        yield v
    finally:
        v.close()


# name -> (the Out struct, the cfg of this test); the order is one every prerequisite allows
def cfgs(control_hz):
    actions, keep = _cabi.make_actions_cfg(table=TABLE8)
    return keep, {
        "stack": (_cabi.StackOut, _cabi.make_stack_cfg(2, 2, 2)),
        "episodes": (_cabi.EpisodesOut, _cabi.make_episodes_cfg(3, control_hz)),
        "episode_log": (_cabi.EpisodeLogOut, _cabi.make_episode_log_cfg(8)),
        "actions": (_cabi.ActionsOut, actions),
        "obs_post": (_cabi.ObsPostOut, _cabi.make_obs_post_cfg(True, True)),
        "normalise": (_cabi.NormaliseOut, _cabi.make_normalise_cfg(True, True)),
        "final_obs": (_cabi.FinalObsOut, _cabi.make_final_obs_cfg(FINAL_FIELDS)),
        "rollout": (_cabi.RolloutOut, _cabi.make_rollout_cfg(T, F, ROLL_FIELDS)),
        "policy": (_cabi.PolicyOut, _cabi.make_policy_cfg("categorical", seed=5, store=True)),
        "policy_loss": (_cabi.PolicyLossOut, _cabi.make_policy_loss_cfg(ROWS)),
        "rollout_minibatch": (_cabi.MinibatchOut, _cabi.make_minibatch_cfg(B, NB, 0)),
    }


def enable(w, name, cfg, out):
    rc = getattr(w.lib, "imgenv_%s_enable" % name)(w.h, C.byref(cfg), C.byref(out))
    return rc, w.lib.imgenv_last_error().decode()


def outputs(w, name, out):
    rc = getattr(w.lib, "imgenv_%s_outputs" % name)(w.h, C.byref(out))
    return rc, w.lib.imgenv_last_error().decode()


def assert_off(w, name, out_type):
    rc, text = outputs(w, name, out_type())
    assert (rc, text) == (_cabi.ESTATE, NOT_CALLED % ("imgenv_%s_enable" % name)), (name, rc, text)


def raw(struct):
    return bytes(memoryview(struct).cast("B"))


def test_an_enable_before_its_prerequisite_is_refused_and_changes_nothing(vec):
    w = vec.world
    keep, c = cfgs(float(vec.yaml["control_hz"]))

    def refused(name, cfg, code, text):
        out_type = c[name][0]
        assert enable(w, name, cfg, out_type()) == (code, text), name
        assert_off(w, name, out_type)

    refused("episode_log", c["episode_log"][1], _cabi.ESTATE, "imgenv_episode_log_enable before imgenv_episodes_enable")
    refused("policy", c["policy"][1], _cabi.ESTATE, "imgenv_policy_enable before imgenv_actions_enable")
    refused("policy_loss", c["policy_loss"][1], _cabi.ESTATE, "imgenv_policy_loss_enable before imgenv_policy_enable")
    refused("rollout_minibatch", c["rollout_minibatch"][1], _cabi.ESTATE, "imgenv_rollout_minibatch_enable before imgenv_rollout_enable")
    refused("rollout_minibatch", _cabi.make_minibatch_cfg(B, NB, _cabi.ROLLOUT_NORM_STATES), _cabi.EINVAL,
            "imgenv_minibatch_cfg.fields 128: IMGENV_ROLLOUT_NORM_* before imgenv_normalise_enable")
    # the field bits in front of the feature that keeps the array
    refused("final_obs", _cabi.make_final_obs_cfg(_cabi.FINAL_BITS["stacks"]), _cabi.ESTATE, "IMGENV_FINAL_STACKS before imgenv_stack_enable")
    refused("rollout", _cabi.make_rollout_cfg(T, F, _cabi.ROLLOUT_BITS["stacks"]), _cabi.ESTATE, "IMGENV_ROLLOUT_STACKS before imgenv_stack_enable")
    refused("final_obs", _cabi.make_final_obs_cfg(_cabi.FINAL_BITS["ped_vector_norm"]), _cabi.ESTATE,
            "IMGENV_FINAL_PED_NORM before imgenv_obs_post_enable with IMGENV_OBS_PED_NORM")
    refused("rollout", _cabi.make_rollout_cfg(T, F, _cabi.ROLLOUT_BITS["ped_vector_norm"]), _cabi.ESTATE,
            "IMGENV_ROLLOUT_PED_NORM before imgenv_obs_post_enable with IMGENV_OBS_PED_NORM")
    refused("final_obs", _cabi.make_final_obs_cfg(1 | _cabi.FINAL_NORM_STATES), _cabi.EINVAL,
            "imgenv_final_obs_cfg.fields 8193: IMGENV_FINAL_NORM_STATES before imgenv_normalise_enable with IMGENV_NORM_OBS")
    refused("rollout", _cabi.make_rollout_cfg(T, F, 2 | _cabi.ROLLOUT_NORM_STATES), _cabi.EINVAL,
            "imgenv_rollout_cfg.fields 130: IMGENV_ROLLOUT_NORM_* before imgenv_normalise_enable")
    # IMGENV_POLICY_STORE in front of the rollout: the actions are there, the head still is not
    assert enable(w, "actions", c["actions"][1], _cabi.ActionsOut())[0] == 0
    refused("policy", c["policy"][1], _cabi.ESTATE, "imgenv_policy_enable: IMGENV_POLICY_STORE before imgenv_rollout_enable")
    del keep


def test_every_enable_in_order_then_repeated_then_with_another_cfg(vec):
    w = vec.world
    hz = float(vec.yaml["control_hz"])
    keep, c = cfgs(hz)
    other_actions, keep2 = _cabi.make_actions_cfg(table=TABLE8[:-1])
    # another cfg for each, and what the refusal says of the stored one
    other = {
        "episodes": (_cabi.make_episodes_cfg(4, hz), "imgenv_episodes_enable: the handle already keeps statistics with min_steps 3, dt %g" % hz),
        "episode_log": (_cabi.make_episode_log_cfg(9), "imgenv_episode_log_enable: the handle already keeps a log of capacity 8"),
        "actions": (other_actions, "imgenv_actions_enable: the handle already decodes actions with another cfg"),
        "obs_post": (_cabi.make_obs_post_cfg(True, True, close_dist=_cabi.CLOSE_DIST + 1.0),
                     "imgenv_obs_post_enable: the handle already post-processes its observations with another cfg"),
        "final_obs": (_cabi.make_final_obs_cfg(1), "imgenv_final_obs_enable: the handle already keeps final observations of the fields %d" % FINAL_FIELDS),
        "rollout": (_cabi.make_rollout_cfg(T + 1, F, ROLL_FIELDS),
                    "imgenv_rollout_enable: the handle already keeps a rollout of horizon %d, final_capacity %d, fields %d" % (T, F, ROLL_FIELDS)),
        "policy": (_cabi.make_policy_cfg("categorical", seed=6, store=True), "imgenv_policy_enable: the handle already has a policy head with another cfg"),
        "policy_loss": (_cabi.make_policy_loss_cfg(ROWS + 1), "imgenv_policy_loss_enable: the handle already has a policy loss with another cfg"),
        "rollout_minibatch": (_cabi.make_minibatch_cfg(B, NB, 2),
                              "imgenv_rollout_minibatch_enable: the handle already gathers minibatches of batch %d, buffers %d, fields 0" % (B, NB)),
    }
    # (the two that refuse any second call)
    second = {"stack": (_cabi.ESTATE, "imgenv_stack_enable has already been called on this handle"),
              "normalise": (_cabi.EINVAL, "imgenv_normalise_enable has already been called on this handle")}
    for name, (out_type, cfg) in c.items():
        assert_off(w, name, out_type)
        first = out_type()
        rc, text = enable(w, name, cfg, first)
        assert rc == 0, (name, rc, text)
        assert first.struct_size == C.sizeof(out_type)
        again = out_type()
        if name in second:
            assert enable(w, name, cfg, again) == second[name], name
        else:
            rc, text = enable(w, name, cfg, again)
            assert rc == 0, (name, rc, text)
            assert raw(again) == raw(first), name
            cfg2, text2 = other[name]
            assert enable(w, name, cfg2, out_type()) == (_cabi.EINVAL, text2), name
        now = out_type()
        assert outputs(w, name, now)[0] == 0, name
        if name != "normalise":  # (later enables add the normalised fields' pointers to imgenv_normalise_out; checked below)
            assert raw(now) == raw(first), name
    # the normalised fields' pointers were handed out through imgenv_normalise_out, by the three features that copy them
    no = _cabi.NormaliseOut()
    assert outputs(w, "normalise", no)[0] == 0
    for member in ("final_norm_vector_states", "final_norm_state_stack", "rollout_obs_norm_vector_states", "rollout_obs_norm_state_stack",
                   "rollout_final_norm_vector_states", "rollout_final_norm_state_stack"):
        assert getattr(no, member), member
    for b in range(_cabi.MB_MAX_BUFFERS):
        assert bool(no.mb_norm_vector_states[b]) == (b < NB) and bool(no.mb_norm_state_stack[b]) == (b < NB), b
    del keep, keep2


# What the features add to a step chain: stack, episodes, obs_post, the two of the normalisation (training, obs and reward) and the
# rollout.  Measured with this test's body on the commit BEFORE the features' state records (its parent), not on the code under test.
PARENT_FEATURE_LAUNCHES = 6


def step_launches(everything):
    v, cfg = make_vec()
    try:
        w = v.world
        if everything:
            w.enable_stack(2, 2, 2)
            w.enable_episodes(3, float(cfg["control_hz"]))
            w.enable_episode_log(8)
            w.enable_actions(discrete_actions=TABLE8)
            w.enable_obs_post(True, True)
            w.enable_normalise(True, True)
            w.enable_final_obs(list(_cabi.FINAL_BITS) + ["norm_states"])
            w.enable_rollout(T, F, list(_cabi.ROLLOUT_BITS) + ["norm_states", "norm_rewards"])
            w.enable_policy("categorical", seed=5, store=True)
            w.enable_policy_loss(ROWS)
            w.enable_minibatch(B, NB)
        v._reset()
        if everything:
            w.rollout_begin()
        acts = fixed_actions(2, E * R)
        counts = []
        for t in range(2):
            w.step(acts[t])
            counts.append(w.launches())
        return counts
    finally:
        v.close()


def test_the_features_add_the_launches_they_added_before():
    plain, full = step_launches(False), step_launches(True)
    print("launches per step: plain", plain, "everything on", full)
    assert [f - p for f, p in zip(full, plain)] == [PARENT_FEATURE_LAUNCHES] * 2


def test_a_minibatch_lands_in_the_buffer_it_names(vec):
    w = vec.world
    w.enable_rollout(T, F, ["vector_states"])
    w.enable_minibatch(B, NB)
    vec._reset()
    w.rollout_begin()
    acts = fixed_actions(T, E * R)
    for t in range(T):
        w.step(acts[t])
    w.rollout_index()
    w.rollout_shuffle(11)
    mb = host(w.rollout_minibatch(0, 1))
    ring = host(w.rollout)["obs_vector_states"]
    both = host({"mb_vector_states": w.minibatch["mb_vector_states"], "mb_index": w.minibatch["mb_index"]})
    index = mb["mb_index"]
    assert (index >= 0).any()
    flat = ring.reshape((-1,) + ring.shape[2:])  # k = t * R_local + row
    for i, k in enumerate(index.tolist()):
        if k >= 0:
            same(both["mb_vector_states"][1][i], flat[k], "buffer 1, slot %d = transition %d" % (i, k))
            assert flat[k].any()
    same(both["mb_index"][1], index, "buffer 1's mb_index")
    assert not both["mb_vector_states"][0].any() and not both["mb_index"][0].any()  # buffer 0: as allocated
