"""tests/rollout_model.py against answers worked out by hand: every branch of the advantage pass (include/imgenv.h:
imgenv_rollout_gae) on a rollout of three steps and one row, with gamma = 0.5, lam = 0.5 (gl = 0.25) and values that are powers of
two, so every product and sum below is exact in float32; and the bookkeeping of a reset chain on a ring of two rows.

Slots 0..3 are worth 1, 2, 4, 8 and every reward is 1 unless a case says otherwise.  With nothing happening:
  t = 2: delta = 1 + 0.5 * 8 - 4 = 1, gae = 1;  t = 1: delta = 1 + 0.5 * 4 - 2 = 1, gae = 1 + 0.25 * 1 = 1.25;
  t = 0: delta = 1 + 0.5 * 2 - 1 = 1, gae = 1 + 0.25 * 1.25 = 1.3125;  ret = gae + value.
Every case changes transition 1 (and says what else)."""
import numpy as np
import pytest

import rollout_model

VALUES = np.array([[1.0], [2.0], [4.0], [8.0]], np.float32)
F = 4


def rollout(dones=(0, 0, 0), info=(0, 0, 0), clean=(1, 1, 1), final_idx=(-1, -1, -1, -1), rewards=(1.0, 1.0, 1.0), n=3):
    col = lambda v, dt: np.array(v, dt).reshape(-1, 1)  # noqa: E731
    return {"n": n, "dones": col(dones, np.uint8), "dones_info": col(info, np.int32), "is_clean": col(clean, np.uint8),
            "final_idx": col(final_idx, np.int32), "rewards": col(rewards, np.float32)}


def run(r, final_values=(16.0, 0.0, 0.0, 0.0), **kw):
    fv = None if final_values is None else np.array(final_values, np.float32)
    adv, ret = rollout_model.gae(r, VALUES, fv, 0.5, 0.5, F, **kw)
    assert adv.dtype == np.float32 and ret.dtype == np.float32
    return adv[:, 0].tolist(), ret[:, 0].tolist()


def test_nothing_happens():
    assert run(rollout()) == ([1.3125, 1.25, 1.0], [2.3125, 3.25, 5.0])


def test_arrive():
    # a real end bootstraps from nothing, although the reset left a final entry worth 16: delta1 = 1 + 0 - 2 = -1, and the trace
    # stops there; t = 0: 1 + 0.25 * -1 = 0.75; t = 2 is the new episode's: 1
    assert run(rollout(dones=(0, 1, 0), info=(0, 5, 0), final_idx=(-1, -1, 0, -1))) == ([0.75, -1.0, 1.0], [1.75, 1.0, 5.0])


def test_collision():
    # the same without a reset behind it (the robot's env goes on): dones_info 1..3
    for code in (1, 2, 3):
        assert run(rollout(dones=(0, 1, 0), info=(0, code, 0))) == ([0.75, -1.0, 1.0], [1.75, 1.0, 5.0])


def test_timeout_with_a_final_entry():
    # the time limit cut the episode off and the reset kept what it overwrote, worth 16: delta1 = 1 + 0.5 * 16 - 2 = 7; no trace
    # from the new episode; t = 0: 1 + 0.25 * 7 = 2.75
    assert run(rollout(dones=(0, 1, 0), info=(0, 10, 0), final_idx=(-1, -1, 0, -1))) == ([2.75, 7.0, 1.0], [3.75, 9.0, 5.0])


def test_timeout_with_the_entry_dropped():
    # e >= F: the final list was full, nothing to bootstrap from: as a real end.  The same without final_values
    r = rollout(dones=(0, 1, 0), info=(0, 10, 0), final_idx=(-1, -1, F + 1, -1))
    assert run(r) == ([0.75, -1.0, 1.0], [1.75, 1.0, 5.0])
    assert run(rollout(dones=(0, 1, 0), info=(0, 10, 0), final_idx=(-1, -1, F, -1))) == ([0.75, -1.0, 1.0], [1.75, 1.0, 5.0])
    assert run(rollout(dones=(0, 1, 0), info=(0, 10, 0), final_idx=(-1, -1, 0, -1)), final_values=None) == ([0.75, -1.0, 1.0], [1.75, 1.0, 5.0])


def test_timeout_not_yet_reset():
    # nobody has reset the row: slot 2 still shows the state the time limit cut off, worth 4: delta1 = 1 + 2 - 2 = 1, but the trace
    # stops at the done; t = 0: 1 + 0.25 * 1 = 1.25
    assert run(rollout(dones=(0, 1, 0), info=(0, 10, 0))) == ([1.25, 1.0, 1.0], [2.25, 3.0, 5.0])


def test_reset_without_done():
    # the caller reset the env in mid-episode: the value of what the reset overwrote (entry 1, worth 32): delta1 = 1 + 16 - 2 = 15,
    # no trace across the restart; t = 0: 1 + 0.25 * 15 = 4.75
    assert run(rollout(final_idx=(-1, -1, 1, -1)), final_values=(16.0, 32.0, 0.0, 0.0)) == ([4.75, 15.0, 1.0], [5.75, 17.0, 5.0])


def test_unclean_row_between_a_done_and_the_restart():
    # the robot arrives at t = 0 (reward 2) while its env goes on; at t = 1 it is frozen (is_clean 0: MultiRobotCleanWrapper), then
    # the env restarts.  t = 1: adv = ret = 0 and the trace is cut; t = 0: delta = 2 + 0 - 1 = 1
    r = rollout(dones=(1, 1, 0), info=(5, 5, 0), clean=(1, 0, 1), final_idx=(-1, -1, 0, -1), rewards=(2.0, 1.0, 1.0))
    assert run(r) == ([1.0, 0.0, 1.0], [2.0, 0.0, 5.0])
    # an unclean row cuts the trace of a row that is not done as well: t = 0: delta = 1 + 1 - 1 = 1 and nothing carried over
    assert run(rollout(clean=(1, 0, 1))) == ([1.0, 0.0, 1.0], [2.0, 0.0, 5.0])


def test_rows_behind_the_cursor_stay():
    keep = np.full((3, 1), 7.0, np.float32)
    adv, ret = run(rollout(n=2), adv=keep, ret=keep)
    # (two transitions: t = 1: delta = 1 + 2 - 2 = 1; t = 0: 1 + 0.25 = 1.25)
    assert adv == [1.25, 1.0, 7.0] and ret == [2.25, 3.0, 7.0]


def test_replay_by_hand():
    # two rows, T = 2, F = 1: a step, a reset chain over row 1 (entry 0), a step, a reset chain over rows 1 and 0 (entries 1 and 2:
    # dropped), in that order
    o = lambda *v: {"x": np.array(v, np.int32).reshape(2, 1)}  # noqa: E731
    step = lambda obs, rew: {"kind": "step", "obs": obs, "actions": np.zeros((2, 3)), "rewards": rew, "dones": [0, 1], "is_clean": [1, 1],  # noqa: E731
                             "dones_info": [0, 10]}
    chains = [step(o(10, 11), [0.1, 0.2]), {"kind": "reset", "rows": [1], "obs": o(10, 21)}, step(o(30, 31), [1.0, 2.0]),
              {"kind": "reset", "rows": [1, 0], "obs": o(40, 41)}]
    r = rollout_model.replay(2, 1, o(0, 1), chains)
    assert r["n"] == 2 and r["resets"] == 2 and r["final_count"] == 3
    assert r["obs_x"][:, :, 0].tolist() == [[0, 1], [10, 21], [40, 41]]
    assert r["final_x"][:, 0].tolist() == [11] and r["final_slot"].tolist() == [1] and r["final_row"].tolist() == [1]
    assert r["final_idx"].tolist() == [[-1, -1], [-1, 0], [2, 1]]
    assert r["final_n"].tolist() == [3, 1]  # (the two words, in turns: chain 0 wrote word 1, chain 1 word 0)
    assert r["rewards"].tolist() == [[np.float32(0.1), np.float32(0.2)], [1.0, 2.0]] and r["dones_info"].tolist() == [[0, 10], [0, 10]]
    with pytest.raises(AssertionError, match="rollout full"):
        rollout_model.replay(2, 1, o(0, 1), chains + [step(o(0, 0), [0.0, 0.0])])
