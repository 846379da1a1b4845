"""A branch of imgenv_step_begin / launch_views that no other GPU test executes, against the oracle at the smallest shape that
reaches it: IMGENV_SERIAL=1 (read when the handle is created) with pedestrians -- plan_side_wiring's serial rows: k_obs and k_orca
(which at several worlds does k_side_robots' part itself) on the caller's stream, no fork, no join, no early observation.

2 worlds x (2 robots + 2 ORCA pedestrians) in one handle, 48 x 48 view, a dozen steps with a reset of world 1 after the sixth,
every field of every world compared with an oracle of its own (tests/test_gpu_multiworld.py's checker).  That the switch was
taken shows in imgenv_layer_mode: the same handle created without it runs early-observation steps, the serial one cannot.
(IMGENV_EARLY_OBS=0 is read once per process and stays uncovered; k_integrate_serial is tests/test_gpu_parity.py's
dt_200_serial_integrate.)"""
import pytest

from scenarios import small_world
from test_gpu_multiworld import _run, _stack_params, worlds  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu
W, RW, PW, SEED = 2, 2, 2, 31


def test_no_side_streams_matches_the_oracle(worlds, monkeypatch):  # noqa: F811
    World, OracleWorld = worlds
    grid, params, _ = small_world(RW, PW, seed=SEED)
    plain = World(_stack_params(params, W), grid)
    try:
        assert plain.layer_mode()["early_observation"]
    finally:
        plain.close()
    monkeypatch.setenv("IMGENV_SERIAL", "1")
    early = []

    def serial_world(*a, **kw):
        w = World(*a, **kw)
        early.append(w.layer_mode()["early_observation"])
        return w

    fails, snap, _ = _run(serial_world, OracleWorld, W, RW, PW, steps=12, resets={5: [1]}, seed=SEED)
    assert not fails, fails[:3]
    assert early == [False] and snap["robot_pose"].shape[0] == W * RW
