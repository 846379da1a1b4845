"""The scenario bank without a GPU (include/imgenv.h, "scenario bank"): ``imgenv_scenario_for_placement`` through ctypes against
tests/scenario_bank_model.py -- the queue with its wrap near 2^64, the draw's spread and its independence from the map bank's and
the track bank's draws of the same seed -- and ``_cabi.pack_scenarios`` round-tripped through ``imgenv_spawn``'s array layout on
the reference's recorded episodes (tests/golden/spawn_ref.npz)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import scenario_bank_model as sbm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 256  # pool slots of a handle of up to 64 worlds: (SPAWN_FILL_PERIOD + 2) * max(64, W)


@pytest.fixture(scope="module")
def lib():
    from img_env_amd import _cabi
    path = _cabi.library_path()
    if not os.path.exists(path):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return _cabi.bind(C.CDLL(path))


def _draw(lib, policy, seed0, first, n, N):
    return int(lib.imgenv_scenario_for_placement(policy, C.c_uint64(seed0 & sbm.M64), C.c_uint64(first & sbm.M64), C.c_uint64(n & sbm.M64), N))


@pytest.mark.parametrize("N", [1, 7, 256, 300])
def test_the_library_agrees_with_the_model_over_100000_placements(lib, N):
    """N > S, N = S and N coprime to S (S = 256 slots): QUEUE and BY_PLACEMENT, the numpy model, the integer model and the library"""
    seed0, first = 0x9E3779B97F4A7C15 * 10, 5
    ns = np.arange(100000, dtype=np.uint64)
    for policy in (1, 2):
        got = np.array([_draw(lib, policy, seed0, first, int(n), N) for n in ns])
        want = sbm.scenarios_for_placements(policy, seed0, first, ns, N)
        assert np.array_equal(got, want), policy
        for n in (0, 1, 255, 256, 257, 99999):
            assert got[n] == sbm.scenario_for_placement(policy, seed0, first, n, N)
        assert got.min() >= 0 and got.max() < N
    q = sbm.scenarios_for_placements("queue", 0, first, ns, N)
    assert np.array_equal(q[:2 * N + 3], (first + np.arange(2 * N + 3)) % N)  # one pass of N resets runs every scenario once
    assert _draw(lib, 0, seed0, first, 3, N) == -1 and _draw(lib, 1, seed0, first, 3, 0) == -1


@pytest.mark.parametrize("N", [7, 256, 300])
def test_the_queue_wraps_modulo_2_to_the_64_on_both_sides(lib, N):
    for first in (sbm.M64, sbm.M64 - 3, sbm.M64 - N, 1 << 63, (1 << 64) - (1 << 32)):
        ns = [0, 1, 2, 3, 4, N, N + 1, 1 << 32, (1 << 63) + 5, sbm.M64]
        got = [_draw(lib, 1, 0, first, n, N) for n in ns]
        assert got == [((first + n) % (1 << 64)) % N for n in ns], first
        assert got == sbm.scenarios_for_placements(1, 0, first, np.array(ns, np.uint64), N).tolist()
        assert got == [sbm.scenario_for_placement("queue", 0, first, n, N) for n in ns]
    # 2^64 is no multiple of 7 or 300: across the wrap the queue jumps, and both sides jump alike
    first = sbm.M64 - 1
    assert [_draw(lib, 1, 0, first, n, 7) for n in range(4)] == [(first % 7), ((first + 1) % 7), 0, 1]


@pytest.mark.parametrize("N", [7, 300])
def test_the_draw_spreads_over_the_bank_and_is_tied_to_no_other_bank(lib, N):
    """BY_PLACEMENT over 10^5 placements: every scenario is drawn about equally often (a binomial count stays within six standard
    deviations), and for one seed the scenario is neither the map bank's draw nor the track bank's"""
    seed0 = 12345
    ns = np.arange(100000, dtype=np.uint64)
    got = sbm.scenarios_for_placements("placement", seed0, 0, ns, N)
    counts = np.bincount(got, minlength=N)
    p = 1.0 / N
    assert np.all(np.abs(counts - len(ns) * p) < 6 * np.sqrt(len(ns) * p * (1 - p))), counts
    maps = np.array([int(lib.imgenv_map_for_placement(C.c_uint64(seed0 + int(n)), N)) for n in ns[:20000]])
    tracks = np.array([int(lib.imgenv_tracks_for_placement(C.c_uint64(seed0 + int(n)), N)) for n in ns[:20000]])
    mine = got[:20000]
    for other in (maps, tracks):  # independent draws agree with probability 1 / N: six standard deviations again
        agree = int((mine == other).sum())
        assert abs(agree - 20000 * p) < 6 * np.sqrt(20000 * p * (1 - p)) + 1, agree
    assert sbm.SALT != sbm.TRACKS_SALT and sbm.SALT != 0


def test_python_binding_and_constants():
    from img_env_amd import _cabi
    assert _cabi.SCENARIO_POLICIES == sbm.POLICIES and _cabi.SCENARIO_PLACEMENT_SALT == sbm.SALT
    for policy in ("off", "queue", "placement"):
        assert [_cabi.scenario_for_placement(policy, 9, 4, n, 5) for n in range(40)] == [sbm.scenario_for_placement(policy, 9, 4, n, 5) for n in range(40)]


def test_the_model_follows_hosts_devices_and_switches():
    m = sbm.ScenarioModel(3, 7, seed0=11)
    assert m.cur.tolist() == [-1, -1, -1]
    m.host_reset(0, 4)
    m.set_policy("queue", first=3)
    assert m.device_reset(1, 0) == 3 and m.device_reset(2, 5) == 1
    m.set_policy("off", at=6)
    assert m.device_reset(1, 6) == -1 and m.scenario_of(5) == 1
    m.set_policy("placement", at=9)
    assert m.device_reset(0, 9) == sbm.scenario_for_placement(2, 11, 0, 9, 7) and m.scenario_of(8) == -1
    m.host_reset(0)
    assert m.cur.tolist() == [-1, -1, 1]


def _golden_layouts():
    """the reference's recorded episodes as layouts, grouped by cast (R, P, O)"""
    from img_env_amd.worldgen import ResetLayout
    z = np.load(os.path.join(ROOT, "tests", "golden", "spawn_ref.npz"))
    casts = {}
    for case in sorted(k[:-5] for k in z.files if k.endswith("/seed")):
        g = lambda k: z["%s/%s" % (case, k)]  # noqa: E731
        nr = int(json.loads(str(g("cfg")))["robot"]["total"])
        init, P = g("init"), len(g("init")) - nr
        quat = lambda yaw: np.stack([np.sin(yaw / 2.0), np.cos(yaw / 2.0)], axis=1)  # noqa: E731
        traj = np.zeros((P, 2, 3))
        traj[:, :, :2] = g("ped_traj")
        for j, n in enumerate(g("ped_traj_len")):
            traj[j, n:] = 0.0
        lay = ResetLayout(robot_pose=np.hstack([init[:nr, :2], g("robot_quat")]), robot_goal=g("robot_goal"),
                          ped_pose=np.hstack([init[nr:, :2], quat(init[nr:, 2])]), ped_goal=g("target")[nr:, :2].copy(), ped_traj=traj,
                          ped_traj_len=g("ped_traj_len"), obs_shape=g("obs_shape"), obs_size=g("obs_size").astype(np.float32),
                          obs_pose=np.hstack([g("obs_range")[:, :2], g("obs_quat")]))
        casts.setdefault((nr, P, len(lay.obs_shape)), []).append(lay)
    return casts


def test_pack_scenarios_round_trips_the_recorded_episodes():
    """every episode of the golden file whose cast fits one bank (robots + pedestrians <= 256, obstacles <= 24, trajectories of at
    most two points): packed per cast, each array keeps its dtype, its [n] axis and every byte"""
    from img_env_amd import _cabi
    casts = _golden_layouts()
    assert sum(len(v) for v in casts.values()) == 15
    packed_any = 0
    for (R, P, O), lays in casts.items():
        if R + P > _cabi.SPAWN_MAX_AGENTS or O > _cabi.SPAWN_MAX_OBST or any(int(l.ped_traj_len.max(initial=0)) > 2 for l in lays):
            continue
        arrays = _cabi.pack_scenarios(lays, R, P, O)
        assert list(arrays) == ["robot_pose", "robot_goal", "ped_pose", "ped_goal", "ped_traj", "ped_traj_len", "obs_shape", "obs_size", "obs_pose"]
        for name, (dt, shape) in _cabi.scenario_arrays(R, P, O).items():
            a = arrays[name]
            assert a.dtype == dt and a.shape == (len(lays),) + shape and a.flags["C_CONTIGUOUS"], name
            for s, lay in enumerate(lays):
                assert a[s].tobytes() == np.ascontiguousarray(getattr(lay, name), dt).tobytes(), (name, s)
        packed_any += len(lays)
        with pytest.raises(ValueError):  # one cast per bank
            _cabi.pack_scenarios(lays, R + 1, P, O)
    assert packed_any >= 10
    with pytest.raises(ValueError):
        _cabi.pack_scenarios([], 1, 0, 0)
