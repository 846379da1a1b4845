"""The track bank without a GPU (include/imgenv.h, "track bank"): the draw ``imgenv_tracks_for_placement`` through ctypes against
tests/tracks_model.py, the CYCLE order against the order the reference's PedTrajectoryDatasetWrapper handed its worlds out in
(tests/golden/ped_dataset_ref.npz), ``envs.dataset_track_sets`` against the same recording's series, bit for bit, and the packing
of sets for ``imgenv_tracks_add``."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import tracks_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ped_dataset_ref.npz")


@pytest.fixture(scope="module")
def lib():
    from img_env_amd import _cabi
    path = _cabi.library_path()
    if not os.path.exists(path):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return _cabi.bind(C.CDLL(path))


def _dataset_cfg(tmp_path, z, **over):
    path = str(tmp_path / "world.csv")
    np.savetxt(path, z["csv"], delimiter=",", fmt="%.17g")
    cfg = dict(control_hz=0.4, ped_traj_dataset=path, repeated_time_per_env=2, ped_dataset_worlds=z["worlds"].tolist(), ped_sim=dict(total=0),
               node_id=0, output_file=str(tmp_path / "log.txt"), offset=z["offset"].tolist(), swapxy=True, fps=15, start_t=0, max_time=20,
               scale_x=1, scale_y=1, spawn_delay_s=0)
    cfg.update(over)
    return cfg


@pytest.mark.parametrize("n_sets", [1, 2, 3, 7])
def test_placement_draw_matches_its_definition_and_hits_every_set(lib, n_sets):
    """10^5 seeds: the library's draw is the documented one (map_for_placement over seed + salt), every set is drawn, and the salt
    does its job -- the set of a seed is not always the map of that seed"""
    draw = lambda s: int(lib.imgenv_tracks_for_placement(C.c_uint64(s & tracks_model.M64), n_sets))
    maps = lambda s: int(lib.imgenv_map_for_placement(C.c_uint64(s & tracks_model.M64), n_sets))
    seeds = list(range(100000 - 6)) + [2 ** 31 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1, 0x9E3779B97F4A7C15, 2 ** 64 - tracks_model.SALT]
    got = [draw(s) for s in seeds]
    assert got == [tracks_model.tracks_for_placement(s, n_sets) for s in seeds]
    assert set(got) == set(range(n_sets))
    if n_sets > 1:
        assert any(g != maps(s) for g, s in zip(got, seeds))
    else:
        assert set(got) == {0}


def test_python_binding_and_constants():
    from img_env_amd import _cabi
    assert _cabi.TRACK_POLICIES == tracks_model.POLICIES and _cabi.TRACKS_PLACEMENT_SALT == tracks_model.SALT
    assert [_cabi.tracks_for_placement(s, 5) for s in range(50)] == [tracks_model.tracks_for_placement(s, 5) for s in range(50)]


def test_cycle_order_is_the_reference_wrappers():
    """the reference ran repeated_time_per_env = 2 episodes per world and recorded which world each reset handed out"""
    z = np.load(GOLDEN)
    n = sum(1 for k in z.files if k.startswith("series_"))
    n_sets = len(z["worlds"])
    want = [int(z["world_%d" % e]) for e in range(n)]
    assert len(set(want)) > 1
    m = tracks_model.TracksModel(3, n_sets, "cycle", repeat=2)
    assert [m.reset(1) for _ in range(n)] == want
    assert [tracks_model.tracks_for_cycle(e, 2, n_sets) for e in range(n)] == want
    assert m.reset(1) == 0                                        # where the reference exits, the bank wraps
    assert m.cur.tolist() == [-1, 0, -1] and m.count.tolist() == [0, n + 1, 0]   # the other worlds have not moved


def test_model_policies():
    m = tracks_model.TracksModel(4, 3)
    assert m.reset(0) == 0 and m.cur[0] == 0
    m.select([1, 2], [2, 1])
    assert (m.reset(1), m.reset(2), m.reset(3)) == (2, 1, 0)
    assert m.reset(1, seed=77) == 2                               # KEEP ignores seeds
    m.reset_explicit(2)
    assert m.cur[2] == -1 and m.next[2] == 1 and m.count[2] == 1  # own tracks: no set, no count, the choice stays
    m.set_policy("placement")
    s = m.reset(3, seed=12345)
    assert s == tracks_model.tracks_for_placement(12345, 3) and m.next[3] == s
    assert m.reset(3) == s                                        # a bank-fed reset without a seed keeps the choice
    m.set_policy("cycle", 2)
    assert [m.reset(0) for _ in range(7)] == [0, 0, 1, 1, 2, 2, 0]
    m.set_policy("keep")
    assert m.reset(0) == 0
    with pytest.raises(ValueError):
        m.set_policy("cycle", 0)


def test_dataset_track_sets_are_the_reference_series(tmp_path):
    from img_env_amd.envs import dataset_track_sets
    z = np.load(GOLDEN)
    cfg = _dataset_cfg(tmp_path, z)
    sets = dataset_track_sets(cfg)
    assert cfg["ped_sim"]["total"] == 0 and not os.path.exists(cfg["output_file"])      # the cfg is read, nothing is written
    assert len(sets) == len(z["worlds"])
    total, cap = int(z["total0"]), max(s.shape[1] for s, _ in sets)
    n = sum(1 for k in z.files if k.startswith("series_"))
    used = set()
    for e in range(n):
        w = int(z["world_%d" % e])
        series, lengths = sets[w]
        ref = z["series_%d" % e]
        assert series.shape == (total, cap, 5) and series.dtype == np.float64 and lengths.dtype == np.int32
        assert (lengths == ref.shape[1]).all()
        assert np.array_equal(series[:, :ref.shape[1]], ref), (e, w)                      # bit for bit
        assert (series[:, ref.shape[1]:] == 0).all()
        used.add(w)
    assert used == set(range(len(sets)))


def test_dataset_track_sets_refuses_a_world_that_yields_fewer(tmp_path):
    from img_env_amd.envs import dataset_track_sets
    z = np.load(GOLDEN)
    with pytest.raises(ValueError, match="fewer"):                # the max_time cut drops pedestrians: IndexError in the reference
        dataset_track_sets(_dataset_cfg(tmp_path, z, max_time=0))
    with pytest.raises(ValueError, match="ped_traj_dataset"):
        dataset_track_sets(dict(control_hz=0.4))


def test_pack_track_sets_and_the_installed_tables():
    from img_env_amd import _cabi, spawn, worldgen
    rng = np.random.default_rng(5)
    a, b = rng.normal(size=(3, 5, 5)), rng.normal(size=(3, 2, 5))
    n, cap, pose, traj, traj_v, length = _cabi.pack_track_sets([a, (b, [1, 2, 1])], 3)
    assert (n, cap) == (2, 5) and pose.shape == (2, 3, 4) and traj.shape == (2, 3, 5, 3) and traj_v.shape == (2, 3, 5, 2)
    assert length.tolist() == [[5, 5, 5], [1, 2, 1]] and length.dtype == np.int32
    lay = spawn.init_ped_dataset(worldgen.ResetLayout(np.zeros((1, 4)), np.zeros((1, 2)), None, np.zeros((3, 2)), None, None), a)
    assert np.array_equal(pose[0], lay.ped_pose) and np.array_equal(traj[0], lay.ped_traj) and np.array_equal(traj_v[0], lay.ped_traj_v)
    assert (traj[1, :, 2:] == 0).all() and np.array_equal(traj[1, :, :2], b[:, :, :3])
    pose3, t, v, ln = tracks_model.installed_tables(pose[1], traj[1], traj_v[1], length[1])
    assert t.shape == (3, 5, 3) and (t[0, 1:] == 0).all() and (v[0, 1:] == 0).all() and np.array_equal(t[1, :2], b[1, :, :3])
    assert np.allclose(pose3[:, 2], np.arctan2(np.sin(b[:, 0, 2]), np.cos(b[:, 0, 2])))
    assert np.array_equal(v[1, :2, 2], np.arctan2(b[1, :, 4], b[1, :, 3]))
    st = tracks_model.replayed_state(pose3, t, v, ln, 4)           # min(step - 1, len - 1): a track of length 1 stands still from step 1 on
    assert np.array_equal(st[0], [b[0, 0, 0], b[0, 0, 1], b[0, 0, 3], b[0, 0, 4]]) and np.array_equal(st[1, :2], b[1, 1, :2])
    for bad in ([a[:2]], [a[:, :, :4]], [(b, [1, 3, 1])], [(b, [0, 1, 1])], []):
        with pytest.raises(ValueError):
            _cabi.pack_track_sets(bad, 3)
