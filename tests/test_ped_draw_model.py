"""The pedestrian map as a function of the pedestrian vector, on the CPU.

1. tests/ped_draw_model.py, fed the oracle's ped_vector_states, gives the oracle's ped_maps bit for bit: every robot and step of a
   small crowd scene.  The oracle draws its map from its PedInfo, not from the vector, so this is the claim the feature rests on.
2. tests/host/ped_draw_check.cpp runs the per-item functions of img_env_amd/csrc/ped_draw.h over a simulated grid on the synthetic
   rows -- 80 pedestrians at most, then 300, more than a workgroup has lanes: equal to the model bit for bit, in the ped_inv_res
   form (48 x 48) and the floor-division form (40 x 40), with 16-byte and with word stores, for every way of choosing the source rows.  The same program runs once more under AddressSanitizer and
   UndefinedBehaviorSanitizer, as a program of its own."""
import os
import subprocess

import numpy as np
import pytest

import ped_draw_model as pdm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "ped_draw_check.cpp")
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_model_on_the_oracles_vectors_equals_the_oracles_maps():
    from oracle_binding import OracleWorld
    from scenarios import random_actions, small_world
    R, P, STEPS = 3, 8, 10
    grid, params, layout = small_world(R, P, seed=21, grid_size=120, clearance=0.6, max_ped=10)
    # six pedestrians within 3 m of a robot: two around each, the others where the layout put them
    rng = np.random.default_rng(5)
    for q in range(6):
        ang, dist = rng.uniform(-np.pi, np.pi), rng.uniform(0.8, 2.2)
        layout.ped_pose[q, :2] = layout.robot_pose[q % R, :2] + dist * np.array([np.cos(ang), np.sin(ang)])
    w = OracleWorld(params, grid)
    try:
        geo = pdm.geometry(*params["ped_image_size"], params["ped_image_r"])
        snaps = [w.reset(layout)]
        snaps = [{k: np.array(snaps[0][k]) for k in ("ped_vector_states", "ped_maps")}]
        for _ in range(STEPS):
            out = w.step(random_actions(rng, R))
            snaps.append({k: np.array(out[k]) for k in ("ped_vector_states", "ped_maps")})
    finally:
        w.close()
    nonzero = 0
    for s, snap in enumerate(snaps):
        vec, maps = snap["ped_vector_states"], snap["ped_maps"]
        assert vec.shape == (R, 1 + 7 * 10) and maps.shape == (R, 3) + tuple(params["ped_image_size"])
        got = pdm.draw(vec, geo)
        for r in range(R):
            assert np.array_equal(words(got[r]), words(maps[r])), (s, r)
            nonzero += bool(words(maps[r]).any())
    print("compared", len(snaps) * R, "maps,", nonzero, "of them not all zero")
    assert nonzero > 0  # (a failure, not a skip: a scene whose robots see no pedestrian shows nothing)


# ---- the host program ----
def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + flags + [SOURCE, "-o", exe])
    return exe


def pow2(x):
    m, _ = np.frexp(x)
    return m == 0.5


def run_case(exe, tmp_path, vectors, size, mode, index=None, n=None, first=0, TR=0, grid=1, wide=1, tag="case"):
    """the program's maps for one case, float32 [n, 3, Hp, Wp]"""
    Hp, Wp, res, r, r2 = geo = pdm.geometry(size, size)
    m, PV = vectors.shape
    index = np.zeros(0, np.int32) if index is None else np.asarray(index, np.int32)
    n = (m if mode == 0 else len(index)) if n is None else n
    inv = 1.0 / res if pow2(res) else 0.0  # (create_plan.h: ped_inv_res)
    blob = (np.array([PV, Hp, Wp, m, n, mode, first, TR, grid, wide, len(index)], "<i4").tobytes() + np.array([res, inv, r, r2], "<f8").tobytes() +
            np.ascontiguousarray(vectors, "<f4").tobytes() + index.astype("<i4").tobytes())
    case, result = tmp_path / (tag + ".bin"), tmp_path / (tag + ".out")
    case.write_bytes(blob)
    out = subprocess.run([exe, str(case), str(result)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    return np.fromfile(result, "<f4").reshape(n, 3, Hp, Wp), geo


def check_cases(exe, tmp_path):
    vectors, names = pdm.synthetic_rows()
    m = len(vectors)
    for size in (48, 40):
        geo = pdm.geometry(size, size)
        assert pow2(geo[2]) == (size == 48)  # 0.125: the ped_inv_res form; 0.15: the floor division
        want = pdm.draw(vectors, geo)
        assert words(want[names.index("one disc at the centre")]).any() and not words(want[0]).any()
        for wide in (1, 0):
            got, _ = run_case(exe, tmp_path, vectors, size, 0, grid=5, wide=wide, tag="plain%d%d" % (size, wide))
            for i, name in enumerate(names):
                assert np.array_equal(words(got[i]), words(want[i])), (size, wide, name)
        # an index list with -1 and repeats: 300 maps over 7 workgroups (every workgroup strides), and one map alone
        rows = pdm.synthetic_index(m, 300)
        got, _ = run_case(exe, tmp_path, vectors, size, 1, rows, grid=7, tag="rows%d" % size)
        assert np.array_equal(words(got), words(pdm.draw(vectors, geo, rows))) and (rows < 0).any()
        got, _ = run_case(exe, tmp_path, vectors, size, 1, rows[1:2], tag="one%d" % size)
        assert np.array_equal(words(got), words(pdm.draw(vectors, geo, rows[1:2])))
        # the minibatch's order: slots first .. first + n - 1, -1 from TR on
        order = pdm.synthetic_index(m, 64, seed=9)
        got, _ = run_case(exe, tmp_path, vectors, size, 2, order, n=32, first=48, TR=64, grid=3, tag="order%d" % size)
        src = np.concatenate([order[48:64], np.full(16, -1, np.int32)])
        assert np.array_equal(words(got), words(pdm.draw(vectors, geo, src)))
    # more pedestrians than a workgroup has lanes: the lanes' further rounds
    crowd, crowd_names = pdm.crowded_rows()
    for size in (48, 40):
        got, geo = run_case(exe, tmp_path, crowd, size, 0, grid=2, tag="crowd%d" % size)
        want = pdm.draw(crowd, geo)
        for i, name in enumerate(crowd_names):
            assert np.array_equal(words(got[i]), words(want[i])), (size, name)
        assert words(want[crowd_names.index("the 300th alone in the box")]).any() and not words(want[-1]).any()
    # 96 x 96 fits the plane; a row shorter than a pedestrian holds none
    got, geo = run_case(exe, tmp_path, vectors[:12], 96, 0, grid=2, tag="p96")
    assert np.array_equal(words(got), words(pdm.draw(vectors[:12], geo)))
    short = np.array([[5.0, 0.0, 0.0, 1.0, 1.0, 0.3]], np.float32)
    got, geo = run_case(exe, tmp_path, short, 48, 0, tag="short")
    assert not words(got).any() and np.array_equal(words(got), words(pdm.draw(short, geo)))


def test_host_functions_equal_the_model(tmp_path):
    check_cases(_build(tmp_path, "ped_draw_check", []), tmp_path)


def test_host_functions_under_sanitizers(tmp_path):
    check_cases(_build(tmp_path, "ped_draw_check_san", SAN), tmp_path)


def test_count_of_the_model():
    assert [pdm.count(v, 71) for v in (0.0, 0.99, 1.0, 2.9, 10.0, 11.0, 1e30, -1.0, -0.0, np.nan, np.inf, -np.inf)] == [0, 0, 1, 2, 10, 10, 10, 0, 0, 0, 0, 0]
    assert pdm.count(5.0, 6) == 0 and pdm.count(5.0, 8) == 1
