"""The map bank without a GPU (include/imgenv.h, "map bank"): the draw ``imgenv_map_for_placement`` -- a pure function of the
library, called through ctypes -- the Python symbol list, and ``config.load_map`` for one map and for several."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def draw():
    from img_env_amd import _cabi
    path = _cabi.library_path()
    if not os.path.exists(path):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(path)
    lib.imgenv_map_for_placement.argtypes = [C.c_uint64, C.c_int32]
    lib.imgenv_map_for_placement.restype = C.c_int32
    return lambda seed, n: int(lib.imgenv_map_for_placement(C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), n))


SEEDS = list(range(300)) + [2 ** 31 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1, 0x9E3779B97F4A7C15, 0x9E3779B97F4A7C15 + (1 << 63)]


@pytest.mark.parametrize("n_maps", [1, 2, 3, 7, 4096])
def test_draw_is_in_range_and_deterministic(draw, n_maps):
    first = [draw(s, n_maps) for s in SEEDS]
    assert all(0 <= m < n_maps for m in first)
    assert first == [draw(s, n_maps) for s in SEEDS]
    if n_maps == 1:
        assert set(first) == {0}


def test_draw_matches_its_documented_definition(draw):
    """splitmix64's finaliser over the seed, the upper 32 bits scaled into [0, n) by multiply-shift: integers only, so a trainer
    can restate it in any language"""
    M = (1 << 64) - 1

    def model(seed, n):
        if n <= 1:
            return 0
        z = (seed + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        z ^= z >> 31
        return ((z >> 32) * n) >> 32

    for n in (1, 2, 3, 7, 8, 4096, 2 ** 31 - 1):
        assert [draw(s, n) for s in SEEDS] == [model(s, n) for s in SEEDS], n


@pytest.mark.parametrize("n_maps", [2, 3, 8])
def test_every_map_is_drawn(draw, n_maps):
    seen = {draw(s, n_maps) for s in range(64 * n_maps)}
    assert seen == set(range(n_maps))


def test_python_symbol_list_names_the_new_functions():
    from img_env_amd import _cabi
    for f in ("imgenv_maps_add", "imgenv_world_maps_set", "imgenv_maps_policy", "imgenv_map_for_placement", "imgenv_world_maps"):
        assert f in _cabi.SYMBOLS
    assert _cabi.MAP_POLICIES == {"keep": 0, "placement": 1}


def test_python_draw_needs_no_device(draw):
    from img_env_amd import _cabi
    assert [_cabi.map_for_placement(s, 5) for s in SEEDS] == [draw(s, 5) for s in SEEDS]


def test_load_map_returns_a_stack_for_a_list_and_the_map_for_a_string(tmp_path):
    from PIL import Image
    from img_env_amd import config
    maps = []
    for k in range(3):
        m = np.full((40, 50), 255, np.uint8)
        m[:4] = 0
        m[10 + 5 * k:14 + 5 * k, 20:30] = 0
        maps.append(m)
        Image.fromarray(m if k != 1 else np.stack([m] * 3, -1)).save(str(tmp_path / ("m%d.png" % k)))  # (one grey-in-RGB file)
    one = config.load_map({"map_dir": str(tmp_path), "global_map": {"map_file": "m1.png"}})
    assert one.shape == (40, 50) and one.dtype == np.uint8 and np.array_equal(one, maps[1])
    many = config.load_map({"map_dir": str(tmp_path), "global_map": {"map_file": ["m0.png", "m1.png", "m2.png"]}})
    assert many.shape == (3, 40, 50) and many.dtype == np.uint8 and many.flags["C_CONTIGUOUS"]
    for k in range(3):
        assert np.array_equal(many[k], maps[k])
    # in-memory maps: 2-D stays 2-D, 3-D / a list of 2-D arrays is the stack
    assert config.load_map({"global_map": {"map_array": maps[0]}}).shape == (40, 50)
    assert np.array_equal(config.load_map({"global_map": {"map_array": np.stack(maps)}}), many)
    assert np.array_equal(config.load_map({"global_map": {"map_array": maps}}), many)
    with pytest.raises(ValueError, match="one size"):
        config.load_map({"global_map": {"map_array": [maps[0], maps[1][:30]]}})
