"""bench.py's `--dump-outputs`: what it writes (names, dtypes, exact values, the fixed robot sample, the 64 MB bound) and its
command line, on host arrays shaped like imgenv_out -- no GPU."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class FakeWorld:
    """what dump_outputs reads of a World: n_local and snapshot()"""

    def __init__(self, R, view, ped_hw, peds, seed=0):
        rng = np.random.default_rng(seed)
        self.n_local = R
        self.arrays = {
            "view_maps": rng.integers(0, 256, (R, view, view), dtype=np.uint8),
            "sensor_maps": rng.random((R, view, view)).astype(np.float16),
            "ped_maps": rng.random((R, 3, ped_hw, ped_hw), dtype=np.float32),
            "lasers": rng.random((R, 360)),
            "is_collisions": rng.integers(-1, 4, R, dtype=np.int8),
            "base_rewards": rng.integers(-5, 5, R, dtype=np.int32),
            "rewards": rng.random(R),
            "ped_state": rng.random((peds, 4)),
            "counters": np.array([7, 0, 3, 123456789], np.int32),
        }

    def snapshot(self):
        return {k: v.copy() for k, v in self.arrays.items()}


def _dump(world, d):
    bench.dump_outputs(world, str(d))
    return {f[:-4]: np.load(os.path.join(str(d), f)) for f in os.listdir(str(d))}


def test_dump_writes_every_output_exactly_as_float(tmp_path):
    w = FakeWorld(2048, 48, 48, 200)
    got = _dump(w, tmp_path)
    assert set(got) == set(w.arrays) | {"sample_robots"}
    sample = got["sample_robots"].astype(np.int64)
    assert len(sample) == bench.DUMP_ROBOTS and np.all(np.diff(sample) > 0) and sample[-1] < 2048
    for name, a in w.arrays.items():
        g = got[name]
        assert g.dtype in (np.float32, np.float64), name
        ref = a[sample] if g.shape[0] != a.shape[0] else a
        assert g.shape == ref.shape, name
        assert np.array_equal(g, ref.astype(g.dtype)) and np.array_equal(g.astype(a.dtype), ref), name
    # int32 (counters can pass 2^24) is widened to float64, not float32
    assert got["counters"].dtype == np.float64 and got["counters"][3] == 123456789
    # small per-robot arrays are written whole
    assert got["rewards"].shape == (2048,) and got["ped_state"].shape == (200, 4)


def test_dump_is_the_same_sample_every_run(tmp_path):
    a = _dump(FakeWorld(2048, 48, 48, 200, seed=1), tmp_path / "a")
    b = _dump(FakeWorld(2048, 48, 48, 200, seed=1), tmp_path / "b")
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_dump_stays_under_64_mb_for_large_views(tmp_path):
    # cfg-5-like: 96 x 96 views and ped maps, where 512 robots of the large arrays would not fit
    _dump(FakeWorld(1024, 96, 96, 1000), tmp_path)
    total = sum(os.path.getsize(os.path.join(str(tmp_path), f)) for f in os.listdir(str(tmp_path)))
    assert total <= 64 << 20
    assert 0 < len(np.load(os.path.join(str(tmp_path), "sample_robots.npy"))) < bench.DUMP_ROBOTS


def test_bench_cli_has_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in out.stdout, opt
