"""k_view's first hits over live beams only (the one-wavefront launches: more than 4096 robots) against the oracle on worlds
where the beams get far: robots a few metres apart on a large map, so that many beams walk every chunk of their path, some
hit on chunk boundaries and the robots near the border see out-of-map cells and walls.  A reset, then steps; view_maps,
sensor_maps and the collision flags bit-exact, lasers at the parity suite's tolerance."""
import os
import sys

import numpy as np
import pytest

from parity import CLOSE, EXACT, compare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(900)
@pytest.mark.parametrize("grid_size,clearance,n_peds", [(1000, 1.5, 0), (600, 1.0, 50)])
def test_sparse_worlds_match_oracle(grid_size, clearance, n_peds):
    import torch
    assert torch.cuda.is_available()
    from img_env_amd import worldgen
    from img_env_amd.world import World
    from oracle_binding import OracleWorld, build_oracle
    build_oracle()
    n, res = 4608, 0.25
    grid = worldgen.make_grid(grid_size, 0)
    layout = worldgen.make_layout(grid, res, n, n_peds, seed=5, clearance=clearance)
    params = worldgen.make_params(n, n_peds, res=res, view_cells=48, beams=360, scene="rvoscene" if n_peds else "")
    gpu, cpu = World(params, grid), OracleWorld(params, grid)
    try:
        rng = np.random.default_rng(3)
        gpu.reset(layout)
        cpu.reset(layout)
        bad = compare(gpu.snapshot(), cpu.snapshot(), EXACT + CLOSE)
        assert not bad, ("reset", bad)
        for s in range(4):
            a = np.stack([np.zeros(n), rng.uniform(-0.9, 0.9, n), np.zeros(n)], 1).astype(np.float32)
            gpu.step(a)
            cpu.step(a)
            bad = compare(gpu.snapshot(), cpu.snapshot(), EXACT + CLOSE)
            assert not bad, ("step %d" % s, bad)
        lasers = cpu.snapshot()["lasers"]
        assert (lasers >= 0.999).mean() > 0.05  # beams that reach their end without a hit: the walk's every chunk
    finally:
        gpu.close()
        cpu.close()
