"""Every kernel instantiation the launch plan can pick, against the oracle, on unfriendly geometry.

The cases are the table of tests/variant_matrix.py: one small world per variant tuple -- `k_view<pow2, a4, stamp, nw>`, the raster
kernel and its `<pow2, layer, nw>` (or the packed raster), the fused move against `k_integrate` with the gated early `k_obs`, split /
roomy / shared raster blocks, `k_remote<pow2>` of robot shards, the tiled kernels -- chosen from the census of
tests/host/variant_census.cpp so that the table's union is everything the plan can reach (tests/test_variant_census.py, on the
CPU, keeps both true).  The test id carries the tuple.

Each case: a reset, 6 steps of random actions (lateral speeds where the robots are omni), a reset of the listed worlds where the
handle holds several, 3 more steps; every EXACT and CLOSE field of tests/parity.py after every call, with its tolerances.  Then
  - the episode exercised what it is there for, by the ORACLE's snapshots alone (variant_matrix.Exercise): robots ran into each
    other and into an obstacle or pedestrian, a view holds another robot's cells (with a laser: a beam ends on them), and at least
    5 % of the robots change grid cell in every step;
  - the handle took the path the census says: imgenv_timing_read's launch counts over the last 3 steps."""
import pytest

import variant_matrix as vm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def worlds():
    import torch
    assert torch.cuda.is_available()
    from img_env_amd.world import World
    from oracle_binding import OracleWorld, build_oracle
    build_oracle()
    return World, OracleWorld


@pytest.mark.parametrize("name", list(vm.CASES), ids=[vm.case_id(n) for n in vm.CASES])
def test_variant_matches_oracle(worlds, name):
    World, OracleWorld = worlds
    case = vm.CASES[name]
    fails, seen, timing = vm.run_case(name, OracleWorld, World)
    assert not fails, fails[:3]
    assert not vm.missing(seen), vm.missing(seen)
    layer = "COMPOSED" if "COMPOSED" in vm.EXPECT[name] else "STAMP" if "STAMP" in vm.EXPECT[name] else "SUM" if "SUM" in vm.EXPECT[name] else None
    for t in timing:
        counts = {k: v[1] for k, v in t.items()}
        fused = "fuse_move=1" in vm.EXPECT[name].split("; ")[0]
        n = vm.STEPS_B
        # K_MOVE_RASTER against K_INTEGRATE + K_RASTER: the move was fused exactly where the census says
        assert counts["k_move_raster"] == (n if fused else 0), (name, counts)
        assert counts["k_integrate"] == (0 if fused else n) and counts["k_raster"] == (0 if fused else n), (name, counts)
        # K_COMPOSE runs in every step exactly on the composed layer (the stamped layer's sweep comes once in 255 steps)
        if layer is not None:
            assert (counts["k_compose"] == n) == (layer == "COMPOSED"), (name, layer, counts)
        # the tiled kernels on big views, and the shrunk sensor_map's taps where the view is resized
        big = "k_crop_big<" in vm.EXPECT[name]
        assert counts["k_crop_big"] == (n if big else 0) and counts["k_view"] == n, (name, counts)
        assert counts["k_taps_big"] == (n if big and case.get("image") else 0), (name, counts)
        # k_remote behind the exchange of a robot shard on the counting layer
        assert counts["k_remote"] == (n if "k_remote<" in vm.EXPECT[name] else 0), (name, counts)
