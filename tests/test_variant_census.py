"""Which kernel instantiations the GPU suite holds to the oracle, against which ones the launch plan can pick -- on the CPU.

tests/host/variant_census.cpp compiles the committed headers (csrc/create_plan.h, csrc/launch_plan.h) and prints, for a handle's
facts, the instantiations its chains of launches run.  Two things are asserted:

(a) the union of what the cases of tests/variant_matrix.py run equals the union over a lattice of handle facts around every
    threshold of the plan (1 / 1024 / 1025 / 4096 / 4097 / 8192 / 8193 robots; 0, 1 and 200 pedestrians; the three layers by
    their flags; power-of-two cells and not; view widths that are a multiple of four and not; LDS-bound views and not; whole
    handles, shards, several worlds; the tiled kernels) -- per kernel and per chain flag, apart from `EXCEPTIONS`;
(b) every case runs exactly the variant tuple its GPU test carries in its id (`variant_matrix.EXPECT`).

A threshold that moves in launch_plan.h fails here, instead of silently emptying a GPU case of the variant it was chosen for."""
import os
import subprocess

import pytest

import variant_matrix as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "variant_census.cpp")

# Words of the lattice no matrix case runs.  ("rule", why the C ABI cannot reach it at a test's size) or ("test", the GPU test that
# already holds the variant to the oracle, its census input) -- the second kind is checked below: the census must print the word
# for that test's shapes.  No k_view, k_raster, k_move_raster, k_remote or k_beams_big instantiation may stand here.
EXCEPTIONS = {
    "k_crop_big<1>": ("rule", "imgenv_create gives every STAMP handle whose map has fewer than 2^24 cells the map's byte-per-cell summary "
                              "(crop_map, ViewPlan::crop_sel 2); <STAMP, no summary> needs a map of 4096 x 4096 cells or more"),
    "k_raster_pack<1,2>": ("test", "tests/test_gpu_raster_pack.py::test_robots_that_move_freeze_and_enter_cells[7]"),
    "k_raster_pack<0,2>": ("test", "tests/test_gpu_raster_pack.py::test_non_power_of_two_resolution"),
    "k_obs<4>": ("test", "tests/test_gpu_parity.py::test_hip_matches_oracle[peds_200_sort4]"),
}
PROTECTED = ("k_view<", "k_raster<", "k_move_raster<", "k_remote<", "k_beams_big<")


def _exception_lines():
    """the census input of the GPU tests `EXCEPTIONS` names, built the way those tests build their handles"""
    from img_env_amd import _cabi, worldgen
    from scenarios import small_world
    from test_gpu_parity import CASES as PARITY_CASES
    lines = {}
    # test_gpu_raster_pack.py: _sum_params(n, 5, res) on make_grid(cells), IMGENV_RASTER_PACK=2 while the handle is created, every
    # step through step_begin / step_end (Trio.step)
    for word, n, res, cells in (("k_raster_pack<1,2>", 7, 0.25, 100), ("k_raster_pack<0,2>", 9, 0.1, 200)):
        params = worldgen.make_params(n, 5, res=res, view_cells=48, beams=360, scene="rvoscene", flags=_cabi.FLAG_LAYER_SUM)
        lines[word] = vm.census_line(word, params, (cells, cells), raster_pack=2, split_step=1)
    grid, params, _ = small_world(**PARITY_CASES["peds_200_sort4"])
    lines["k_obs<4>"] = vm.census_line("k_obs<4>", params, grid.shape)
    return lines


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("census") / "variant_census")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), SOURCE, "-o", exe])

    def run(lines=None):
        out = subprocess.run([exe] + ([] if lines is not None else ["--lattice"]), input="\n".join(lines or ()) + "\n",
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return out.stdout
    return run


@pytest.fixture(scope="module")
def matrix(census):
    """{handle name: {chain: [words]}} of every handle the matrix creates"""
    lines = [line for name in vm.CASES for line in vm.case_census_lines(name)]
    return vm.parse_census(census(lines))


def test_matrix_runs_every_variant_the_plan_can_pick(census, matrix):
    lattice = set(census().split())
    ran = {w for chains in matrix.values() for words in chains.values() for w in words}
    assert len([w for w in lattice if w.startswith("k_view<")]) == 32 and "k_remote<0>" in lattice  # the lattice itself is whole
    for word in EXCEPTIONS:
        assert not word.startswith(PROTECTED), "%s may not be excepted" % word
        assert word in lattice and word not in ran, "%s: a stale exception" % word
    missing = sorted(lattice - ran - set(EXCEPTIONS))
    assert not missing, "the plan can pick what no matrix case runs: %s" % missing
    assert not sorted(ran - lattice), "matrix cases run what the lattice never reaches (widen the lattice): %s" % sorted(ran - lattice)


def test_excepted_variants_run_in_the_tests_that_are_named_for_them(census):
    lines = _exception_lines()
    assert set(lines) == {w for w, (kind, _) in EXCEPTIONS.items() if kind == "test"}
    out = vm.parse_census(census(list(lines.values())))
    for word, chains in out.items():
        assert any(word in words for words in chains.values()), (word, EXCEPTIONS[word][1], chains)


def test_every_case_runs_the_variant_tuple_in_its_test_id(matrix):
    got = {name: vm.tuple_of(chains) for name, chains in matrix.items()}
    for name in vm.CASES:
        ranks = [k for k in got if k == name or k.startswith(name + "/rank")]
        assert ranks and len({got[k] for k in ranks}) == 1, (name, {k: got[k] for k in ranks})  # both ranks of a shard run the same
        assert vm.EXPECT.get(name) == got[ranks[0]], (name, got[ranks[0]])


def test_the_matrix_stays_within_its_budget_of_large_cases():
    """the oracle does ~12.7 k robot-steps/s: at most ten cases above 4096 robots, two of them above 8192; shards of 64 or fewer"""
    robots = {name: c["n_robots"] * c.get("worlds", 1) for name, c in vm.CASES.items()}
    assert sum(n > 4096 for n in robots.values()) <= 10 and sum(n > 8192 for n in robots.values()) <= 2
    assert all(robots[name] <= 64 for name, c in vm.CASES.items() if c.get("kind") == "shards")
