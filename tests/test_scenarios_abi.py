"""The scenario bank's entry points (imgenv_scenarios_* / imgenv_scenario_for_placement / imgenv_reset_worlds_scenarios /
imgenv_world_scenarios) without a GPU: the exports, the constants and the prototypes against gcc's reading of include/imgenv.h, the
refusals that need no handle, and the host half of imgenv_scenarios_add (csrc/scenario_bank.h) as a stand-alone program under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPES = {
    "imgenv_scenarios_add": "int (*%s)(imgenv_t*, int32_t, int32_t, const double*, const double*, const double*, const double*, const double*, "
                            "const int32_t*, const int32_t*, const float*, const double*)",
    "imgenv_scenarios_policy": "int (*%s)(imgenv_t*, int32_t, uint64_t, void*)",
    "imgenv_scenario_for_placement": "int32_t (*%s)(int32_t, uint64_t, uint64_t, uint64_t, int32_t)",
    "imgenv_reset_worlds_scenarios": "int (*%s)(imgenv_t*, int32_t, const int32_t*, const int32_t*, void*)",
    "imgenv_world_scenarios": "int (*%s)(imgenv_t*, int32_t*, void*)",
}


@pytest.fixture(scope="module")
def hip_lib():
    from img_env_amd import _cabi
    path = _cabi.library_path()
    if not os.path.exists(path):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return _cabi.bind(C.CDLL(path))


def test_library_exports_the_entry_points(hip_lib):
    from img_env_amd import _cabi
    header = open(os.path.join(ROOT, "include", "imgenv.h")).read()
    for f in PROTOTYPES:
        assert hasattr(hip_lib, f), f
        assert f in _cabi.SYMBOLS, f
        assert " %s(" % f in header, f
    assert "#define IMGENV_ABI_VERSION 2 " in header  # new entry points only: no existing struct changed
    assert "imgenv_step_autoreset, the HOST-side auto-reset, keeps sampling" in header  # said where the policy is declared


def test_constants_and_prototypes_match_the_header(tmp_path):
    """gcc reads include/imgenv.h: the policy constants, and every prototype assigned to a pointer of the type the Python
    bindings assume (-Werror: a changed parameter does not compile)"""
    from img_env_amd import _cabi
    consts = {"IMGENV_SCENARIOS_OFF": _cabi.SCENARIOS_OFF, "IMGENV_SCENARIOS_QUEUE": _cabi.SCENARIOS_QUEUE,
              "IMGENV_SCENARIOS_BY_PLACEMENT": _cabi.SCENARIOS_BY_PLACEMENT}
    lines = ['#include "imgenv.h"']
    for k, (f, proto) in enumerate(PROTOTYPES.items()):
        lines.append("%s = %s;" % (proto % ("p%d" % k), f))
    probe = tmp_path / "probe.c"
    probe.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-Wno-unused-variable", "-c", "-I", os.path.join(ROOT, "include"), str(probe), "-o",
                           str(tmp_path / "probe.o")])
    lines = ['#include "imgenv.h"'] + ["value_of_%s=%s" % (c.lower(), c) for c in consts]
    (tmp_path / "consts.c").write_text("\n".join(lines))
    out = subprocess.check_output(["gcc", "-E", "-P", "-I", os.path.join(ROOT, "include"), str(tmp_path / "consts.c")]).decode()
    got = dict(ln.replace(" ", "").split("=") for ln in out.splitlines() if ln.startswith("value_of_"))
    assert {k[len("value_of_"):].upper(): int(v) for k, v in got.items()} == consts
    assert _cabi.SCENARIO_POLICIES == {"off": 0, "queue": 1, "placement": 2}
    lib = _cabi.bind(C.CDLL(_cabi.library_path()))
    assert [len(getattr(lib, f).argtypes) for f in PROTOTYPES] == [12, 4, 5, 5, 3]
    assert lib.imgenv_scenario_for_placement.restype is C.c_int32
    # the slot limits the Python side repeats
    slot = open(os.path.join(ROOT, "img_env_amd", "csrc", "spawn_slot.h")).read()
    assert "#define SPAWN_MAX_AGENTS %d " % _cabi.SPAWN_MAX_AGENTS in slot and "#define SPAWN_MAX_OBST %d " % _cabi.SPAWN_MAX_OBST in slot


def test_refusals_that_need_no_handle(hip_lib):
    from img_env_amd import _cabi
    buf = (C.c_int32 * 4)()
    assert hip_lib.imgenv_scenarios_add(None, 1, 0, *([None] * 9)) == _cabi.EINVAL
    assert b"null" in hip_lib.imgenv_last_error()
    assert hip_lib.imgenv_scenarios_policy(None, _cabi.SCENARIOS_QUEUE, 0, None) == _cabi.EINVAL
    assert hip_lib.imgenv_reset_worlds_scenarios(None, 1, buf, buf, None) == _cabi.EINVAL
    assert hip_lib.imgenv_world_scenarios(None, buf, None) == _cabi.EINVAL
    u = C.c_uint64
    assert hip_lib.imgenv_scenario_for_placement(_cabi.SCENARIOS_QUEUE, u(1), u(2), u(3), 0) == -1
    assert hip_lib.imgenv_scenario_for_placement(_cabi.SCENARIOS_OFF, u(1), u(2), u(3), 5) == -1
    assert hip_lib.imgenv_scenario_for_placement(7, u(1), u(2), u(3), 5) == -1
    assert hip_lib.imgenv_scenario_for_placement(_cabi.SCENARIOS_QUEUE, u(1), u(2), u(3), 1) == 0
    assert hip_lib.imgenv_scenario_for_placement(_cabi.SCENARIOS_BY_PLACEMENT, u(1), u(2), u(3), 1) == 0


def test_record_scenarios_is_the_spawn_by_seed():
    """spawn.record_scenarios(cfg, n, seed): placement k is native_spawn(cfg, seed + k), byte for byte (no device needed)"""
    import numpy as np
    from img_env_amd import _cabi, spawn, worldgen
    cfg = worldgen.make_yaml_cfg(2, 3, worldgen.make_grid(200, 3), n_obstacles=2, seed=9)
    lays = spawn.record_scenarios(cfg, 4, 100)
    assert len(lays) == 4
    a, b = _cabi.pack_scenarios(lays, 2, 3, 2), _cabi.pack_scenarios([spawn.native_spawn(cfg, 100 + k) for k in range(4)], 2, 3, 2)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    assert not np.array_equal(a["robot_pose"][0], a["robot_pose"][1])


def test_host_conversion_under_the_sanitizers(tmp_path):
    """a stand-alone program with its own main: good banks (trajectory lengths 0, 1 and 2, a one-entry bank without pedestrians
    and obstacles) and every kind of bad bank (NaN pose, zero quaternion, ped_traj_len 3, shape 9, ...)"""
    exe = str(tmp_path / "scenario_bank_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "scenario_bank_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
