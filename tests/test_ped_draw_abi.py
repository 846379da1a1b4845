"""Pedestrian maps drawn from pedestrian vectors (imgenv_ped_maps_draw, IMGENV_ROLLOUT_PED_MAPS_DRAWN) without a GPU: the export,
the constants and struct sizes as gcc sees include/imgenv.h against the ctypes mirror, the refusals that need no device, and the
field plan -- tests/host/ped_draw_plan_check.cpp compiles feature_plan.h, obs_fields.h and launch_plan.h for the host: the two
illegal combinations, no ring slot and one minibatch slot for the drawn field, the rank plane's limit.  (Everything that needs a
live handle is in tests/test_gpu_ped_draw.py.)"""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "ped_draw_plan_check.cpp")


@pytest.fixture(scope="module")
def hip_lib():
    from img_env_amd import _cabi
    path = _cabi.library_path()
    if not os.path.exists(path):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return _cabi.bind(C.CDLL(path))


def test_library_exports_the_entry_point(hip_lib):
    from img_env_amd import _cabi
    header = open(os.path.join(ROOT, "include", "imgenv.h")).read()
    assert hasattr(hip_lib, "imgenv_ped_maps_draw") and "imgenv_ped_maps_draw" in _cabi.SYMBOLS
    assert "int imgenv_ped_maps_draw(imgenv_t* h, const float* ped_vectors, const int32_t* rows, int64_t n, float* out, void* stream);" in header
    assert hip_lib.imgenv_ped_maps_draw.argtypes[3] == C.c_int64
    assert "#define IMGENV_ABI_VERSION 2 " in header and hip_lib.imgenv_abi_version() == 2


def test_the_bit_and_what_stays_as_it_was(tmp_path):
    from img_env_amd import _cabi
    consts = ["IMGENV_ROLLOUT_PED_MAPS_DRAWN", "IMGENV_ROLLOUT_ALL", "IMGENV_ROLLOUT_NORM_STATES", "IMGENV_ROLLOUT_NORM_REWARDS", "IMGENV_K_COUNT",
              "IMGENV_ABI_VERSION"]
    structs = {"imgenv_rollout_cfg": _cabi.RolloutCfg, "imgenv_rollout_out": _cabi.RolloutOut, "imgenv_minibatch_cfg": _cabi.MinibatchCfg,
               "imgenv_minibatch_buffer": _cabi.MinibatchBuffer, "imgenv_minibatch_out": _cabi.MinibatchOut, "imgenv_minibatch_args": _cabi.MinibatchArgs}
    lines = ['#include <stdio.h>', '#include "imgenv.h"', "int main(void) {"]
    lines += ['printf("%s %%d\\n", (int)%s);' % (c, c) for c in consts]
    lines += ['printf("%s %%zu\\n", sizeof(%s));' % (st, st) for st in structs]
    lines.append("return 0; }")
    probe, exe = tmp_path / "probe.c", tmp_path / "probe"
    probe.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)])
    got = {k: int(v) for k, v in (ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())}
    assert got["IMGENV_ROLLOUT_PED_MAPS_DRAWN"] == _cabi.ROLLOUT_PED_MAPS_DRAWN == 512
    assert got["IMGENV_ROLLOUT_ALL"] == _cabi.ROLLOUT_ALL == 127 and not _cabi.ROLLOUT_ALL & 512
    assert (got["IMGENV_ROLLOUT_NORM_STATES"], got["IMGENV_ROLLOUT_NORM_REWARDS"]) == (_cabi.ROLLOUT_NORM_STATES, _cabi.ROLLOUT_NORM_REWARDS) == (128, 256)
    assert got["IMGENV_ABI_VERSION"] == 2 and got["IMGENV_K_COUNT"] == _cabi.K_COUNT == 14
    for st, mirror in structs.items():  # no struct grew: the drawn maps land in the buffers' existing mb_ped_maps
        assert got[st] == C.sizeof(mirror), st
    assert C.sizeof(_cabi.RolloutOut) == 24 + 8 * (2 * 9 + 9) and C.sizeof(_cabi.MinibatchBuffer) == 8 * (9 + 7)
    # the names: the first five of ROLLOUT_BITS are the single-frame fields, in their order; the new name is accepted wherever names are
    assert list(_cabi.ROLLOUT_BITS)[:5] == ["sensor_maps", "vector_states", "lasers", "ped_vector_states", "ped_maps"]
    assert sum(_cabi.ROLLOUT_BITS.values()) == _cabi.ROLLOUT_ALL
    assert _cabi.make_rollout_cfg(4, 4, ["ped_vector_states", "ped_maps_drawn"]).fields == 8 | 512
    assert _cabi.make_minibatch_cfg(4, 1, ["ped_maps_drawn"]).fields == 512
    assert (_cabi.PED_DRAW_BLOCK, _cabi.PED_DRAW_MAX_BLOCKS, _cabi.PED_DRAW_LDS_BYTES) == (256, 2048, 65536)
    plan = open(os.path.join(ROOT, "img_env_amd", "csrc", "launch_plan.h")).read()
    for name in ("PED_DRAW_BLOCK", "PED_DRAW_MAX_BLOCKS", "PED_DRAW_LDS_BYTES"):
        assert "#define %s %d " % (name, getattr(_cabi, name)) in plan, name


def test_refusals_that_need_no_device(hip_lib):
    from img_env_amd import _cabi
    assert hip_lib.imgenv_ped_maps_draw(None, None, None, 0, None, None) == _cabi.EINVAL
    assert hip_lib.imgenv_ped_maps_draw(None, 256, None, 4, 512, None) == _cabi.EINVAL and b"null" in hip_lib.imgenv_last_error()
    o = _cabi.RolloutOut()

    def refused(bits, word):
        assert hip_lib.imgenv_rollout_enable(None, C.byref(_cabi.make_rollout_cfg(8, 8, bits)), C.byref(o)) == _cabi.EINVAL
        assert word in hip_lib.imgenv_last_error(), (word, hip_lib.imgenv_last_error())
    refused(["ped_vector_states", "ped_maps_drawn"], b"null")  # a good cfg: only the handle is missing
    refused(["ped_vector_states", "ped_maps", "ped_maps_drawn"], b"excludes IMGENV_ROLLOUT_PED_MAPS")
    refused(["sensor_maps", "ped_maps_drawn"], b"needs IMGENV_ROLLOUT_PED_VECTOR_STATES")
    refused(["ped_maps_drawn"], b"fields 512")
    mo = _cabi.MinibatchOut()
    assert hip_lib.imgenv_rollout_minibatch_enable(None, C.byref(_cabi.make_minibatch_cfg(8, 1, ["ped_maps_drawn"])), C.byref(mo)) == _cabi.EINVAL
    assert b"null" in hip_lib.imgenv_last_error()


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-Wall", "-Werror"] + flags + [SOURCE, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    return out.stdout.split()


def test_field_plan_of_the_drawn_maps(tmp_path):
    assert int(_build_and_run(tmp_path, "ped_draw_plan_check", [])[1]) > 80


def test_field_plan_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "ped_draw_plan_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
