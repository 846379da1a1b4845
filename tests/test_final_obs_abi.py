"""The final observations (imgenv_final_obs_enable / _outputs) without a GPU: the exports, the struct layouts and bits as gcc sees
include/imgenv.h against the ctypes mirror, and the refusals that need no device.  (Everything that needs a live handle -- fields the
handle does not produce, a second call with another cfg, IMGENV_ESTATE for STACKS / PED_NORM before their own enable call and for
imgenv_final_obs_outputs before the enable call -- is in tests/test_gpu_final_obs.py.)"""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("imgenv_final_obs_enable", "imgenv_final_obs_outputs")
BIT_MACROS = {"vector_states": "VECTOR_STATES", "sensor_maps": "SENSOR_MAPS", "lasers": "LASERS", "ped_vector_states": "PED_VECTOR_STATES",
              "ped_maps": "PED_MAPS", "is_collisions": "IS_COLLISIONS", "is_arrives": "IS_ARRIVES", "step_ds": "STEP_DS",
              "ped_min_dists": "PED_MIN_DISTS", "view_maps": "VIEW_MAPS", "lasers_raw": "LASERS_RAW", "stacks": "STACKS",
              "ped_vector_norm": "PED_NORM"}


@pytest.fixture(scope="module")
def hip_lib():
    from img_env_amd import _cabi
    path = _cabi.library_path()
    if not os.path.exists(path):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return _cabi.bind(C.CDLL(path))


def test_library_exports_the_final_obs_entry_points(hip_lib):
    from img_env_amd import _cabi
    header = open(os.path.join(ROOT, "include", "imgenv.h")).read()
    for f in ENTRY_POINTS:
        assert hasattr(hip_lib, f), f
        assert f in _cabi.SYMBOLS, f
        assert "int %s(" % f in header, f
    assert "#define IMGENV_ABI_VERSION 2 " in header  # new entry points only: no existing struct changed


def test_final_obs_structs_and_bits_match_the_c_layout(tmp_path):
    from img_env_amd import _cabi
    assert set(BIT_MACROS) == set(_cabi.FINAL_BITS)
    fields = {"imgenv_final_obs_cfg": ["struct_size", "fields"],
              "imgenv_final_obs_out": ["struct_size", "n_local"] + list(_cabi.FINAL_ARRAYS)}
    consts = ["IMGENV_FINAL_%s" % m for m in BIT_MACROS.values()] + ["IMGENV_FINAL_IMAGE_STATE", "IMGENV_FINAL_ALL"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "imgenv.h"', "int main(void) {"]
    for c in consts:
        lines.append('printf("%s %%d\\n", %s);' % (c, c))
    for st, fs in fields.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        for f in fs:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, f, st, f))
    lines.append("return 0; }")
    probe = tmp_path / "probe.c"
    probe.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())
    mirror = {"imgenv_final_obs_cfg": _cabi.FinalObsCfg, "imgenv_final_obs_out": _cabi.FinalObsOut}
    for st, fs in fields.items():
        assert int(got[st]) == C.sizeof(mirror[st]), st
        for f in fs:
            assert int(got["%s.%s" % (st, f)]) == getattr(mirror[st], f).offset, (st, f)
    assert C.sizeof(_cabi.FinalObsCfg) == 8
    assert C.sizeof(_cabi.FinalObsOut) == 8 + 8 * len(_cabi.FINAL_ARRAYS)
    for name, macro in BIT_MACROS.items():
        assert int(got["IMGENV_FINAL_" + macro]) == _cabi.FINAL_BITS[name], name
    bits = list(_cabi.FINAL_BITS.values())
    assert bits == [1 << k for k in range(len(bits))]  # one bit each, in the order of the names
    assert int(got["IMGENV_FINAL_ALL"]) == _cabi.FINAL_ALL == sum(bits)
    assert int(got["IMGENV_FINAL_IMAGE_STATE"]) == _cabi.FINAL_IMAGE_STATE == sum(bits[:9])
    # the first eleven names are fields of imgenv_out, with its types
    lay = _cabi.out_layout(_cabi.Out(), 0, 1, 1)
    assert all(name in lay for name in list(_cabi.FINAL_BITS)[:11])


def test_make_final_obs_cfg():
    from img_env_amd import _cabi
    c = _cabi.make_final_obs_cfg(["vector_states", "ped_maps", "ped_maps"])
    assert c.struct_size == 8 and c.fields == 1 | 16
    assert _cabi.make_final_obs_cfg(_cabi.FINAL_IMAGE_STATE).fields == 511
    with pytest.raises(ValueError):
        _cabi.make_final_obs_cfg(["vector_states", "no_such_field"])


def test_refusals_that_need_no_device(hip_lib):
    """imgenv_final_obs_enable judges its cfg before it touches the handle: a wrong struct_size and no or unknown bits are
    IMGENV_EINVAL with a message that names the field; so is a null handle or cfg"""
    from img_env_amd import _cabi
    c = _cabi.make_final_obs_cfg(_cabi.FINAL_IMAGE_STATE)
    o = _cabi.FinalObsOut()

    def refused(cfg, word):
        assert hip_lib.imgenv_final_obs_enable(None, C.byref(cfg), C.byref(o)) == _cabi.EINVAL
        assert word in hip_lib.imgenv_last_error(), (word, hip_lib.imgenv_last_error())
    refused(c, b"null")  # a good cfg: only the handle is missing
    bad = _cabi.make_final_obs_cfg(_cabi.FINAL_IMAGE_STATE)
    bad.struct_size = 12
    refused(bad, b"struct_size")
    for bits in (0, _cabi.FINAL_ALL + 1, -1, 1 << 20):
        refused(_cabi.make_final_obs_cfg(bits), b"fields")
    for bits in (1, _cabi.FINAL_ALL, _cabi.FINAL_BITS["stacks"]):
        refused(_cabi.make_final_obs_cfg(bits), b"null")  # legal bits: what they need of the handle is judged with the handle
    wrong_out = _cabi.FinalObsOut()
    wrong_out.struct_size = 4
    assert hip_lib.imgenv_final_obs_enable(None, C.byref(c), C.byref(wrong_out)) == _cabi.EINVAL
    assert hip_lib.imgenv_final_obs_enable(None, None, None) == _cabi.EINVAL
    assert hip_lib.imgenv_final_obs_outputs(None, C.byref(o)) == _cabi.EINVAL
