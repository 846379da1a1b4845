"""The rollout storage (imgenv_rollout_enable / _outputs / _begin / _gae) without a GPU: the exports, the struct layouts and bits as
gcc sees include/imgenv.h against the ctypes mirror, and the refusals that need no device.  (Everything that needs a live handle --
fields the handle does not produce, a second call with another cfg, IMGENV_ESTATE for STACKS / PED_NORM before their own enable
call, begin before the first reset, the full ring -- is in tests/test_gpu_rollout.py.)"""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("imgenv_rollout_enable", "imgenv_rollout_outputs", "imgenv_rollout_begin", "imgenv_rollout_gae")
BIT_MACROS = {"sensor_maps": "SENSOR_MAPS", "vector_states": "VECTOR_STATES", "lasers": "LASERS", "ped_vector_states": "PED_VECTOR_STATES",
              "ped_maps": "PED_MAPS", "ped_vector_norm": "PED_NORM", "stacks": "STACKS"}


@pytest.fixture(scope="module")
def hip_lib():
    from img_env_amd import _cabi
    path = _cabi.library_path()
    if not os.path.exists(path):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return _cabi.bind(C.CDLL(path))


def test_library_exports_the_rollout_entry_points(hip_lib):
    from img_env_amd import _cabi
    header = open(os.path.join(ROOT, "include", "imgenv.h")).read()
    for f in ENTRY_POINTS:
        assert hasattr(hip_lib, f), f
        assert f in _cabi.SYMBOLS, f
        assert "int %s(" % f in header, f
    assert "#define IMGENV_ABI_VERSION 2 " in header  # new entry points only: no existing struct changed
    assert ("int imgenv_rollout_gae(imgenv_t* h, const float* values, const float* final_values, float gamma, float lam, float* adv, "
            "float* ret, void* stream);") in header
    assert hip_lib.imgenv_rollout_gae.argtypes[3:5] == [C.c_float, C.c_float]


def test_rollout_structs_and_bits_match_the_c_layout(tmp_path):
    from img_env_amd import _cabi
    assert list(BIT_MACROS) == list(_cabi.ROLLOUT_BITS)
    out_fields = (list(_cabi.ROLLOUT_HEADER) + ["obs_" + n for n in _cabi.ROLLOUT_FIELDS] + ["final_" + n for n in _cabi.ROLLOUT_FIELDS] +
                  list(_cabi.ROLLOUT_SCALARS))
    fields = {"imgenv_rollout_cfg": ["struct_size", "horizon", "final_capacity", "fields"], "imgenv_rollout_out": out_fields}
    consts = ["IMGENV_ROLLOUT_%s" % m for m in BIT_MACROS.values()] + ["IMGENV_ROLLOUT_ALL"]
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
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())
    mirror = {"imgenv_rollout_cfg": _cabi.RolloutCfg, "imgenv_rollout_out": _cabi.RolloutOut}
    for st, fs in fields.items():
        assert int(got[st]) == C.sizeof(mirror[st]), st
        assert [name for name, _ in mirror[st]._fields_] == fs, st
        for f in fs:
            assert int(got["%s.%s" % (st, f)]) == getattr(mirror[st], f).offset, (st, f)
    assert C.sizeof(_cabi.RolloutCfg) == 16
    assert C.sizeof(_cabi.RolloutOut) == 24 + 8 * (2 * len(_cabi.ROLLOUT_FIELDS) + len(_cabi.ROLLOUT_SCALARS))
    for name, macro in BIT_MACROS.items():
        assert int(got["IMGENV_ROLLOUT_" + macro]) == _cabi.ROLLOUT_BITS[name], name
    bits = list(_cabi.ROLLOUT_BITS.values())
    assert bits == [1 << k for k in range(len(bits))]  # one bit each, in the order of the names
    assert int(got["IMGENV_ROLLOUT_ALL"]) == _cabi.ROLLOUT_ALL == sum(bits)
    # the five single-frame fields are fields of imgenv_out, with its types
    lay = _cabi.out_layout(_cabi.Out(), 0, 1, 1)
    assert all(name in lay for name in _cabi.ROLLOUT_FIELDS[:5])


def test_make_rollout_cfg():
    from img_env_amd import _cabi
    c = _cabi.make_rollout_cfg(128, 64, ["vector_states", "ped_maps", "ped_maps"])
    assert (c.struct_size, c.horizon, c.final_capacity, c.fields) == (16, 128, 64, 2 | 16)
    assert _cabi.make_rollout_cfg(1, 1, _cabi.ROLLOUT_ALL).fields == 127
    with pytest.raises(ValueError):
        _cabi.make_rollout_cfg(1, 1, ["vector_states", "no_such_field"])


def test_refusals_that_need_no_device(hip_lib):
    """imgenv_rollout_enable judges its cfg before it touches the handle: a wrong struct_size, a horizon or a final capacity below
    1 and no or unknown bits are IMGENV_EINVAL with a message that names the field; so is a null handle or cfg"""
    from img_env_amd import _cabi
    o = _cabi.RolloutOut()

    def refused(cfg, word):
        assert hip_lib.imgenv_rollout_enable(None, C.byref(cfg), C.byref(o)) == _cabi.EINVAL
        assert word in hip_lib.imgenv_last_error(), (word, hip_lib.imgenv_last_error())
    refused(_cabi.make_rollout_cfg(8, 8, 3), b"null")  # a good cfg: only the handle is missing
    bad = _cabi.make_rollout_cfg(8, 8, 3)
    bad.struct_size = 12
    refused(bad, b"struct_size")
    for horizon in (0, -1):
        refused(_cabi.make_rollout_cfg(horizon, 8, 3), b"horizon")
    for cap in (0, -5):
        refused(_cabi.make_rollout_cfg(8, cap, 3), b"final_capacity")
    for bits in (0, _cabi.ROLLOUT_ALL + 1, -1, 1 << 20):
        refused(_cabi.make_rollout_cfg(8, 8, bits), b"fields")
    for bits in (1, _cabi.ROLLOUT_ALL, _cabi.ROLLOUT_BITS["stacks"]):
        refused(_cabi.make_rollout_cfg(8, 8, bits), b"null")  # legal bits: what they need of the handle is judged with the handle
    wrong_out = _cabi.RolloutOut()
    wrong_out.struct_size = 4
    assert hip_lib.imgenv_rollout_enable(None, C.byref(_cabi.make_rollout_cfg(8, 8, 3)), C.byref(wrong_out)) == _cabi.EINVAL
    assert hip_lib.imgenv_rollout_enable(None, None, None) == _cabi.EINVAL
    assert hip_lib.imgenv_rollout_outputs(None, C.byref(o)) == _cabi.EINVAL
    assert hip_lib.imgenv_rollout_begin(None, None) == _cabi.EINVAL
    assert hip_lib.imgenv_rollout_gae(None, None, None, 0.5, 0.5, None, None, None) == _cabi.EINVAL
