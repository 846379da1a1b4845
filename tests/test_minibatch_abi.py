"""The rollout minibatches (imgenv_rollout_minibatch_enable / _outputs, imgenv_rollout_index / _stats / _shuffle / _minibatch)
without a GPU: the exports, the struct layouts and constants as gcc sees include/imgenv.h against the ctypes mirror, and the
refusals that need no device.  (Everything that needs a live handle -- a bit the rollout does not store, a second call with another
cfg, IMGENV_ESTATE before imgenv_rollout_enable, the stale generation -- is in tests/test_gpu_minibatch.py.)"""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("imgenv_rollout_minibatch_enable", "imgenv_rollout_minibatch_outputs", "imgenv_rollout_index", "imgenv_rollout_stats",
                "imgenv_rollout_shuffle", "imgenv_rollout_minibatch")


@pytest.fixture(scope="module")
def hip_lib():
    from img_env_amd import _cabi
    path = _cabi.library_path()
    if not os.path.exists(path):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return _cabi.bind(C.CDLL(path))


def test_library_exports_the_minibatch_entry_points(hip_lib):
    from img_env_amd import _cabi
    header = open(os.path.join(ROOT, "include", "imgenv.h")).read()
    for f in ENTRY_POINTS:
        assert hasattr(hip_lib, f), f
        assert f in _cabi.SYMBOLS, f
        assert "int %s(" % f in header, f
    assert "#define IMGENV_ABI_VERSION 2 " in header  # new entry points only: no existing struct changed
    assert hip_lib.imgenv_abi_version() == 2
    assert "int imgenv_rollout_stats(imgenv_t* h, const float* x, double eps, float* norm_out, void* stream);" in header
    assert "int imgenv_rollout_shuffle(imgenv_t* h, uint32_t seed_lo, uint32_t seed_hi, void* stream);" in header
    assert hip_lib.imgenv_rollout_stats.argtypes[2] == C.c_double
    assert hip_lib.imgenv_rollout_shuffle.argtypes[1:3] == [C.c_uint32, C.c_uint32]
    assert "population variance" in header.lower()  # (not torch's unbiased default: the header says so)


def test_minibatch_structs_and_constants_match_the_c_layout(tmp_path):
    from img_env_amd import _cabi
    buffer_fields = ["mb_" + n for n in _cabi.ROLLOUT_FIELDS] + list(_cabi.MB_SCALARS)
    fields = {"imgenv_minibatch_cfg": ["struct_size", "batch", "buffers", "fields"],
              "imgenv_minibatch_buffer": buffer_fields,
              "imgenv_minibatch_out": list(_cabi.MB_HEADER) + list(_cabi.MB_ARRAYS) + ["buf"],
              "imgenv_minibatch_args": ["struct_size", "j", "buffer", "n_scalars", "normalise", "reserved", "scalars", "norm"],
              "imgenv_rollout_cfg": ["struct_size", "horizon", "final_capacity", "fields"]}
    consts = ["IMGENV_MB_MAX_SCALARS", "IMGENV_MB_MAX_BUFFERS", "IMGENV_ROLLOUT_ALL", "IMGENV_K_COUNT", "IMGENV_ABI_VERSION"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "imgenv.h"', "int main(void) {"]
    for c in consts:
        lines.append('printf("%s %%d\\n", (int)%s);' % (c, c))
    lines.append('printf("imgenv_rollout_out %zu\\n", sizeof(imgenv_rollout_out));')
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
    mirror = {"imgenv_minibatch_cfg": _cabi.MinibatchCfg, "imgenv_minibatch_buffer": _cabi.MinibatchBuffer, "imgenv_minibatch_out": _cabi.MinibatchOut,
              "imgenv_minibatch_args": _cabi.MinibatchArgs, "imgenv_rollout_cfg": _cabi.RolloutCfg}
    for st, fs in fields.items():
        assert int(got[st]) == C.sizeof(mirror[st]), st
        assert [name for name, _ in mirror[st]._fields_] == fs, st
        for f in fs:
            assert int(got["%s.%s" % (st, f)]) == getattr(mirror[st], f).offset, (st, f)
    assert int(got["IMGENV_MB_MAX_SCALARS"]) == _cabi.MB_MAX_SCALARS == 6
    assert int(got["IMGENV_MB_MAX_BUFFERS"]) == _cabi.MB_MAX_BUFFERS == 4
    assert C.sizeof(_cabi.MinibatchCfg) == 16
    assert C.sizeof(_cabi.MinibatchBuffer) == 8 * (len(_cabi.ROLLOUT_FIELDS) + len(_cabi.MB_SCALARS))
    assert C.sizeof(_cabi.MinibatchOut) == 24 + 8 * len(_cabi.MB_ARRAYS) + 4 * C.sizeof(_cabi.MinibatchBuffer)
    assert C.sizeof(_cabi.MinibatchArgs) == 24 + 8 * 6 + 8
    # what stays exactly as it was
    assert int(got["IMGENV_ABI_VERSION"]) == 2 and int(got["IMGENV_K_COUNT"]) == _cabi.K_COUNT == 14
    assert int(got["imgenv_rollout_out"]) == C.sizeof(_cabi.RolloutOut) == 24 + 8 * (2 * len(_cabi.ROLLOUT_FIELDS) + len(_cabi.ROLLOUT_SCALARS))
    assert int(got["IMGENV_ROLLOUT_ALL"]) == _cabi.ROLLOUT_ALL


def test_make_minibatch_cfg_and_args():
    from img_env_amd import _cabi
    c = _cabi.make_minibatch_cfg(4096, 2, ["vector_states", "ped_maps", "ped_maps"])
    assert (c.struct_size, c.batch, c.buffers, c.fields) == (16, 4096, 2, 2 | 16)
    assert _cabi.make_minibatch_cfg(8).fields == 0 and _cabi.make_minibatch_cfg(8, 1, None).fields == 0  # 0: every field of the rollout
    with pytest.raises(ValueError):
        _cabi.make_minibatch_cfg(8, 1, ["no_such_field"])
    a = _cabi.make_minibatch_args(3, 1, [256, 512], 1, 768)
    assert (a.struct_size, a.j, a.buffer, a.n_scalars, a.normalise, a.reserved) == (C.sizeof(_cabi.MinibatchArgs), 3, 1, 2, 1, 0)
    assert list(a.scalars) == [256, 512, None, None, None, None] and a.norm == 768


def test_refusals_that_need_no_device(hip_lib):
    """imgenv_rollout_minibatch_enable judges its cfg before it touches the handle: a wrong struct_size, batch < 1, buffers 0 and 5
    and unknown bits are IMGENV_EINVAL with a message that names the field; so is a null handle or cfg, in every entry point"""
    from img_env_amd import _cabi
    o = _cabi.MinibatchOut()

    def refused(cfg, word):
        assert hip_lib.imgenv_rollout_minibatch_enable(None, C.byref(cfg), C.byref(o)) == _cabi.EINVAL
        assert word in hip_lib.imgenv_last_error(), (word, hip_lib.imgenv_last_error())
    refused(_cabi.make_minibatch_cfg(8, 1, 3), b"null")  # a good cfg: only the handle is missing
    refused(_cabi.make_minibatch_cfg(8, 4, 0), b"null")
    bad = _cabi.make_minibatch_cfg(8, 1, 3)
    bad.struct_size = 12
    refused(bad, b"struct_size")
    for batch in (0, -1):
        refused(_cabi.make_minibatch_cfg(batch, 1, 3), b"batch")
    for buffers in (0, 5, -1):
        refused(_cabi.make_minibatch_cfg(8, buffers, 3), b"buffers")
    for bits in (_cabi.ROLLOUT_ALL + 1, -1, 1 << 20):
        refused(_cabi.make_minibatch_cfg(8, 1, bits), b"fields")
    wrong_out = _cabi.MinibatchOut()
    wrong_out.struct_size = 4
    assert hip_lib.imgenv_rollout_minibatch_enable(None, C.byref(_cabi.make_minibatch_cfg(8, 1, 3)), C.byref(wrong_out)) == _cabi.EINVAL
    assert hip_lib.imgenv_rollout_minibatch_enable(None, None, None) == _cabi.EINVAL
    assert hip_lib.imgenv_rollout_minibatch_outputs(None, C.byref(o)) == _cabi.EINVAL
    assert hip_lib.imgenv_rollout_index(None, None) == _cabi.EINVAL
    assert hip_lib.imgenv_rollout_stats(None, None, 1e-8, None, None) == _cabi.EINVAL
    assert hip_lib.imgenv_rollout_shuffle(None, 1, 2, None) == _cabi.EINVAL
    assert hip_lib.imgenv_rollout_minibatch(None, None, None) == _cabi.EINVAL

    def args_refused(a, word):
        assert hip_lib.imgenv_rollout_minibatch(None, C.byref(a), None) == _cabi.EINVAL
        assert word in hip_lib.imgenv_last_error(), (word, hip_lib.imgenv_last_error())
    args_refused(_cabi.make_minibatch_args(0, 0, [256]), b"null")  # good args: only the handle is missing
    a = _cabi.make_minibatch_args(0)
    a.struct_size = 8
    args_refused(a, b"struct_size")
    args_refused(_cabi.make_minibatch_args(-1), b".j")
    a = _cabi.make_minibatch_args(0)
    a.n_scalars = 7
    args_refused(a, b"n_scalars")
    args_refused(_cabi.make_minibatch_args(0, 0, [256], 1), b"normalise")
    args_refused(_cabi.make_minibatch_args(0, 0, [256], -2), b"normalise")
    args_refused(_cabi.make_minibatch_args(0, 0, [256, 0]), b"scalars[1]")
