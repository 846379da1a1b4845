"""The episode log (imgenv_episode_log_enable / _outputs / _read) without a GPU: the exports, the struct layouts and the refusals that
need no device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("imgenv_episode_log_enable", "imgenv_episode_log_outputs", "imgenv_episode_log_read")
RECORD_FIELDS = ["seq", "placement", "robot", "world", "code", "steps", "len", "counted", "episode", "map", "tracks", "scenario", "ep_return",
                 "figures"]


@pytest.fixture(scope="module")
def hip_lib():
    from img_env_amd import _cabi
    path = _cabi.library_path()
    if not os.path.exists(path):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return _cabi.bind(C.CDLL(path))


def test_library_exports_the_episode_log_entry_points(hip_lib):
    from img_env_amd import _cabi
    header = open(os.path.join(ROOT, "include", "imgenv.h")).read()
    for f in ENTRY_POINTS:
        assert hasattr(hip_lib, f), f
        assert f in _cabi.SYMBOLS, f
        assert " %s(" % f in header, f
    assert "int64_t imgenv_episode_log_read(" in header
    assert "#define IMGENV_ABI_VERSION 2 " in header  # new entry points only: no existing struct changed


def test_episode_log_structs_match_the_c_layout(tmp_path):
    """sizeof / offsetof as gcc sees include/imgenv.h vs the ctypes mirrors and the numpy record dtype; the row constants vs the names
    Python and the model give the rows"""
    from img_env_amd import _cabi
    import episode_log_model
    fields = {"imgenv_episode_log_cfg": ["struct_size", "capacity"],
              "imgenv_episode_log_out": ["struct_size", "capacity"] + list(_cabi.EPISODE_LOG_ARRAYS),
              "imgenv_episode_record": RECORD_FIELDS}
    consts = ["IMGENV_EPLOG_MAX_CAPACITY", "IMGENV_EPLOG_I32", "IMGENV_EPLOG_F64", "IMGENV_EPLOG_SCN_DEVICE", "IMGENV_EP_FIGURES"]
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
    mirror = {"imgenv_episode_log_cfg": _cabi.EpisodeLogCfg, "imgenv_episode_log_out": _cabi.EpisodeLogOut,
              "imgenv_episode_record": _cabi.EpisodeRecord}
    for st, fs in fields.items():
        assert int(got[st]) == C.sizeof(mirror[st]), st
        for f in fs:
            assert int(got["%s.%s" % (st, f)]) == getattr(mirror[st], f).offset, (st, f)
    assert int(got["imgenv_episode_record"]) == 128 == C.sizeof(_cabi.EpisodeRecord) == _cabi.EPISODE_RECORD_DTYPE.itemsize
    assert C.sizeof(_cabi.EpisodeLogCfg) == 8
    for f in RECORD_FIELDS:
        assert _cabi.EPISODE_RECORD_DTYPE.fields[f][1] == getattr(_cabi.EpisodeRecord, f).offset, f
    assert _cabi.EPISODE_RECORD_DTYPE["figures"].shape == (int(got["IMGENV_EP_FIGURES"]),)
    assert int(got["IMGENV_EPLOG_MAX_CAPACITY"]) == _cabi.EPLOG_MAX_CAPACITY == 1 << 22
    assert int(got["IMGENV_EPLOG_I32"]) == _cabi.EPLOG_I32 == len(_cabi.EPLOG_I32_NAMES) == 10
    assert int(got["IMGENV_EPLOG_F64"]) == _cabi.EPLOG_F64 == len(_cabi.EPLOG_F64_NAMES) == 9
    assert int(got["IMGENV_EPLOG_SCN_DEVICE"]) == _cabi.EPLOG_SCN_DEVICE == episode_log_model.SCN_DEVICE == -2
    assert _cabi.EPLOG_I32_NAMES == episode_log_model.I32_NAMES and _cabi.EPLOG_F64_NAMES == episode_log_model.F64_NAMES
    assert _cabi.EPISODE_LOG_ARRAYS["i32"][1] == _cabi.EPLOG_I32 and _cabi.EPISODE_LOG_ARRAYS["f64"][1] == _cabi.EPLOG_F64
    assert np.uint64(episode_log_model.NONE64) == np.uint64(0xFFFFFFFFFFFFFFFF)


def test_refusals_that_need_no_device(hip_lib):
    """imgenv_episode_log_enable judges its cfg before it touches the handle: a wrong struct_size and a capacity outside
    1 .. IMGENV_EPLOG_MAX_CAPACITY are IMGENV_EINVAL with a message that names the field; so is a null handle or cfg.  (The order
    against imgenv_episodes_enable and the second call need a live handle: tests/test_gpu_episode_log.py.)"""
    from img_env_amd import _cabi
    c = _cabi.make_episode_log_cfg(100)
    assert c.struct_size == 8 and c.capacity == 100
    o = _cabi.EpisodeLogOut()

    def refused(cfg, word):
        assert hip_lib.imgenv_episode_log_enable(None, C.byref(cfg), C.byref(o)) == _cabi.EINVAL
        assert word in hip_lib.imgenv_last_error(), (word, hip_lib.imgenv_last_error())
    refused(c, b"null")  # a good cfg: only the handle is missing
    bad = _cabi.make_episode_log_cfg(100)
    bad.struct_size = 12
    refused(bad, b"struct_size")
    for cap in (0, -1, _cabi.EPLOG_MAX_CAPACITY + 1):
        refused(_cabi.make_episode_log_cfg(cap), b"capacity")
    for cap in (1, _cabi.EPLOG_MAX_CAPACITY):
        refused(_cabi.make_episode_log_cfg(cap), b"null")  # both ends of the range are legal
    wrong_out = _cabi.EpisodeLogOut()
    wrong_out.struct_size = 4
    assert hip_lib.imgenv_episode_log_enable(None, C.byref(c), C.byref(wrong_out)) == _cabi.EINVAL
    assert hip_lib.imgenv_episode_log_enable(None, None, None) == _cabi.EINVAL
    assert hip_lib.imgenv_episode_log_outputs(None, C.byref(o)) == _cabi.EINVAL
    assert hip_lib.imgenv_episode_log_read(None, 0, 0, None, None, None, None) == _cabi.EINVAL
