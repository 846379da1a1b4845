"""Action decoding and observation post-processing (imgenv_actions_* / imgenv_obs_post_*) without a GPU: the exports, the struct
layouts against gcc's, and the refusals that need no device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("imgenv_actions_enable", "imgenv_actions_outputs", "imgenv_actions_decode", "imgenv_obs_post_enable",
                "imgenv_obs_post_outputs")
TABLE8 = [[0.0, -0.9], [0.0, 0.3], [0.2, -0.6], [0.2, 0.0], [0.4, 0.6], [0.6, -0.3], [0.6, 0.0, 1], [0.6, 0.9]]


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
    for f in ENTRY_POINTS:
        assert hasattr(hip_lib, f), f
        assert f in _cabi.SYMBOLS, f
        assert "int %s(" % f in header, f
    assert "#define IMGENV_ABI_VERSION 2 " in header  # new entry points only: no existing struct changed


def test_structs_and_constants_match_the_c_layout(tmp_path):
    """sizeof / offsetof as gcc sees include/imgenv.h vs the ctypes mirrors"""
    from img_env_amd import _cabi
    import action_model
    fields = {"imgenv_actions_cfg": ["struct_size", "mode", "n_cols", "n_table", "table", "clip"],
              "imgenv_actions_out": ["struct_size", "n_local", "actions", "speeds", "n_bad"],
              "imgenv_obs_post_cfg": ["struct_size", "flags", "avg", "std", "close_dist"],
              "imgenv_obs_post_out": ["struct_size", "n_local", "ped_vector_norm", "close_to_human"]}
    consts = {"IMGENV_ACTIONS_TABLE": _cabi.ACTIONS_TABLE, "IMGENV_ACTIONS_CLIP": _cabi.ACTIONS_CLIP,
              "IMGENV_ACTIONS_MAX_TABLE": _cabi.ACTIONS_MAX_TABLE, "IMGENV_RAW_I32": _cabi.RAW_I32, "IMGENV_RAW_I64": _cabi.RAW_I64,
              "IMGENV_RAW_F32": _cabi.RAW_F32, "IMGENV_RAW_F64": _cabi.RAW_F64, "IMGENV_OBS_PED_NORM": _cabi.OBS_PED_NORM,
              "IMGENV_OBS_CLOSE": _cabi.OBS_CLOSE}
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
    mirror = {"imgenv_actions_cfg": _cabi.ActionsCfg, "imgenv_actions_out": _cabi.ActionsOut,
              "imgenv_obs_post_cfg": _cabi.ObsPostCfg, "imgenv_obs_post_out": _cabi.ObsPostOut}
    for st, fs in fields.items():
        assert int(got[st]) == C.sizeof(mirror[st]), st
        assert [f for f, _ in mirror[st]._fields_] == fs, st
        for f in fs:
            assert int(got["%s.%s" % (st, f)]) == getattr(mirror[st], f).offset, (st, f)
    for name, value in consts.items():
        assert int(got[name]) == value, name
    assert C.sizeof(_cabi.ActionsCfg) == 48 and C.sizeof(_cabi.ObsPostCfg) == 128
    assert (_cabi.ACTIONS_TABLE, _cabi.ACTIONS_CLIP) == (action_model.TABLE, action_model.CLIP)
    assert _cabi.PED_NORM_AVG == tuple(action_model.PED_NORM_AVG) and _cabi.PED_NORM_STD == tuple(action_model.PED_NORM_STD)
    assert list(_cabi.ACTION_ARRAYS) == fields["imgenv_actions_out"][2:]
    assert set(_cabi.RAW_DTYPES.values()) == {0, 1, 2, 3}


def test_make_actions_cfg_fills_the_table_and_the_ranges():
    from img_env_amd import _cabi
    import action_model
    c, keep = _cabi.make_actions_cfg(table=TABLE8)
    assert (c.mode, c.n_cols, c.n_table) == (_cabi.ACTIONS_TABLE, 2, 8) and c.table == keep.ctypes.data
    assert keep.dtype == np.float32 and (keep == action_model.table_rows(TABLE8)).all() and keep[6, 2] == 1 and keep[0, 2] == 0
    c, keep = _cabi.make_actions_cfg(clip=[[0, 0.6], [-0.9, 0.9], [-0.6, 0.6]], n_cols=2)  # the baseline YAML: three ranges, act_dim 2
    assert (c.mode, c.n_cols) == (_cabi.ACTIONS_CLIP, 2) and keep is None
    assert [list(r) for r in c.clip] == [[0.0, np.float32(0.6)], [np.float32(-0.9), np.float32(0.9)], [np.float32(-0.6), np.float32(0.6)]]
    with pytest.raises(ValueError):
        _cabi.make_actions_cfg(clip=[[0, 0.6], [-0.9, 0.9]], n_cols=3)
    with pytest.raises(ValueError):
        _cabi.make_actions_cfg(table=[[0.1]])
    p = _cabi.make_obs_post_cfg()
    assert p.flags == 3 and list(p.avg) == list(_cabi.PED_NORM_AVG) and list(p.std) == list(_cabi.PED_NORM_STD) and p.close_dist == 1.0


def test_refusals_that_need_no_device(hip_lib):
    """both enables judge their cfg before they touch the handle, so every refusal of a cfg shows with a null handle: a good cfg is
    refused for the handle ("null"), a bad one for the field the message names.  (Decode before enable / reset, a second enable
    with another cfg and indices in CLIP mode need a live handle: tests/test_gpu_actions.py.)"""
    from img_env_amd import _cabi
    ao, po = _cabi.ActionsOut(), _cabi.ObsPostOut()

    def refused(fn, cfg, out, word):
        assert fn(None, C.byref(cfg), C.byref(out)) == _cabi.EINVAL
        assert word in hip_lib.imgenv_last_error(), (word, hip_lib.imgenv_last_error())
    act = lambda cfg, word: refused(hip_lib.imgenv_actions_enable, cfg, ao, word)
    good, keep = _cabi.make_actions_cfg(table=TABLE8)
    act(good, b"null")
    bad, _ = _cabi.make_actions_cfg(table=TABLE8)
    bad.struct_size -= 4
    act(bad, b"struct_size")
    bad, _ = _cabi.make_actions_cfg(table=TABLE8)
    bad.mode = 2
    act(bad, b"mode")
    for n_cols in (0, 1, 4):
        bad, _ = _cabi.make_actions_cfg(table=TABLE8, n_cols=n_cols)
        act(bad, b"n_cols")
    bad, _ = _cabi.make_actions_cfg(table=TABLE8)
    bad.table = None
    act(bad, b"table")
    bad, _ = _cabi.make_actions_cfg(table=TABLE8)
    bad.n_table = 0
    act(bad, b"table")
    bad, _ = _cabi.make_actions_cfg(table=[[0.0, 0.0]] * 4097)
    act(bad, b"table")
    ok, k2 = _cabi.make_actions_cfg(table=[[0.0, 0.0]] * 4096)
    act(ok, b"null")
    for v in (float("nan"), float("inf")):
        bad, k3 = _cabi.make_actions_cfg(table=[[0.0, 0.1], [0.2, v]])
        act(bad, b"not finite")
    act(_cabi.make_actions_cfg(clip=[[0, 0.6], [-0.9, 0.9]])[0], b"null")
    act(_cabi.make_actions_cfg(clip=[[0, 0.6], [-0.9, -0.9]])[0], b"null")  # the shipped YAMLs' own (lo == hi is legal)
    act(_cabi.make_actions_cfg(clip=[[0.6, 0], [-0.9, 0.9]])[0], b"clip[0]")
    act(_cabi.make_actions_cfg(clip=[[0, 0.6], [-0.9, float("inf")]])[0], b"clip[1]")
    act(_cabi.make_actions_cfg(clip=[[0, 0.6], [float("nan"), 0.9]])[0], b"clip[1]")
    act(_cabi.make_actions_cfg(clip=[[0, 0.6], [-0.9, 0.9], [1, 0]], n_cols=2)[0], b"null")  # (a range beyond n_cols is not read)
    act(_cabi.make_actions_cfg(clip=[[0, 0.6], [-0.9, 0.9], [1, 0]], n_cols=3)[0], b"clip[2]")
    assert hip_lib.imgenv_actions_enable(None, None, None) == _cabi.EINVAL
    assert hip_lib.imgenv_actions_outputs(None, C.byref(ao)) == _cabi.EINVAL
    assert hip_lib.imgenv_actions_decode(None, None, 0, None) == _cabi.EINVAL

    post = lambda cfg, word: refused(hip_lib.imgenv_obs_post_enable, cfg, po, word)
    post(_cabi.make_obs_post_cfg(), b"null")
    bad = _cabi.make_obs_post_cfg()
    bad.struct_size += 8
    post(bad, b"struct_size")
    post(_cabi.make_obs_post_cfg(ped_norm=False, close=False), b"flags")
    bad = _cabi.make_obs_post_cfg()
    bad.flags = 4
    post(bad, b"flags")
    std = list(_cabi.PED_NORM_STD)
    std[3] = 0.0
    post(_cabi.make_obs_post_cfg(std=std), b"std[3] is 0")
    std[3] = float("nan")
    post(_cabi.make_obs_post_cfg(std=std), b"not finite")
    avg = list(_cabi.PED_NORM_AVG)
    avg[6] = float("inf")
    post(_cabi.make_obs_post_cfg(avg=avg), b"not finite")
    post(_cabi.make_obs_post_cfg(ped_norm=False, std=[0.0] * 7), b"null")  # (constants of a part that is off are not read)
    post(_cabi.make_obs_post_cfg(close_dist=float("nan")), b"close_dist")
    assert hip_lib.imgenv_obs_post_enable(None, None, None) == _cabi.EINVAL
    assert hip_lib.imgenv_obs_post_outputs(None, C.byref(po)) == _cabi.EINVAL
