"""PPO's loss (imgenv_policy_loss_*) without a GPU: the exports, the struct layouts and constants against gcc's, the refusals that
need no device, and that the ABI version and the timing registry stayed as they were."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("imgenv_policy_loss_enable", "imgenv_policy_loss_outputs", "imgenv_policy_loss")


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
    assert "#define IMGENV_ABI_VERSION 2 " in header and hip_lib.imgenv_abi_version() == 2  # new entry points only
    assert "#define IMGENV_K_COUNT 14" in header and _cabi.K_COUNT == 14  # the new kernels are not in the timing registry
    hip_lib.imgenv_kernel_name.restype = C.c_char_p
    assert hip_lib.imgenv_kernel_name(13) and not hip_lib.imgenv_kernel_name(14)


def test_structs_and_constants_match_the_c_layout(tmp_path):
    """sizeof / offsetof as gcc sees include/imgenv.h vs the ctypes mirrors"""
    from img_env_amd import _cabi
    fields = {"imgenv_policy_loss_cfg": ["struct_size", "max_rows", "reserved"],
              "imgenv_policy_loss_out": ["struct_size", "n_params", "max_rows", "reserved", "logp", "entropy", "ratio", "pg", "vl", "d_params",
                                         "d_log_std", "d_log_std_shared", "d_values", "stats", "n_bad", "inv_w"],
              "imgenv_policy_loss_args": ["struct_size", "flags", "rows", "reserved", "params", "log_std", "values", "action", "old_logp",
                                          "old_value", "adv", "ret", "weight", "clip", "clip_vf", "vf_coef", "ent_coef"]}
    consts = {"IMGENV_PLOSS_CLIP_VALUE": _cabi.PLOSS_CLIP_VALUE, "IMGENV_POLICY_LOG_STD_PER_ROW": _cabi.POLICY_LOG_STD_PER_ROW,
              "IMGENV_MB_MAX_SCALARS": _cabi.MB_MAX_SCALARS}
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
    mirror = {"imgenv_policy_loss_cfg": _cabi.PolicyLossCfg, "imgenv_policy_loss_out": _cabi.PolicyLossOut,
              "imgenv_policy_loss_args": _cabi.PolicyLossArgs}
    for st, fs in fields.items():
        assert int(got[st]) == C.sizeof(mirror[st]), st
        assert [f for f, _ in mirror[st]._fields_] == fs, st
        for f in fs:
            assert int(got["%s.%s" % (st, f)]) == getattr(mirror[st], f).offset, (st, f)
    for name, value in consts.items():
        assert int(got[name]) == value, name
    assert (C.sizeof(_cabi.PolicyLossCfg), C.sizeof(_cabi.PolicyLossOut), C.sizeof(_cabi.PolicyLossArgs)) == (16, 112, 120)
    assert list(_cabi.PLOSS_ARRAYS) == fields["imgenv_policy_loss_out"][4:]
    assert _cabi.PLOSS_CLIP_VALUE & _cabi.POLICY_LOG_STD_PER_ROW == 0 and _cabi.MB_MAX_SCALARS == 6


def test_refusals_that_need_no_device(hip_lib):
    """the enable judges its cfg before it touches the handle: a good cfg is refused for the handle ("null"), a bad one for the
    field the message names.  (ESTATE before imgenv_policy_enable, a second enable with another max_rows and the refusals of
    imgenv_policy_loss's arguments need a live handle: tests/test_gpu_policy_loss.py.)"""
    from img_env_amd import _cabi
    lo = _cabi.PolicyLossOut()

    def refused(cfg, word, out=lo):
        assert hip_lib.imgenv_policy_loss_enable(None, C.byref(cfg), C.byref(out)) == _cabi.EINVAL
        assert word in hip_lib.imgenv_last_error(), (word, hip_lib.imgenv_last_error())
    refused(_cabi.make_policy_loss_cfg(4096), b"null")
    bad = _cabi.make_policy_loss_cfg(8)
    bad.struct_size += 4
    refused(bad, b"struct_size")
    refused(_cabi.make_policy_loss_cfg(0), b"max_rows")
    bad = _cabi.make_policy_loss_cfg(8)
    bad.reserved[1] = 1
    refused(bad, b"reserved")
    wrong = _cabi.PolicyLossOut()
    wrong.struct_size = 8
    refused(_cabi.make_policy_loss_cfg(8), b"imgenv_policy_loss_out.struct_size", out=wrong)
    assert hip_lib.imgenv_policy_loss_enable(None, None, None) == _cabi.EINVAL
    assert hip_lib.imgenv_policy_loss_outputs(None, C.byref(lo)) == _cabi.EINVAL
    assert hip_lib.imgenv_policy_loss(None, None, None) == _cabi.EINVAL
    args = _cabi.PolicyLossArgs()
    assert hip_lib.imgenv_policy_loss(None, C.byref(args), None) == _cabi.EINVAL
