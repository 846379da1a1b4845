"""The policy head (imgenv_policy_*) without a GPU: the exports, the struct layouts and constants against gcc's, and the refusals
that need no device."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("imgenv_policy_enable", "imgenv_policy_outputs", "imgenv_policy_sample")


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
    hip_lib.imgenv_kernel_name.restype = C.c_char_p
    assert hip_lib.imgenv_kernel_name(5) == b"k_view" and hip_lib.imgenv_kernel_name(6) == b"k_obs"


def test_structs_and_constants_match_the_c_layout(tmp_path):
    """sizeof / offsetof as gcc sees include/imgenv.h vs the ctypes mirrors"""
    from img_env_amd import _cabi
    fields = {"imgenv_policy_cfg": ["struct_size", "kind", "flags", "reserved", "seed"],
              "imgenv_policy_out": ["struct_size", "n_local", "n_params", "horizon", "index", "raw", "logp", "entropy", "pol_raw",
                                    "pol_logp", "pol_value"],
              "imgenv_policy_args": ["struct_size", "flags", "draw", "params", "log_std", "values"]}
    consts = {"IMGENV_POLICY_CATEGORICAL": _cabi.POLICY_CATEGORICAL, "IMGENV_POLICY_GAUSSIAN": _cabi.POLICY_GAUSSIAN,
              "IMGENV_POLICY_STORE": _cabi.POLICY_STORE, "IMGENV_POLICY_DETERMINISTIC": _cabi.POLICY_DETERMINISTIC,
              "IMGENV_POLICY_LOG_STD_PER_ROW": _cabi.POLICY_LOG_STD_PER_ROW, "IMGENV_POLICY_NO_STORE": _cabi.POLICY_NO_STORE,
              "IMGENV_POLICY_VALUE_ONLY": _cabi.POLICY_VALUE_ONLY}
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
    mirror = {"imgenv_policy_cfg": _cabi.PolicyCfg, "imgenv_policy_out": _cabi.PolicyOut, "imgenv_policy_args": _cabi.PolicyArgs}
    for st, fs in fields.items():
        assert int(got[st]) == C.sizeof(mirror[st]), st
        assert [f for f, _ in mirror[st]._fields_] == fs, st
        for f in fs:
            assert int(got["%s.%s" % (st, f)]) == getattr(mirror[st], f).offset, (st, f)
    for name, value in consts.items():
        assert int(got[name]) == value, name
    assert (C.sizeof(_cabi.PolicyCfg), C.sizeof(_cabi.PolicyOut), C.sizeof(_cabi.PolicyArgs)) == (24, 72, 40)
    assert list(_cabi.POLICY_ARRAYS) == fields["imgenv_policy_out"][4:]


def test_make_policy_cfg():
    from img_env_amd import _cabi
    c = _cabi.make_policy_cfg("categorical", seed=(5 << 32) | 7, store=True)
    assert (c.struct_size, c.kind, c.flags, c.reserved, c.seed) == (24, 0, 1, 0, (5 << 32) | 7)
    c = _cabi.make_policy_cfg("gaussian", seed=-1)
    assert (c.kind, c.flags, c.seed) == (1, 0, 2 ** 64 - 1)


def test_refusals_that_need_no_device(hip_lib):
    """the enable judges its cfg before it touches the handle, so every refusal of a cfg shows with a null handle: a good cfg is
    refused for the handle ("null"), a bad one for the field the message names.  (The ESTATE paths -- before imgenv_actions_enable,
    STORE before imgenv_rollout_enable, a sample before the first reset or outside the window -- and a second enable with another
    cfg need a live handle: tests/test_gpu_policy.py.)"""
    from img_env_amd import _cabi
    po = _cabi.PolicyOut()

    def refused(cfg, word, out=po):
        assert hip_lib.imgenv_policy_enable(None, C.byref(cfg), C.byref(out)) == _cabi.EINVAL
        assert word in hip_lib.imgenv_last_error(), (word, hip_lib.imgenv_last_error())
    refused(_cabi.make_policy_cfg("categorical", 1), b"null")
    refused(_cabi.make_policy_cfg("gaussian", 1, store=True), b"null")
    bad = _cabi.make_policy_cfg("categorical")
    bad.struct_size += 8
    refused(bad, b"struct_size")
    bad = _cabi.make_policy_cfg("categorical")
    bad.kind = 2
    refused(bad, b"kind")
    bad = _cabi.make_policy_cfg("categorical")
    bad.flags = 2
    refused(bad, b"flags")
    bad = _cabi.make_policy_cfg("categorical")
    bad.reserved = 1
    refused(bad, b"reserved")
    wrong = _cabi.PolicyOut()
    wrong.struct_size = 8
    refused(_cabi.make_policy_cfg("categorical"), b"imgenv_policy_out.struct_size", out=wrong)
    assert hip_lib.imgenv_policy_enable(None, None, None) == _cabi.EINVAL
    assert hip_lib.imgenv_policy_outputs(None, C.byref(po)) == _cabi.EINVAL
    assert hip_lib.imgenv_policy_sample(None, None, None) == _cabi.EINVAL
    args = _cabi.PolicyArgs()
    assert hip_lib.imgenv_policy_sample(None, C.byref(args), None) == _cabi.EINVAL
