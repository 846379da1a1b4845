"""The track bank's entry points (imgenv_tracks_* / imgenv_world_tracks*) without a GPU: the exports, the constants and the
prototypes against gcc's reading of include/imgenv.h, the refusals that need no device, and the host half of imgenv_tracks_add
(csrc/track_bank.h: tracks_convert_set) as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPES = {
    "imgenv_tracks_add": "int (*%s)(imgenv_t*, int32_t, int32_t, const double*, const double*, const double*, const int32_t*)",
    "imgenv_world_tracks_set": "int (*%s)(imgenv_t*, int32_t, const int32_t*, const int32_t*, void*)",
    "imgenv_tracks_policy": "int (*%s)(imgenv_t*, int32_t, int32_t)",
    "imgenv_tracks_for_placement": "int32_t (*%s)(uint64_t, int32_t)",
    "imgenv_world_tracks": "int (*%s)(imgenv_t*, int32_t*, void*)",
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
    assert "sys.exit()" in header                      # the CYCLE policy's deviation from the reference is stated where it is declared


def test_constants_and_prototypes_match_the_header(tmp_path):
    """gcc reads include/imgenv.h: the policy constants, and every prototype assigned to a pointer of the type the Python
    bindings assume (-Werror: a changed parameter does not compile)"""
    from img_env_amd import _cabi
    consts = {"IMGENV_TRACKS_KEEP": _cabi.TRACKS_KEEP, "IMGENV_TRACKS_BY_PLACEMENT": _cabi.TRACKS_BY_PLACEMENT,
              "IMGENV_TRACKS_CYCLE": _cabi.TRACKS_CYCLE}
    lines = ['#include <stdio.h>', '#include "imgenv.h"']
    for k, (f, proto) in enumerate(PROTOTYPES.items()):
        lines.append("%s = %s;" % (proto % ("p%d" % k), f))
    lines.append("int main(void) {")
    for c in consts:
        lines.append('printf("%s %%d\\n", %s);' % (c, c))
    lines.append("return 0; }")
    probe = tmp_path / "probe.c"
    probe.write_text("\n".join(lines))
    obj = tmp_path / "probe.o"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-Wno-unused-variable", "-c", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(obj)])
    # (the constants through the preprocessor alone: linking would need the library)
    lines = ['#include "imgenv.h"'] + ["value_of_%s=%s" % (c.lower(), c) for c in consts]
    (tmp_path / "consts.c").write_text("\n".join(lines))
    out = subprocess.check_output(["gcc", "-E", "-P", "-I", os.path.join(ROOT, "include"), str(tmp_path / "consts.c")]).decode()
    got = dict(ln.replace(" ", "").split("=") for ln in out.splitlines() if ln.startswith("value_of_"))
    assert {k[len("value_of_"):].upper(): int(v) for k, v in got.items()} == consts
    assert _cabi.TRACK_POLICIES == {"keep": 0, "placement": 1, "cycle": 2}
    lib = _cabi.bind(C.CDLL(_cabi.library_path()))
    assert [len(getattr(lib, f).argtypes) for f in PROTOTYPES] == [7, 5, 3, 2, 3]
    assert lib.imgenv_tracks_for_placement.restype is C.c_int32


def test_refusals_that_need_no_device(hip_lib):
    from img_env_amd import _cabi
    buf = (C.c_int32 * 4)()
    assert hip_lib.imgenv_tracks_add(None, 1, 1, None, None, None, None) == _cabi.EINVAL
    assert b"null" in hip_lib.imgenv_last_error()
    assert hip_lib.imgenv_world_tracks_set(None, 1, buf, buf, None) == _cabi.EINVAL
    assert hip_lib.imgenv_tracks_policy(None, _cabi.TRACKS_CYCLE, 1) == _cabi.EINVAL
    assert hip_lib.imgenv_world_tracks(None, buf, None) == _cabi.EINVAL
    assert hip_lib.imgenv_tracks_for_placement(C.c_uint64(123), 0) == 0 and hip_lib.imgenv_tracks_for_placement(C.c_uint64(123), 1) == 0


def test_host_conversion_under_the_sanitizers(tmp_path):
    """a stand-alone program with its own main: odd Pw * stride, tracks of length 1, junk behind the lengths, the refusals"""
    exe = str(tmp_path / "track_bank_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "track_bank_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
