"""The episode statistics (imgenv_episodes_enable / _outputs / _clear) without a GPU: the exports, the struct layouts and the
refusals that need no device."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("imgenv_episodes_enable", "imgenv_episodes_outputs", "imgenv_episodes_clear")


@pytest.fixture(scope="module")
def hip_lib():
    from img_env_amd import _cabi
    path = _cabi.library_path()
    if not os.path.exists(path):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return _cabi.bind(C.CDLL(path))


def test_library_exports_the_episode_entry_points(hip_lib):
    from img_env_amd import _cabi
    for f in ENTRY_POINTS:
        assert hasattr(hip_lib, f), f
        assert f in _cabi.SYMBOLS, f
    header = open(os.path.join(ROOT, "include", "imgenv.h")).read()
    for f in ENTRY_POINTS:
        assert "int %s(" % f in header, f
    assert "#define IMGENV_ABI_VERSION 2 " in header  # new entry points only: no existing struct changed


def test_episode_structs_match_the_c_layout(tmp_path):
    """sizeof / offsetof as gcc sees include/imgenv.h vs the ctypes mirror; the row constants vs the names Python gives the rows"""
    from img_env_amd import _cabi
    import episode_model
    fields = {"imgenv_episodes_cfg": ["struct_size", "min_steps", "dt"],
              "imgenv_episodes_out": ["struct_size", "n_local"] + list(_cabi.EPISODE_ARRAYS)}
    consts = ["IMGENV_EP_ARRIVE", "IMGENV_EP_TIMEOUT", "IMGENV_EP_COLLISION", "IMGENV_EP_ABORTED", "IMGENV_EP_END_BINS", "IMGENV_EP_FIGURES",
              "IMGENV_EP_OPEN_F64"]
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
    mirror = {"imgenv_episodes_cfg": _cabi.EpisodesCfg, "imgenv_episodes_out": _cabi.EpisodesOut}
    for st, fs in fields.items():
        assert int(got[st]) == C.sizeof(mirror[st]), st
        for f in fs:
            assert int(got["%s.%s" % (st, f)]) == getattr(mirror[st], f).offset, (st, f)
    assert C.sizeof(_cabi.EpisodesCfg) == 16 and len(_cabi.EPISODE_ARRAYS) == 19
    assert int(got["IMGENV_EP_END_BINS"]) == _cabi.EP_END_BINS == len(_cabi.EP_ENDS) == len(episode_model.ENDS)
    assert int(got["IMGENV_EP_FIGURES"]) == _cabi.EP_FIGURES == len(_cabi.EP_FIGURE_NAMES)
    assert int(got["IMGENV_EP_OPEN_F64"]) == _cabi.EP_OPEN_F64 == len(_cabi.EP_OPEN_NAMES)
    assert _cabi.EP_ENDS == episode_model.ENDS and _cabi.EP_FIGURE_NAMES == episode_model.FIGURES and _cabi.EP_OPEN_NAMES == episode_model.OPEN_F64
    ends = _cabi.EP_ENDS
    assert ends[int(got["IMGENV_EP_ARRIVE"])] == "arrive" and ends[int(got["IMGENV_EP_TIMEOUT"])] == "timeout"
    assert ends[int(got["IMGENV_EP_COLLISION"])] == "static_collision" and ends[int(got["IMGENV_EP_ABORTED"])] == "aborted"
    assert _cabi.EPISODE_ARRAYS["ends"][1] == _cabi.EP_END_BINS and _cabi.EPISODE_ARRAYS["figure_sums"][1] == _cabi.EP_FIGURES
    assert _cabi.EPISODE_ARRAYS["open_f64"][1] == _cabi.EP_OPEN_F64


def test_refusals_that_need_no_device(hip_lib):
    """imgenv_episodes_enable judges its cfg before it touches the handle: a wrong struct_size, dt <= 0 (or not a number) and
    min_steps < 0 are IMGENV_EINVAL with a message that names the field; so is a null handle or cfg.  (The second enable with another
    cfg needs a live handle: tests/test_gpu_episodes.py.)"""
    from img_env_amd import _cabi
    c = _cabi.make_episodes_cfg(3, 0.25)
    assert c.struct_size == 16 and c.min_steps == 3 and c.dt == 0.25
    o = _cabi.EpisodesOut()

    def refused(cfg, word):
        assert hip_lib.imgenv_episodes_enable(None, C.byref(cfg), C.byref(o)) == _cabi.EINVAL
        assert word in hip_lib.imgenv_last_error(), (word, hip_lib.imgenv_last_error())
    refused(c, b"null")  # a good cfg: only the handle is missing
    bad = _cabi.make_episodes_cfg(3, 0.25)
    bad.struct_size = 12
    refused(bad, b"struct_size")
    for dt in (0.0, -0.25, float("nan"), float("inf")):
        refused(_cabi.make_episodes_cfg(3, dt), b"dt")
    refused(_cabi.make_episodes_cfg(-1, 0.25), b"min_steps")
    refused(_cabi.make_episodes_cfg(0, 0.25), b"null")  # min_steps 0 is legal
    assert hip_lib.imgenv_episodes_enable(None, None, None) == _cabi.EINVAL
    assert hip_lib.imgenv_episodes_outputs(None, C.byref(o)) == _cabi.EINVAL
    assert hip_lib.imgenv_episodes_clear(None, None) == _cabi.EINVAL
