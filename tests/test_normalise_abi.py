"""The running normalisation (imgenv_normalise_enable / _outputs / _training / _stats_get / _stats_set) without a GPU: the exports,
the struct layouts and bits as gcc sees include/imgenv.h against the ctypes mirror, that no struct of an earlier feature changed, and
the refusals that need no device.  (Everything that needs a live handle is in tests/test_gpu_normalise.py.)"""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("imgenv_normalise_enable", "imgenv_normalise_outputs", "imgenv_normalise_training", "imgenv_normalise_stats_get",
                "imgenv_normalise_stats_set")


@pytest.fixture(scope="module")
def hip_lib():
    from img_env_amd import _cabi
    path = _cabi.library_path()
    if not os.path.exists(path):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return _cabi.bind(C.CDLL(path))


def test_library_exports_the_normalise_entry_points(hip_lib):
    from img_env_amd import _cabi
    header = open(os.path.join(ROOT, "include", "imgenv.h")).read()
    for f in ENTRY_POINTS:
        assert hasattr(hip_lib, f), f
        assert f in _cabi.SYMBOLS, f
        assert "int %s(" % f in header, f
    assert "#define IMGENV_ABI_VERSION 2 " in header  # new entry points and new bits only: no existing struct changed


def test_structs_and_bits_match_the_c_layout(tmp_path):
    from img_env_amd import _cabi
    mirror = {"imgenv_normalise_cfg": _cabi.NormaliseCfg, "imgenv_normalise_out": _cabi.NormaliseOut, "imgenv_normalise_stats": _cabi.NormaliseStats,
              # the structs of the features whose storage the normalised fields can join: as they were
              "imgenv_rollout_out": _cabi.RolloutOut, "imgenv_minibatch_buffer": _cabi.MinibatchBuffer, "imgenv_final_obs_out": _cabi.FinalObsOut}
    consts = {"IMGENV_NORM_OBS": _cabi.NORM_OBS, "IMGENV_NORM_REWARD": _cabi.NORM_REWARD, "IMGENV_ROLLOUT_NORM_STATES": _cabi.ROLLOUT_NORM_STATES,
              "IMGENV_ROLLOUT_NORM_REWARDS": _cabi.ROLLOUT_NORM_REWARDS, "IMGENV_FINAL_NORM_STATES": _cabi.FINAL_NORM_STATES,
              "IMGENV_ROLLOUT_ALL": _cabi.ROLLOUT_ALL, "IMGENV_FINAL_ALL": _cabi.FINAL_ALL, "IMGENV_MB_MAX_BUFFERS": _cabi.MB_MAX_BUFFERS}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "imgenv.h"', "int main(void) {"]
    for c in consts:
        lines.append('printf("%s %%d\\n", %s);' % (c, c))
    for st, m in mirror.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        for f, _ in m._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, f, st, f))
    lines.append("return 0; }")
    probe = tmp_path / "probe.c"
    probe.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())
    for name, v in consts.items():
        assert int(got[name]) == v, name
    for st, m in mirror.items():
        assert int(got[st]) == C.sizeof(m), st
        for f, _ in m._fields_:
            assert int(got["%s.%s" % (st, f)]) == getattr(m, f).offset, (st, f)
    # the sizes of the parent commit's header: 9 obs_ + 9 final_ + 9 scalars behind six ints; 9 + 7 pointers; 16 pointers behind two ints
    assert (C.sizeof(_cabi.RolloutOut), C.sizeof(_cabi.MinibatchBuffer), C.sizeof(_cabi.FinalObsOut)) == (24 + 8 * 27, 8 * 16, 8 + 8 * 16)
    assert C.sizeof(_cabi.NormaliseCfg) == 40 and C.sizeof(_cabi.NormaliseStats) == 72
    # the new bits lie outside the old masks
    assert not (_cabi.ROLLOUT_ALL & (_cabi.ROLLOUT_NORM_STATES | _cabi.ROLLOUT_NORM_REWARDS)) and not (_cabi.FINAL_ALL & _cabi.FINAL_NORM_STATES)


def test_make_normalise_cfg_and_stats():
    from img_env_amd import _cabi
    c = _cabi.make_normalise_cfg()
    assert (c.struct_size, c.flags, c.gamma, c.clip_obs, c.clip_reward, c.eps) == (40, 3, 0.99, 10.0, 10.0, 1e-8)
    assert _cabi.make_normalise_cfg(obs=False).flags == 2 and _cabi.make_normalise_cfg(reward=False).flags == 1
    s, arrays = _cabi.make_normalise_stats(5, 3)
    assert (s.struct_size, s.state_dim, s.n_rows, s.obs_count, s.ret_var) == (72, 5, 3, 1e-4, 1.0) and s.obs_var == arrays["obs_var"].ctypes.data
    assert _cabi.make_rollout_cfg(1, 1, ["vector_states", "norm_states", "norm_rewards"]).fields == 2 | 128 | 256
    assert _cabi.make_final_obs_cfg(["norm_states"]).fields == 8192


def test_refusals_that_need_no_device(hip_lib):
    """imgenv_normalise_enable judges its cfg before it touches the handle; the bits that need it are IMGENV_EINVAL without it"""
    from img_env_amd import _cabi
    o = _cabi.NormaliseOut()

    def refused(cfg, word):
        assert hip_lib.imgenv_normalise_enable(None, C.byref(cfg), C.byref(o)) == _cabi.EINVAL
        assert word in hip_lib.imgenv_last_error(), (word, hip_lib.imgenv_last_error())
    refused(_cabi.make_normalise_cfg(), b"null")  # a good cfg: only the handle is missing
    bad = _cabi.make_normalise_cfg()
    bad.struct_size = 32
    refused(bad, b"struct_size")
    refused(_cabi.make_normalise_cfg(obs=False, reward=False), b"flags")
    for kw, word in ((dict(clip_obs=0.0), b"clip_obs"), (dict(clip_obs=float("inf")), b"clip_obs"), (dict(clip_reward=-1.0), b"clip_reward"),
                     (dict(eps=0.0), b"eps"), (dict(eps=float("nan")), b"eps"), (dict(gamma=-0.1), b"gamma"), (dict(gamma=1.5), b"gamma"),
                     (dict(gamma=float("nan")), b"gamma")):
        refused(_cabi.make_normalise_cfg(**kw), word)
    wrong_out = _cabi.NormaliseOut()
    wrong_out.struct_size = 4
    assert hip_lib.imgenv_normalise_enable(None, C.byref(_cabi.make_normalise_cfg()), C.byref(wrong_out)) == _cabi.EINVAL
    assert hip_lib.imgenv_normalise_outputs(None, C.byref(o)) == _cabi.EINVAL
    assert hip_lib.imgenv_normalise_training(None, 1, None) == _cabi.EINVAL
    s, _ = _cabi.make_normalise_stats(5, 3)
    assert hip_lib.imgenv_normalise_stats_get(None, C.byref(s)) == _cabi.EINVAL and hip_lib.imgenv_normalise_stats_set(None, C.byref(s)) == _cabi.EINVAL
    # the storage bits before imgenv_normalise_enable (here: without a handle at all)
    assert hip_lib.imgenv_rollout_enable(None, C.byref(_cabi.make_rollout_cfg(8, 8, 2 | _cabi.ROLLOUT_NORM_STATES)), None) == _cabi.EINVAL
    assert b"imgenv_normalise_enable" in hip_lib.imgenv_last_error()
    assert hip_lib.imgenv_final_obs_enable(None, C.byref(_cabi.make_final_obs_cfg(_cabi.FINAL_NORM_STATES)), None) == _cabi.EINVAL
    assert b"imgenv_normalise_enable" in hip_lib.imgenv_last_error()
    assert hip_lib.imgenv_rollout_minibatch_enable(None, C.byref(_cabi.make_minibatch_cfg(8, 1, _cabi.ROLLOUT_NORM_REWARDS)), None) == _cabi.EINVAL
