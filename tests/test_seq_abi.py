"""The sequence minibatches (imgenv_rollout_seq_enable / _outputs / _index / _shuffle / _minibatch) without a GPU: the exports, the
struct layouts and constants as gcc sees include/imgenv.h against the ctypes mirror, what stays exactly as it was (ABI version 2,
IMGENV_K_COUNT 14, imgenv_rollout_out, imgenv_minibatch_out, imgenv_normalise_out), and the refusals that need no device.
(Everything that needs a live handle is in tests/test_gpu_sequences.py.)"""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("imgenv_rollout_seq_enable", "imgenv_rollout_seq_outputs", "imgenv_rollout_seq_index", "imgenv_rollout_seq_shuffle",
                "imgenv_rollout_seq_minibatch")


@pytest.fixture(scope="module")
def hip_lib():
    from img_env_amd import _cabi
    path = _cabi.library_path()
    if not os.path.exists(path):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return _cabi.bind(C.CDLL(path))


def test_library_exports_the_sequence_entry_points(hip_lib):
    from img_env_amd import _cabi
    header = open(os.path.join(ROOT, "include", "imgenv.h")).read()
    for f in ENTRY_POINTS:
        assert hasattr(hip_lib, f), f
        assert f in _cabi.SYMBOLS, f
        assert "int %s(" % f in header, f
    assert "#define IMGENV_ABI_VERSION 2 " in header  # new entry points only: no existing struct changed
    assert hip_lib.imgenv_abi_version() == 2
    assert "int imgenv_rollout_seq_shuffle(imgenv_t* h, uint32_t seed_lo, uint32_t seed_hi, void* stream);" in header
    assert hip_lib.imgenv_rollout_seq_shuffle.argtypes[1:3] == [C.c_uint32, C.c_uint32]
    assert "does NOT say whether slot 0 continues" in " ".join(header.split()).replace("* ", "")  # mb_first's limit is written down
    source = open(os.path.join(ROOT, "img_env_amd", "csrc", "sequences.h")).read()
    assert "does NOT say whether slot 0 continues" in " ".join(source.split()).replace("// ", "")


def test_seq_structs_and_constants_match_the_c_layout(tmp_path):
    from img_env_amd import _cabi
    buffer_fields = ["mb_" + n for n in _cabi.ROLLOUT_FIELDS + _cabi.ROLLOUT_NORM_FIELDS] + list(_cabi.SEQ_SCALARS)
    fields = {"imgenv_seq_cfg": ["struct_size", "length", "batch", "buffers", "fields", "state_bytes", "reserved"],
              "imgenv_seq_buffer": buffer_fields,
              "imgenv_seq_out": list(_cabi.SEQ_HEADER) + list(_cabi.SEQ_ARRAYS) + ["buf"],
              "imgenv_seq_args": ["struct_size", "j", "buffer", "n_scalars", "normalise", "reserved", "scalars", "norm", "states"]}
    unchanged = {"imgenv_rollout_out": _cabi.RolloutOut, "imgenv_minibatch_out": _cabi.MinibatchOut, "imgenv_minibatch_buffer": _cabi.MinibatchBuffer,
                 "imgenv_normalise_out": _cabi.NormaliseOut, "imgenv_minibatch_args": _cabi.MinibatchArgs, "imgenv_rollout_cfg": _cabi.RolloutCfg}
    consts = ["IMGENV_SEQ_MAX_STATES", "IMGENV_MB_MAX_SCALARS", "IMGENV_MB_MAX_BUFFERS", "IMGENV_K_COUNT", "IMGENV_ABI_VERSION"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "imgenv.h"', "int main(void) {"]
    for c in consts:
        lines.append('printf("%s %%d\\n", (int)%s);' % (c, c))
    for st in unchanged:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (st, st))
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
    mirror = {"imgenv_seq_cfg": _cabi.SeqCfg, "imgenv_seq_buffer": _cabi.SeqBuffer, "imgenv_seq_out": _cabi.SeqOut, "imgenv_seq_args": _cabi.SeqArgs}
    for st, fs in fields.items():
        assert int(got[st]) == C.sizeof(mirror[st]), st
        assert [name for name, _ in mirror[st]._fields_] == fs, st
        for f in fs:
            assert int(got["%s.%s" % (st, f)]) == getattr(mirror[st], f).offset, (st, f)
    assert int(got["IMGENV_SEQ_MAX_STATES"]) == _cabi.SEQ_MAX_STATES == 2
    assert C.sizeof(_cabi.SeqCfg) == 32
    assert C.sizeof(_cabi.SeqBuffer) == 8 * (len(_cabi.ROLLOUT_FIELDS) + 2 + len(_cabi.SEQ_SCALARS) + 1)
    assert C.sizeof(_cabi.SeqOut) == 40 + 8 * len(_cabi.SEQ_ARRAYS) + 4 * C.sizeof(_cabi.SeqBuffer)
    assert C.sizeof(_cabi.SeqArgs) == 24 + 8 * 6 + 8 + 8 * 2
    # what stays exactly as it was
    assert int(got["IMGENV_ABI_VERSION"]) == 2 and int(got["IMGENV_K_COUNT"]) == _cabi.K_COUNT == 14
    assert int(got["IMGENV_MB_MAX_SCALARS"]) == 6 and int(got["IMGENV_MB_MAX_BUFFERS"]) == 4
    for st, m in unchanged.items():
        assert int(got[st]) == C.sizeof(m), st
    assert C.sizeof(_cabi.RolloutOut) == 24 + 8 * (2 * len(_cabi.ROLLOUT_FIELDS) + len(_cabi.ROLLOUT_SCALARS))
    assert C.sizeof(_cabi.MinibatchOut) == 24 + 8 * len(_cabi.MB_ARRAYS) + 4 * 8 * (len(_cabi.ROLLOUT_FIELDS) + len(_cabi.MB_SCALARS))
    assert C.sizeof(_cabi.NormaliseOut) == 16 + 8 * 5 + 16 + 8 * 4 + 8 * 8 + 8 * 2


def test_make_seq_cfg_and_args():
    from img_env_amd import _cabi
    c = _cabi.make_seq_cfg(16, 256, 2, ["vector_states", "ped_maps"], (512, 512))
    assert (c.struct_size, c.length, c.batch, c.buffers, c.fields, list(c.state_bytes), c.reserved) == (32, 16, 256, 2, 2 | 16, [512, 512], 0)
    assert _cabi.make_seq_cfg(4, 8).fields == 0 and list(_cabi.make_seq_cfg(4, 8, 1, None, (32,)).state_bytes) == [32, 0]
    with pytest.raises(ValueError):
        _cabi.make_seq_cfg(4, 8, 1, ["no_such_field"])
    with pytest.raises(ValueError):
        _cabi.make_seq_cfg(4, 8, 1, None, (4, 4, 4))
    a = _cabi.make_seq_args(3, 1, [256, 512], 1, 768, [1024, None])
    assert (a.struct_size, a.j, a.buffer, a.n_scalars, a.normalise, a.reserved) == (C.sizeof(_cabi.SeqArgs), 3, 1, 2, 1, 0)
    assert list(a.scalars) == [256, 512, None, None, None, None] and a.norm == 768 and list(a.states) == [1024, None]


def test_refusals_that_need_no_device(hip_lib):
    """imgenv_rollout_seq_enable judges its cfg before it touches the handle: a wrong struct_size, length < 1, batch < 1, buffers 0 and
    5, unknown bits and a bad state size are IMGENV_EINVAL with a message that names the field; so is a null handle or cfg, in every
    entry point; imgenv_rollout_seq_minibatch judges its args likewise"""
    from img_env_amd import _cabi
    o = _cabi.SeqOut()

    def refused(cfg, word):
        assert hip_lib.imgenv_rollout_seq_enable(None, C.byref(cfg), C.byref(o)) == _cabi.EINVAL
        assert word in hip_lib.imgenv_last_error(), (word, hip_lib.imgenv_last_error())
    refused(_cabi.make_seq_cfg(4, 8, 1, 3, (32,)), b"null")  # a good cfg: only the handle is missing
    bad = _cabi.make_seq_cfg(4, 8)
    bad.struct_size = 12
    refused(bad, b"struct_size")
    for length in (0, -1):
        refused(_cabi.make_seq_cfg(length, 8), b"length")
    for batch in (0, -1):
        refused(_cabi.make_seq_cfg(4, batch), b"batch")
    for buffers in (0, 5, -1):
        refused(_cabi.make_seq_cfg(4, 8, buffers), b"buffers")
    for bits in (_cabi.ROLLOUT_ALL + 1, -1, 1 << 20):
        refused(_cabi.make_seq_cfg(4, 8, 1, bits), b"fields")
    for nb in (-4, 6, 65540):
        refused(_cabi.make_seq_cfg(4, 8, 1, 0, (nb,)), b"state_bytes[0]")
    wrong_out = _cabi.SeqOut()
    wrong_out.struct_size = 4
    assert hip_lib.imgenv_rollout_seq_enable(None, C.byref(_cabi.make_seq_cfg(4, 8)), C.byref(wrong_out)) == _cabi.EINVAL
    assert hip_lib.imgenv_rollout_seq_enable(None, None, None) == _cabi.EINVAL
    assert hip_lib.imgenv_rollout_seq_outputs(None, C.byref(o)) == _cabi.EINVAL
    assert hip_lib.imgenv_rollout_seq_index(None, None) == _cabi.EINVAL
    assert hip_lib.imgenv_rollout_seq_shuffle(None, 1, 2, None) == _cabi.EINVAL
    assert hip_lib.imgenv_rollout_seq_minibatch(None, None, None) == _cabi.EINVAL

    def args_refused(a, word):
        assert hip_lib.imgenv_rollout_seq_minibatch(None, C.byref(a), None) == _cabi.EINVAL
        assert word in hip_lib.imgenv_last_error(), (word, hip_lib.imgenv_last_error())
    args_refused(_cabi.make_seq_args(0, 0, [256], 0, 512), b"null")  # good args: only the handle is missing
    a = _cabi.make_seq_args(0)
    a.struct_size = 8
    args_refused(a, b"struct_size")
    args_refused(_cabi.make_seq_args(-1), b".j")
    a = _cabi.make_seq_args(0)
    a.n_scalars = 7
    args_refused(a, b"n_scalars")
    args_refused(_cabi.make_seq_args(0, 0, [256], 1, 512), b"normalise")
    args_refused(_cabi.make_seq_args(0, 0, [256], -2), b"normalise")
    args_refused(_cabi.make_seq_args(0, 0, [256, 0]), b"scalars[1]")
    args_refused(_cabi.make_seq_args(0, 0, [256], 0, None), b"norm is null")
