"""The observation stacks (imgenv_stack_bytes / imgenv_stack_enable) without a GPU: the exports, the struct layouts, the byte
counts -- and the numpy model the GPU tests compare against (tests/stack_model.py), held to what the reference's own
StateBatchWrapper returned (tests/golden/python_stack_*.npz)."""
import ast
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from stack_model import StackModel, depths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def hip_lib():
    from img_env_amd import _cabi
    path = _cabi.library_path()
    if not os.path.exists(path):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return _cabi.bind(C.CDLL(path))


def test_library_exports_the_stack_entry_points(hip_lib):
    from img_env_amd import _cabi
    for f in ("imgenv_stack_bytes", "imgenv_stack_enable", "imgenv_stack_outputs"):
        assert hasattr(hip_lib, f), f
        assert f in _cabi.SYMBOLS, f


def test_stack_structs_match_the_c_layout(tmp_path):
    """sizeof / offsetof as gcc sees include/imgenv.h vs the ctypes mirror"""
    from img_env_amd import _cabi
    fields = {"imgenv_stack_cfg": ["struct_size", "image_batch", "state_batch", "laser_batch", "arena", "arena_bytes"],
              "imgenv_stack_out": ["struct_size", "n_local", "image_depth", "state_depth", "laser_depth", "sensor_maps", "vector_states",
                                   "lasers"]}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "imgenv.h"', "int main(void) {",
             'printf("cap %d\\n", IMGENV_STACK_MAX_DEPTH);']
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
    mirror = {"imgenv_stack_cfg": _cabi.StackCfg, "imgenv_stack_out": _cabi.StackOut}
    for st, fs in fields.items():
        assert int(got[st]) == C.sizeof(mirror[st]), st
        for f in fs:
            assert int(got["%s.%s" % (st, f)]) == getattr(mirror[st], f).offset, (st, f)
    assert int(got["cap"]) == _cabi.STACK_MAX_DEPTH >= 16


def _align256(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("batches", [(1, 3, 0), (2, 3, 2), (4, 1, -1), (0, 0, -1)])
@pytest.mark.parametrize("state_dim,beams,image", [(3, 360, (48, 48)), (5, 181, (48, 48)), (3, 360, (20, 12))])
@pytest.mark.parametrize("shard", [None, (5, 12)])
def test_stack_bytes_is_the_rounded_sum_over_the_deep_fields(hip_lib, batches, state_dim, beams, image, shard):
    from img_env_amd import _cabi, worldgen
    n = 16
    params = worldgen.make_params(n, 0, state_dim=state_dim, range_total=beams, image_size=list(image))
    if shard:
        params = dict(params, robot_begin=shard[0], robot_end=shard[1])
    cfg, keep = _cabi.make_cfg(params)
    R = shard[1] - shard[0] if shard else n
    frame = (image[0] * image[1] * 2, state_dim * 4, beams * 8)
    want = 0
    for k, f in zip(depths(*batches), frame):
        if k >= 2:  # depth 1 aliases the output array, 0 is off: neither takes space
            want += _align256(R * k * f)
    s = _cabi.make_stack_cfg(*batches)
    assert hip_lib.imgenv_stack_bytes(C.byref(cfg), C.byref(s)) == want
    if max(depths(*batches)) <= 1:
        assert want == 0


def test_stack_bytes_without_lasers_and_above_the_cap(hip_lib):
    from img_env_amd import _cabi, worldgen
    params = worldgen.make_params(4, 0, use_laser=False)
    cfg, keep = _cabi.make_cfg(params)
    s = _cabi.make_stack_cfg(0, 0, 4)  # no lasers on the handle: nothing to stack
    assert hip_lib.imgenv_stack_bytes(C.byref(cfg), C.byref(s)) == 0
    cfg, keep = _cabi.make_cfg(worldgen.make_params(4, 0))
    cap = _cabi.STACK_MAX_DEPTH
    for ok in ((cap, 0, -1), (0, cap, -1), (0, 0, cap)):
        assert hip_lib.imgenv_stack_bytes(C.byref(cfg), C.byref(_cabi.make_stack_cfg(*ok))) > 0, ok
    for bad in ((cap + 1, 0, -1), (0, cap + 1, -1), (0, 0, cap + 1)):
        assert hip_lib.imgenv_stack_bytes(C.byref(cfg), C.byref(_cabi.make_stack_cfg(*bad))) < 0, bad
    s = _cabi.make_stack_cfg(2, 2, 2)
    s.struct_size = 4
    assert hip_lib.imgenv_stack_bytes(C.byref(cfg), C.byref(s)) < 0


@pytest.mark.parametrize("name,n_steps,n_resets,want_depths", [("a", 21, 3, (2, 3, 2)), ("b", 15, 3, (1, 1, 1)), ("c", 45, 6, (1, 3, 1))])
def test_the_model_reproduces_the_references_recordings(name, n_steps, n_resets, want_depths):
    """the yardstick of the GPU tests on the reference itself: the rule of tests/stack_model.py replayed over what the
    reference's unmodified wrapper stack returned (frame = the newest slot, reset = the step after exp_all_down is all true)"""
    z = np.load(os.path.join(GOLDEN, "python_stack_%s.npz" % name))
    meta = ast.literal_eval(str(z["meta"]))
    over = meta["cfg_over"]
    kd = depths(over["image_batch"], over["state_batch"], over["laser_batch"])
    assert kd == want_depths
    n = meta["n_robots"]
    assert len(z["exp_obs0"]) == n_steps == meta["steps"] + 1 and int(z["n_resets"]) == n_resets
    resets, mismatches = 0, 0
    for k, field in enumerate(meta["obs_names"][:2]):
        exp = z["exp_obs%d" % k]
        depth = kd[{"sensor_maps": 0, "vector_states": 1, "lasers": 2}[field]]
        if field == "vector_states":
            exp = exp.reshape(exp.shape[0], n, depth, -1)
        assert exp.shape[2] == depth
        model, n_reset = StackModel(depth), 0
        for t in range(n_steps):
            reset = t == 0 or bool(z["exp_all_down"][t - 1].all())
            n_reset += reset
            got = model.update(exp[t][:, -1], np.full(n, reset))
            mismatches += not np.array_equal(got, exp[t])
        resets = n_reset
    assert resets == n_resets
    assert mismatches == 0
