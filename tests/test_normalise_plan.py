"""k_norm_part and k_norm_apply (img_env_amd/csrc/normalise.h) on the CPU, beside tests/test_rollout_plan.py:
tests/host/normalise_check.cpp compiles the header's per-lane functions for the host and runs them over a simulated grid on seeded
cases written here; what it leaves after every chain -- the statistics, the returns and the three normalised arrays -- is compared
bit for bit with tests/normalise_model.py.  The cases: state_dim 1, 5 and 7; 1 row, 15 rows and one tile + 1 (so the tiles' merge
and the striding over a one-block grid run); listed reset chains with the host's count and with a device-side count of 0, 1 and
all worlds; a step with every row frozen; evaluation chains; a state stack; observation-only and reward-only handles.  The same
program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own."""
import os
import subprocess

import numpy as np
import pytest

import normalise_model as nm
from img_env_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "normalise_check.cpp")
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
PAR = dict(gamma=0.97, clip_obs=2.5, clip_reward=1.5, eps=1e-6)  # (clips that bite)


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + flags + [SOURCE, "-o", exe])
    return exe


def _run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    return out.stdout.split()


def make_case(seed, W, Rw, D, K, obs, reward, script):
    """``script``: ("step", training, frozen, grid_part, grid_apply) | ("reset", training, mode, worlds, grid_part, grid_apply)
    entries; frozen: "some" | "all" | "none".  Returns (the case file's bytes, what the model leaves after every chain)"""
    rng = np.random.default_rng(seed)
    R = W * Rw
    i32 = lambda *v: np.array(v, "<i4").tobytes()  # noqa: E731
    blob = [i32(R, Rw, D, K, (1 if obs else 0) | (2 if reward else 0), len(script)),
            np.array([PAR["gamma"], PAR["clip_obs"], PAR["clip_reward"], PAR["eps"]], "<f8").tobytes()]
    m = nm.Normalise(R, D, K, obs, reward, **PAR)
    offs, scl = rng.uniform(-2, 2, D), rng.uniform(0.2, 3, D)
    want = []
    for entry in script:
        vs = (offs + scl * rng.standard_normal((R, D))).astype(np.float32)
        stack = (offs + scl * rng.standard_normal((R, K, D))).astype(np.float32)
        if K:
            stack[:, -1] = vs
            stack[rng.random(R) < 0.3, 0] = 0.0  # (zero padding of a young stack: normalised like any value)
        m.training = bool(entry[1])
        if entry[0] == "step":
            _, training, frozen, gp, ga = entry
            rewards = rng.standard_normal(R) * 3.0
            clean = {"some": rng.random(R) < 0.7, "all": np.zeros(R, bool), "none": np.ones(R, bool)}[frozen].astype(np.uint8)
            dones = (rng.random(R) < 0.2).astype(np.uint8)
            blob += [i32(0, training, gp, ga), vs.tobytes(), stack.tobytes(), rewards.astype("<f8").tobytes(), clean.tobytes(), dones.tobytes()]
            m.step(vs, rewards, clean, dones, stack)
        else:
            _, training, mode, worlds, gp, ga = entry
            rows = list(range(R)) if mode == 0 else [w * Rw + i for w in worlds for i in range(Rw)]
            blob += [i32(1, training, gp, ga), vs.tobytes(), stack.tobytes(), i32(mode, len(worlds), *worlds)]
            m.reset(rows, vs, stack)
        s = m.stats()
        want.append(b"".join([np.array([s["obs_count"], s["ret_count"], s["ret_mean"], s["ret_var"]], "<f8").tobytes(), s["obs_mean"].tobytes(),
                              s["obs_var"].tobytes(), s["returns"].tobytes(), m.norm_vector_states.tobytes(), m.norm_state_stack.tobytes(),
                              m.norm_rewards.tobytes()]))
    return b"".join(blob), want


def _script(W):
    every = list(range(W))
    return [("step", 1, "some", 0, 0), ("reset", 1, 2, every[:1], 0, 0), ("step", 1, "some", 1, 1), ("reset", 1, 2, [], 0, 0),
            ("step", 1, "all", 0, 0), ("reset", 1, 2, every[::-1], 0, 2), ("step", 1, "none", 2, 3), ("reset", 1, 1, every[::2], 1, 0),
            ("step", 0, "some", 0, 0), ("reset", 0, 1, every[-1:], 0, 0), ("reset", 1, 0, [], 0, 0), ("step", 1, "some", 0, 0)]


TILE_7 = nm.tile_rows(7 + 1)  # rows of a tile of a step's 7 + 1 columns
# (seed, worlds, robots per world, D, K, obs, reward)
CASES = [
    (0, 1, 1, 1, 0, True, True),
    (1, 1, 1, 5, 3, True, True),
    (2, 5, 3, 5, 3, True, True),
    (3, 15, 1, 7, 0, True, True),
    (4, TILE_7 + 1, 1, 7, 2, True, True),          # one tile + 1: two tiles merge; a grid of one block strides
    (5, nm.tile_rows(1) // 4 + 1, 4, 1, 0, True, True),  # state_dim 1: two columns, 32 rows per wavefront, one tile + 4 rows
    (6, 5, 3, 5, 2, True, False),
    (7, 5, 3, 5, 0, False, True),
    (8, nm.tile_rows(1) + 1, 1, 5, 0, False, True),      # one column: 64 rows per wavefront
]


def check_cases(exe, tmp_path):
    for seed, W, Rw, D, K, obs, reward in CASES:
        blob, want = make_case(seed, W, Rw, D, K, obs, reward, _script(W))
        case, result = tmp_path / ("case%d.bin" % seed), tmp_path / ("result%d.bin" % seed)
        case.write_bytes(blob)
        assert int(_run(exe, "run", case, result)[2]) == len(want)
        got = result.read_bytes()
        assert len(got) == sum(len(w) for w in want), seed
        at = 0
        for q, w in enumerate(want):
            assert got[at:at + len(w)] == w, (seed, q, _script(W)[q])
            at += len(w)


def test_normalise_plan_and_launch_shapes(tmp_path):
    words = _run(_build(tmp_path, "normalise_check", []), "plan")
    consts = dict(zip(words[1::2], (int(w) for w in words[2::2])))
    assert consts == {"NORM_BLOCK": _cabi.NORM_BLOCK, "NORM_PER_LANE": _cabi.NORM_PER_LANE, "NORM_MAX_COLS": _cabi.NORM_MAX_COLS,
                      "NORM_MAX_BLOCKS": _cabi.NORM_MAX_BLOCKS}
    assert (nm.NORM_BLOCK, nm.NORM_PER_LANE) == (_cabi.NORM_BLOCK, _cabi.NORM_PER_LANE)


def test_normalise_walk_against_the_model(tmp_path):
    check_cases(_build(tmp_path, "normalise_check", []), tmp_path)


def test_normalise_walk_under_sanitizers(tmp_path):
    exe = _build(tmp_path, "normalise_check_san", SAN)
    _run(exe, "plan")
    check_cases(exe, tmp_path)
