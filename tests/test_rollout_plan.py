"""k_rollout and k_rollout_gae (img_env_amd/csrc/rollout.h) on the CPU, beside tests/test_final_obs_plan.py:
tests/host/rollout_check.cpp compiles the header's item function, its count and the advantage pass's row function for the host and
runs them over a simulated grid on seeded cases written here; what it leaves is compared bit for bit with tests/rollout_model.py.
The cases reach every chunk unit (rows of 48, 1448, 20, 6 and 3 bytes: 16 / 8 / 4 / 2 / 1), listed reset chains with the host's and
with a device-side count, an unlisted one, both parities of final_n, a final list that overflows, grids of one block, of the
planner's size and of two blocks that stride, and more rows than the advantage pass's grid has lanes.  The same program runs once
more under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own."""
import os
import subprocess

import numpy as np
import pytest

import rollout_model
from img_env_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "rollout_check.cpp")
ROW_BYTES = {"a16": 48, "b8": 1448, "c4": 20, "d2": 6, "e1": 3}
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + flags + [SOURCE, "-o", exe])
    return exe


def _run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    return out.stdout.split()


def make_case(seed, n_worlds, Rw, T, F, script, row_bytes=ROW_BYTES):
    """``script``: ("step", blocks) | ("reset", mode, worlds, blocks) entries.  Returns (the case file's bytes, the model's input)"""
    rng = np.random.default_rng(seed)
    R = n_worlds * Rw

    def obs():
        return {name: rng.integers(0, 256, (R, nb), dtype=np.uint8) for name, nb in row_bytes.items()}
    i32 = lambda *v: np.array(v, "<i4").tobytes()  # noqa: E731
    first = obs()
    blob = [i32(R, Rw, T, F, len(row_bytes), len(script)), i32(*row_bytes.values())] + [a.tobytes() for a in first.values()]
    chains = []
    for entry in script:
        o = obs()
        if entry[0] == "step":
            info = rng.choice(np.array([0, 0, 0, 1, 2, 3, 5, 10], np.int32), R)
            c = {"kind": "step", "obs": o, "actions": rng.standard_normal((R, 3)).astype(np.float32), "rewards": rng.standard_normal(R) * 3.0,
                 "dones": (info != 0).astype(np.uint8), "is_clean": (rng.random(R) < 0.8).astype(np.uint8), "dones_info": info}
            blob += [i32(0), c["actions"].tobytes(), c["rewards"].astype("<f8").tobytes(), c["dones"].tobytes(), c["is_clean"].tobytes(),
                     info.astype("<i4").tobytes(), i32(entry[1])]
        else:
            _, mode, worlds, blocks = entry
            rows = list(range(R)) if mode == 0 else [w * Rw + i for w in worlds for i in range(Rw)]
            c = {"kind": "reset", "rows": rows, "obs": o}
            blob += [i32(1, mode, len(worlds), *worlds), i32(blocks)]
        blob += [a.tobytes() for a in o.values()]
        chains.append(c)
    gae = {"gamma": np.float32(0.97), "lam": np.float32(0.9), "values": rng.standard_normal((T + 1, R)).astype(np.float32),
           "final_values": rng.standard_normal(F).astype(np.float32), "adv": rng.standard_normal((T, R)).astype(np.float32),
           "ret": rng.standard_normal((T, R)).astype(np.float32), "has_fv": bool(seed % 2 == 0)}
    blob += [np.array([gae["gamma"], gae["lam"]], "<f4").tobytes(), i32(int(gae["has_fv"]))] + [gae[k].tobytes() for k in ("values", "final_values", "adv", "ret")]
    return b"".join(blob), first, chains, gae


def read_result(path, R, T, F, row_bytes=ROW_BYTES):
    raw = np.fromfile(path, np.uint8)
    at = [0]

    def take(dtype, shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = raw[at[0]:at[0] + n].view(dtype).reshape(shape)
        at[0] += n
        return a
    r = {}
    for name, nb in row_bytes.items():
        r["obs_" + name] = take(np.uint8, (T + 1, R, nb))
        r["final_" + name] = take(np.uint8, (F, nb))
    for name, dt, shape in (("actions", "<f4", (T, R, 3)), ("rewards", "<f4", (T, R)), ("dones", np.uint8, (T, R)), ("is_clean", np.uint8, (T, R)),
                            ("dones_info", "<i4", (T, R)), ("final_idx", "<i4", (T + 1, R)), ("final_slot", "<i4", (F,)), ("final_row", "<i4", (F,)),
                            ("final_n", "<i4", (2,)), ("adv", "<f4", (T, R)), ("ret", "<f4", (T, R))):
        r[name] = take(dt, shape)
    assert at[0] == raw.size
    return r


# (seed, worlds, robots per world, T, F, script)
CASES = [
    # both parities of final_n, the three kinds of reset chain, a stride of two blocks, a reset right after begin and one on the last slot
    (0, 3, 2, 5, 16, [("reset", 1, [1], 0), ("step", 0), ("reset", 1, [0, 2], 0), ("step", 2), ("step", 1), ("reset", 2, [2, 0, 1], 2),
                      ("step", 0), ("reset", 0, [], 1), ("step", 0), ("reset", 2, [1], 0)]),
    # a final list of three entries and twelve restarted rows: the kept entries and the ring stay intact, the count goes on
    (1, 3, 2, 4, 3, [("step", 0), ("reset", 1, [2, 1], 0), ("step", 0), ("reset", 0, [], 0), ("step", 0), ("reset", 2, [0], 0), ("step", 0)]),
    # fewer transitions than the horizon (the rows t >= n of adv / ret stay), and a device-side count of zero
    (2, 2, 3, 6, 8, [("step", 0), ("reset", 2, [], 0), ("step", 0), ("reset", 1, [1], 0)]),
    # more rows than the advantage pass's simulated grid has lanes (2 x GAE_BLOCK), small rows
    (3, 50, 3, 9, 200, [("step", 0), ("step", 3), ("reset", 1, list(range(0, 50, 3)), 0), ("step", 0), ("step", 0), ("reset", 2, [4, 9, 49], 1),
                        ("step", 0), ("step", 0), ("step", 0), ("step", 0), ("step", 0)]),
]


def check_cases(exe, tmp_path):
    for seed, W, Rw, T, F, script in CASES:
        row_bytes = ROW_BYTES if W < 10 else {"c4": 20, "e1": 3}
        blob, first, chains, g = make_case(seed, W, Rw, T, F, script, row_bytes)
        case, result = tmp_path / ("case%d.bin" % seed), tmp_path / ("result%d.bin" % seed)
        case.write_bytes(blob)
        words = _run(exe, "run", case, result)
        want = rollout_model.replay(T, F, first, chains)
        assert int(words[2]) == want["n"] and int(words[4]) == want["resets"]
        got = read_result(result, W * Rw, T, F, row_bytes)
        for name in got:
            if name in ("adv", "ret", "final_n"):
                continue
            assert got[name].tobytes() == want[name].tobytes(), (seed, name)
        assert int(got["final_n"][want["resets"] & 1]) == want["final_count"], seed
        adv, ret = rollout_model.gae(want, g["values"], g["final_values"] if g["has_fv"] else None, g["gamma"], g["lam"], F, g["adv"], g["ret"])
        assert got["adv"].tobytes() == adv.tobytes() and got["ret"].tobytes() == ret.tobytes(), seed
        assert adv[want["n"]:].tobytes() == g["adv"][want["n"]:].tobytes()  # (the model too leaves t >= n alone)
    # what the cases are there to reach
    w1 = rollout_model.replay(CASES[1][3], CASES[1][4], *make_case(*CASES[1])[1:3])
    assert w1["final_count"] == 12 > CASES[1][4] and (w1["final_idx"] >= CASES[1][4]).any()


def test_rollout_plan_and_launch_shapes(tmp_path):
    words = _run(_build(tmp_path, "rollout_check", []), "plan")
    consts = dict(zip(words[3::2], (int(w) for w in words[4::2])))
    assert consts["ROLLOUT_BLOCK"] == _cabi.ROLLOUT_BLOCK and consts["ROLLOUT_MAX_BLOCKS"] == _cabi.ROLLOUT_MAX_BLOCKS
    assert consts["GAE_BLOCK"] == _cabi.GAE_BLOCK and consts["GAE_MAX_BLOCKS"] == _cabi.GAE_MAX_BLOCKS
    assert consts["ROLLOUT_MAX_FIELDS"] == len(_cabi.ROLLOUT_FIELDS)  # every obs_* pointer of the out struct is a field
    assert consts["GAE_BATCH"] >= 1


def test_rollout_walk_against_the_model(tmp_path):
    check_cases(_build(tmp_path, "rollout_check", []), tmp_path)


def test_rollout_walk_under_sanitizers(tmp_path):
    exe = _build(tmp_path, "rollout_check_san", SAN)
    _run(exe, "plan")
    check_cases(exe, tmp_path)


def test_model_refuses_a_step_on_a_full_ring():
    blob, first, chains, g = make_case(5, 1, 2, 1, 2, [("step", 0), ("step", 0)], {"c4": 20})
    with pytest.raises(AssertionError, match="rollout full"):
        rollout_model.replay(1, 2, first, chains)
