"""The sequence kernels (img_env_amd/csrc/sequences.h) on the CPU, beside tests/test_minibatch_plan.py: tests/host/seq_check.cpp
compiles the header's flag and gather functions (and the minibatches' compaction and shuffle they run on) for the host and runs them
over a simulated grid on seeded cases written here; what it leaves is compared bit for bit with tests/seq_model.py.  Its ``plan``
mode holds seq_enable_plan's refusals, the launch shapes and the block's layout.  The cases reach: n a multiple of L and not; L = 1
and L = T; C R exactly one tile and one tile plus one; no valid sequence; Bs larger than Vs; j beyond the last minibatch; every
chunk unit (rows of 48, 1448, 20, 6 and 3 bytes); state rows of 4, 24 and 512 bytes; gather grids that stride.  The same program
runs once more under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own: is_clean is an allocation of exactly
n R bytes and seq_flag of exactly C R there, so a flag read or written past the end is found."""
import os
import subprocess

import numpy as np

import minibatch_model as mm
import seq_model as sm
from img_env_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "seq_check.cpp")
ROW_BYTES = {"a16": 48, "b8": 1448, "c4": 20, "d2": 6, "e1": 3}
SMALL = {"c4": 20, "e1": 3}
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
TILE = _cabi.MB_TILE


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + flags + [SOURCE, "-o", exe])
    return exe


def _run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    return out.stdout.split()


def make_case(seed, R, T, n, L, Bs, j, p_clean, row_bytes, n_scalars, normalise, blocks, state_bytes):
    rng = np.random.default_rng(seed)
    c = {"R": R, "T": T, "n": n, "L": L, "Bs": Bs, "j": j, "normalise": None if normalise < 0 else normalise,
         "seed": int(rng.integers(0, 2 ** 63)) * 2 + 1, "norm": np.array([0.25, 2.0], np.float32)}
    c["is_clean"] = (rng.random((T, R)) < p_clean).astype(np.uint8) * rng.integers(1, 256, (T, R)).astype(np.uint8)  # (any non-zero byte counts)
    c["final_idx"] = np.where(rng.random((T + 1, R)) < 0.2, rng.integers(0, 50, (T + 1, R)), -1).astype(np.int32)
    c["fields"] = {name: rng.integers(0, 256, (T + 1, R, nb), dtype=np.uint8) for name, nb in row_bytes.items()}
    c["ring"] = {"actions": rng.standard_normal((T, R, 3)).astype(np.float32), "rewards": rng.standard_normal((T, R)).astype(np.float32),
                 "dones": (rng.random((T, R)) < 0.2).astype(np.uint8), "dones_info": rng.integers(0, 11, (T, R)).astype(np.int32)}
    c["scalars"] = [rng.standard_normal((T + 1, R)).astype(np.float32) for _ in range(n_scalars)]
    c["states"] = [rng.integers(0, 256, (T + 1, R, nb), dtype=np.uint8) for nb in state_bytes if nb]
    sb = (list(state_bytes) + [0, 0])[:2]
    lo, hi = mm.split_seed(c["seed"])
    blob = [np.array([R, T, n, L, Bs, j, len(row_bytes), n_scalars, normalise, blocks] + sb, "<i4").tobytes(), np.array([lo, hi], "<u4").tobytes(),
            c["norm"].tobytes(), np.array(list(row_bytes.values()), "<i4").tobytes(), c["is_clean"].tobytes(), c["final_idx"].tobytes()]
    blob += [a.tobytes() for a in c["fields"].values()]
    blob += [c["ring"][k].tobytes() for k in ("actions", "rewards", "dones", "dones_info")] + [a.tobytes() for a in c["scalars"]]
    blob += [a.tobytes() for a in c["states"]]
    return b"".join(blob), c


def read_result(path, CR, S, L, Bs, row_bytes, state_bytes):
    raw = np.fromfile(path, np.uint8)
    at = [0]

    def take(dtype, shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = raw[at[0]:at[0] + n].view(dtype).reshape(shape)
        at[0] += n
        return a
    r = {"valid_n": int(take("<i4", (1,))[0]), "flag": take(np.uint8, (CR,)), "valid": take("<i4", (S,)), "order": take("<i4", (S,))}
    for name, nb in row_bytes.items():
        r["mb_" + name] = take(np.uint8, (L, Bs, nb))
    for name, dt, shape in (("mb_actions", "<f4", (L, Bs, 3)), ("mb_rewards", "<f4", (L, Bs)), ("mb_dones", np.uint8, (L, Bs)),
                            ("mb_dones_info", "<i4", (L, Bs)), ("mb_index", "<i4", (L, Bs)), ("mb_weight", "<f4", (L, Bs)),
                            ("mb_first", np.uint8, (L, Bs)), ("mb_scalars", "<f4", (_cabi.MB_MAX_SCALARS, L, Bs)), ("mb_seq", "<i4", (Bs,)),
                            ("mb_seq_len", "<i4", (Bs,))):
        r[name] = take(dt, shape)
    for a, nb in enumerate(nb for nb in state_bytes if nb):
        r["mb_seq_state%d" % a] = take(np.uint8, (Bs, nb))
    assert at[0] == raw.size
    return r


# (seed, R, T, n, L, Bs, j, share of clean flags, rows, scalars, normalise, gather blocks, state bytes)
CASES = [
    (0, 6, 15, 15, 4, 4, 0, 0.3, ROW_BYTES, 3, 1, 0, (4, 24)),     # n no multiple of L: the last chunk has 3 steps; every chunk unit; the planner's grid
    (1, 6, 15, 15, 4, 5, 3, 0.3, ROW_BYTES, 3, 1, 2, (512,)),      # its last minibatch: slots behind the valid list; two blocks stride
    (2, 6, 16, 12, 4, 4, 9, 0.5, SMALL, 1, -1, 1, ()),             # n a multiple of L, below the horizon; j beyond the last minibatch
    (3, 7, 5, 5, 2, 64, 0, 0.0, SMALL, 2, 0, 0, (24,)),            # no valid sequence: Bs > Vs = 0
    (4, 7, 5, 5, 1, 64, 0, 1.0, SMALL, 6, 5, 1, (4, 512)),         # L = 1, all valid, 35 < Bs; six scalars
    (5, 9, 6, 5, 6, 4, 1, 0.6, SMALL, 1, 0, 0, (24, 4)),           # L = T with the cursor below: one chunk per row
    (6, 1024, 8, 8, 2, 200, 3, 0.3, {"e1": 3}, 1, 0, 3, ()),       # C R exactly one tile (4096 sequences); three blocks stride
    (7, 4097, 2, 1, 2, 100, 40, 0.9, {"c4": 20}, 0, -1, 0, (4,)),  # C R one tile plus one, C < C_max
    (8, 5, 7, 7, 3, 8, 0, 0.4, {}, 2, 1, 0, (24,)),                # no copied field (all drawn): the scalars' lane alone
]


def check_cases(exe, tmp_path, cases):
    for case in cases:
        seed, R, T, n, L, Bs, j, p, row_bytes, n_scalars, normalise, blocks, state_bytes = case
        blob, c = make_case(*case)
        path, result = tmp_path / ("case%d.bin" % seed), tmp_path / ("result%d.bin" % seed)
        path.write_bytes(blob)
        words = _run(exe, "run", path, result)
        CR, S = sm.chunks(n, L) * R, sm.chunks(T, L) * R
        got = read_result(result, CR, S, L, Bs, row_bytes, state_bytes)
        assert got["flag"].tobytes() == sm.flags(c["is_clean"], n, L).tobytes(), seed
        valid = sm.valid_list(c["is_clean"], n, L)
        Vs = len(valid)
        assert int(words[2]) == Vs == got["valid_n"], seed
        assert int(words[4]) == -(-CR // TILE), seed
        assert got["valid"][:Vs].tobytes() == valid.tobytes(), seed
        order = sm.order_list(valid, S, c["seed"])
        assert got["order"].tobytes() == order.tobytes(), seed
        mb = sm.gather(order, j, Bs, L, n, R, c["fields"], c["ring"], c["is_clean"], c["final_idx"], c["scalars"], c["normalise"], c["norm"], c["states"])
        for name in mb:
            if name == "mb_scalars":
                assert got[name][:n_scalars].tobytes() == mb[name].tobytes(), seed
                assert not got[name][n_scalars:].any()
            else:
                assert got[name].tobytes() == mb[name].tobytes(), (seed, name)
        assert set(got) - {"valid_n", "flag", "valid", "order"} == set(mb), seed


def test_what_the_cases_reach():
    reach = {}
    for c in CASES:
        _, case = make_case(*c)
        reach[c[0]] = (sm.chunks(c[3], c[4]) * c[1], len(sm.valid_list(case["is_clean"], c[3], c[4])), case)
    assert 15 % 4 == 3 and 12 % 4 == 0
    flags0 = sm.flags(reach[0][2]["is_clean"], 15, 4)
    assert (flags0 == 0).any() and (flags0 == 1).any()  # wholly unclean sequences beside valid ones
    assert 3 * 5 < reach[1][1] < 4 * 5     # minibatch 3 is the last one, partly empty
    assert reach[2][1] < 9 * 4
    assert reach[3][1] == 0 and reach[4][:2] == (35, 35)
    assert reach[5][0] == 9 and CASES[5][4] == CASES[5][2]
    assert reach[6][0] == TILE and reach[7][0] == TILE + 1
    assert {next(u for u in (16, 8, 4, 2, 1) if nb % u == 0) for nb in ROW_BYTES.values()} == {16, 8, 4, 2, 1}
    chunks = sum(nb // next(u for u in (16, 8, 4, 2, 1) if nb % u == 0) for nb in ROW_BYTES.values())
    assert 20 * chunks > 2 * _cabi.ROLLOUT_BLOCK                # case 1: two blocks stride
    assert 2 * 200 * 3 > 3 * _cabi.ROLLOUT_BLOCK                # case 6: three blocks stride
    assert {nb for c in CASES for nb in c[12]} == {4, 24, 512}


def test_seq_plan_refusals_and_launch_shapes(tmp_path):
    words = _run(_build(tmp_path, "seq_check", []), "plan")
    consts = dict(zip(words[3::2], (int(w) for w in words[4::2])))
    for name in ("SEQ_FLAG_BLOCK", "SEQ_MAX_STATES", "SEQ_MAX_STATE_BYTES"):
        assert consts[name] == getattr(_cabi, name), name


def test_seq_walk_against_the_model(tmp_path):
    check_cases(_build(tmp_path, "seq_check", []), tmp_path, CASES)


def test_seq_walk_under_sanitizers(tmp_path):
    exe = _build(tmp_path, "seq_check_san", SAN)
    _run(exe, "plan")
    check_cases(exe, tmp_path, CASES)
