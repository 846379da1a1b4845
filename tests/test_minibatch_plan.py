"""The minibatch kernels (img_env_amd/csrc/minibatch.h) on the CPU, beside tests/test_rollout_plan.py:
tests/host/minibatch_check.cpp compiles the header's flag, scatter, shuffle, statistics and gather functions for the host and runs
them over a simulated grid on seeded cases written here; what it leaves is compared bit for bit with tests/minibatch_model.py.
The cases reach: n R not a multiple of 16 (a tail inside one tile); exactly one tile, one tile plus one flag, more tiles than the scan
workgroup has lanes; no valid transition, all valid; B larger than valid_n, j beyond the last minibatch; every chunk unit (rows of
48, 1448, 20, 6 and 3 bytes: 16 / 8 / 4 / 2 / 1); gather grids of one block and of two blocks that stride, and the planner's.  The
same program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own: is_clean is an
allocation of exactly n R bytes there, so a flag read past the end is found."""
import math
import os
import subprocess

import numpy as np

import minibatch_model as mm
from img_env_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "minibatch_check.cpp")
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


def make_case(seed, R, T, n, B, j, p_clean, row_bytes, n_scalars, normalise, blocks):
    rng = np.random.default_rng(seed)
    TR, total, ring_rows = T * R, n * R, (T + 1) * R
    c = {"TR": TR, "total": total, "R": R, "T": T, "n": n, "B": B, "j": j, "normalise": None if normalise < 0 else normalise,
         "seed": int(rng.integers(0, 2 ** 63)) * 2 + 1, "norm": np.array([0.25, 2.0], np.float32), "eps": 1e-8}
    c["is_clean"] = (rng.random((T, R)) < p_clean).astype(np.uint8) * rng.integers(1, 256, (T, R)).astype(np.uint8)  # (any non-zero byte counts)
    c["fields"] = {name: rng.integers(0, 256, (T + 1, R, nb), dtype=np.uint8) for name, nb in row_bytes.items()}
    c["ring"] = {"actions": rng.standard_normal((T, R, 3)).astype(np.float32), "rewards": rng.standard_normal((T, R)).astype(np.float32),
                 "dones": (rng.random((T, R)) < 0.2).astype(np.uint8), "dones_info": rng.integers(0, 11, (T, R)).astype(np.int32)}
    c["x"] = (1.0 + rng.standard_normal((T, R))).astype(np.float32)
    c["scalars"] = [rng.standard_normal((T + 1, R)).astype(np.float32) for _ in range(n_scalars)]
    lo, hi = mm.split_seed(c["seed"])
    blob = [np.array([TR, total, ring_rows, B, j, len(row_bytes), n_scalars, normalise, blocks], "<i4").tobytes(), np.array([lo, hi], "<u4").tobytes(),
            c["norm"].tobytes(), np.array([c["eps"]], "<f8").tobytes(), np.array(list(row_bytes.values()), "<i4").tobytes(), c["is_clean"].tobytes()]
    blob += [a.tobytes() for a in c["fields"].values()]
    blob += [c["ring"][k].tobytes() for k in ("actions", "rewards", "dones", "dones_info")] + [c["x"].tobytes()] + [a.tobytes() for a in c["scalars"]]
    return b"".join(blob), c


def read_result(path, TR, B, row_bytes):
    raw = np.fromfile(path, np.uint8)
    at = [0]

    def take(dtype, shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = raw[at[0]:at[0] + n].view(dtype).reshape(shape)
        at[0] += n
        return a
    r = {"valid_n": int(take("<i4", (1,))[0]), "valid": take("<i4", (TR,)), "order": take("<i4", (TR,)), "stats": take("<f4", (2, 2))}
    for name, nb in row_bytes.items():
        r["mb_" + name] = take(np.uint8, (B, nb))
    for name, dt, shape in (("mb_actions", "<f4", (B, 3)), ("mb_rewards", "<f4", (B,)), ("mb_dones", np.uint8, (B,)), ("mb_dones_info", "<i4", (B,)),
                            ("mb_index", "<i4", (B,)), ("mb_weight", "<f4", (B,)), ("mb_scalars", "<f4", (_cabi.MB_MAX_SCALARS, B))):
        r[name] = take(dt, shape)
    assert at[0] == raw.size
    return r


# (seed, R, T, n, B, j, share of clean flags, rows, scalars, normalise, gather blocks)
CASES = [
    (0, 15, 6, 6, 32, 0, 0.8, ROW_BYTES, 3, 1, 0),       # 90 flags: a tail of 10 inside one tile; every chunk unit; the planner's grid
    (1, 15, 6, 6, 32, 2, 0.8, ROW_BYTES, 3, 1, 2),       # its last minibatch: slots behind the valid list; two blocks stride
    (2, 15, 6, 5, 32, 9, 0.8, SMALL, 1, -1, 1),          # j beyond the last minibatch, the cursor below the horizon
    (3, 7, 5, 5, 64, 0, 0.0, SMALL, 2, 0, 0),            # no valid transition: B > valid_n = 0
    (4, 7, 5, 5, 64, 0, 1.0, SMALL, 6, 5, 1),            # all valid, 35 < B; six scalars
    (5, 64, 64, 64, 100, 40, 0.5, SMALL, 1, 0, 0),       # exactly one tile (4096 flags)
    (6, 4097, 1, 1, 100, 3, 0.9, SMALL, 0, -1, 0),       # one tile plus one flag
    (7, 4099, 3, 2, 256, 1, 0.87, {"e1": 3}, 1, 0, 3),   # two tiles and a tail of 6 in the third, n < T
    (8, 4096, 257, 257, 512, 2000, 0.24, {"e1": 1}, 0, -1, 0),  # 257 tiles: the scan's second round, with a carry
    (9, 4099, 256, 256, 512, 0, 0.99, {"e1": 1}, 0, -1, 0),     # 257 tiles, the last one partial
]


def check_cases(exe, tmp_path, cases):
    worst = 0.0
    for case in cases:
        seed, R, T, n, B, j, p, row_bytes, n_scalars, normalise, blocks = case
        blob, c = make_case(*case)
        path, result = tmp_path / ("case%d.bin" % seed), tmp_path / ("result%d.bin" % seed)
        path.write_bytes(blob)
        words = _run(exe, "run", path, result)
        got = read_result(result, c["TR"], B, row_bytes)
        valid = mm.valid_list(c["is_clean"], n)
        V = len(valid)
        assert int(words[2]) == V == got["valid_n"], seed
        assert int(words[4]) == -(-c["total"] // TILE), seed
        assert got["valid"][:V].tobytes() == valid.tobytes(), seed
        order = mm.order_list(valid, c["TR"], c["seed"])
        assert got["order"].tobytes() == order.tobytes(), seed
        # the statistics: the kernels' order of sums bit for bit, two runs the same bits, and the error against math.fsum
        want = mm.stats(c["x"], valid, c["total"], c["eps"])
        assert got["stats"][0].tobytes() == got["stats"][1].tobytes() == want.tobytes(), (seed, got["stats"], want)
        if V:
            v = c["x"].reshape(-1)[valid].astype(np.float64)
            mean = math.fsum(v) / V
            var = math.fsum((v - mean) ** 2) / V
            assert abs(float(got["stats"][0][0]) - mean) <= np.spacing(np.float32(mean)), seed
            inv = 1.0 / math.sqrt(var + c["eps"])
            worst = max(worst, abs(float(got["stats"][0][1]) - inv) / float(np.spacing(np.float32(inv))))
        else:
            assert got["stats"][0].tolist() == [0.0, 1.0]
        mb = mm.gather(order, j, B, c["fields"], c["ring"], c["scalars"], c["normalise"], c["norm"])
        for name in mb:
            if name == "mb_scalars":
                assert got[name][:n_scalars].tobytes() == mb[name].tobytes(), seed
                assert not got[name][n_scalars:].any()
            else:
                assert got[name].tobytes() == mb[name].tobytes(), (seed, name)
    assert worst <= 1.0, worst  # (float32 ulps of 1 / sqrt(var + eps): the final rounding alone)
    return worst


def test_what_the_cases_reach():
    reach = {c[0]: (c[1] * c[3], len(mm.valid_list(make_case(*c)[1]["is_clean"], c[3]))) for c in CASES[:8]}
    assert reach[0][0] == 90 and reach[0][0] % 16 == 10
    assert reach[1][1] < 3 * 32 and reach[1][1] > 2 * 32  # minibatch 2 is the last one, partly empty
    assert reach[2][1] < 9 * 32
    assert reach[3][1] == 0 and reach[4] == (35, 35)
    assert reach[5][0] == TILE and reach[6][0] == TILE + 1 and reach[7][0] == 2 * TILE + 6
    assert all(-(-c[1] * c[3] // TILE) > _cabi.MB_SCAN_BLOCK for c in CASES[8:])
    assert {next(u for u in (16, 8, 4, 2, 1) if nb % u == 0) for nb in ROW_BYTES.values()} == {16, 8, 4, 2, 1}
    chunks = sum(nb // next(u for u in (16, 8, 4, 2, 1) if nb % u == 0) for nb in ROW_BYTES.values())
    assert 32 * chunks > 2 * _cabi.ROLLOUT_BLOCK  # case 1: two blocks stride


def test_minibatch_plan_and_launch_shapes(tmp_path):
    words = _run(_build(tmp_path, "minibatch_check", []), "plan")
    consts = dict(zip(words[3::2], (int(w) for w in words[4::2])))
    for name in ("MB_INDEX_BLOCK", "MB_LANE_FLAGS", "MB_TILE", "MB_SCAN_BLOCK", "MB_STATS_BLOCK", "MB_STATS_PER_LANE", "MB_SHUFFLE_BLOCK", "MB_ROUNDS",
                 "MB_MAX_SCALARS"):
        assert consts[name] == getattr(_cabi, name), name
    assert (mm.STATS_BLOCK, mm.STATS_PER_LANE, mm.ROUNDS) == (_cabi.MB_STATS_BLOCK, _cabi.MB_STATS_PER_LANE, _cabi.MB_ROUNDS)


def test_minibatch_walk_against_the_model(tmp_path):
    check_cases(_build(tmp_path, "minibatch_check", []), tmp_path, CASES)


def test_minibatch_walk_under_sanitizers(tmp_path):
    exe = _build(tmp_path, "minibatch_check_san", SAN)
    _run(exe, "plan")
    check_cases(exe, tmp_path, CASES)
