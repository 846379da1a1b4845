"""csrc/policy.h's host/device rules and launch_plan.h's plan_policy_launch on the CPU: tests/host/policy_check.cpp compiles them
with g++, walks them over a simulated grid for every group width and compares with vectors that tests/policy_model.py writes --
Philox outputs, the counter of a robot shard (a non-zero robot_begin), the block partition, and, for given e[], the lane sums, the
scan, s, the target and the chosen index bit for bit, bad rows included.  The launch shapes at A = 1 ... 4096 and R = 1, 256, 257
and the Gaussian row's rules are asserted inside the program."""
import os
import subprocess

import numpy as np

import policy_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _hex(a):
    return " ".join("%x" % int(x) for x in np.asarray(a).view(np.uint32).ravel())


def _vectors():
    rng = np.random.default_rng(2024)
    lines = []
    for ctr, key in [((0, 0, 0, 0), (0, 0)), ((0xffffffff,) * 4, (0xffffffff,) * 2),
                     ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))] + \
                    [(tuple(rng.integers(0, 2 ** 32, 4)), tuple(rng.integers(0, 2 ** 32, 2))) for _ in range(20)]:
        out = pm.philox(ctr, key)
        lines.append("PHILOX " + " ".join("%x" % int(x) for x in list(ctr) + list(key) + list(out)))
    for g, draw, seed, second in [(0, 0, 0, 0), (12345, 7, 99, 0), (2 ** 32 + 5, (9 << 32) | 4, (3 << 32) | 1, 1), (4095, 2 ** 63, 2 ** 64 - 1, 1)]:
        out = pm.draw_block(np.array([g], np.uint64), draw, seed, second=bool(second))[0]
        lines.append("DRAW %x %x %x %x %x %x %x " % (g & pm.MASK, g >> 32, draw & pm.MASK, draw >> 32, seed & pm.MASK, seed >> 32, second)
                     + " ".join("%x" % int(x) for x in out))
    shapes = [(1, 5), (3, 9), (16, 9), (17, 257), (40, 9), (64, 9), (65, 9), (100, 7), (256, 5), (257, 5), (1000, 3), (1024, 3), (1025, 3), (4096, 2)]
    for q, (A, R) in enumerate(shapes):
        for det in (0, 1):
            G, g0, draw, seed = pm.group(A), 1000 * q + 3, (q << 32) | (5 + det), 77 + q
            l = pm.make_logits(rng, R, A, (0.0, 1.0, 8.0, 30.0)[q % 4], masked=0.3)
            # given e[]: any positive float32 for an unmasked action (1 for a row's maximum), 0 for a masked one
            m = l.max(axis=1)
            e = np.where(np.isfinite(l), rng.uniform(1e-6, 1.0, l.shape), 0.0).astype(F32)
            e[l == m[:, None]] = 1
            if R >= 5 and A >= 3:  # bad rows: a NaN, a +inf, nothing finite
                l[1, A - 1] = np.nan
                l[2, A // 2] = np.inf
                l[3, :] = -np.inf
            u = pm.u01(pm.draw_block(np.arange(R, dtype=np.uint64) + np.uint64(g0), draw, seed)[:, 0])
            out = pm.categorical_f32(l, u, deterministic=bool(det), e=e)
            lines.append("CAT %d %d %d %d %d %x %x %x %x" % (R, A, G, det, g0, draw & pm.MASK, draw >> 32, seed & pm.MASK, seed >> 32))
            for r in range(R):
                lines.append("ROW %d %d %s %s" % (int(out["bad"][r]), int(out["index"][r]), _hex(out["s"][r:r + 1]), _hex(out["target"][r:r + 1])))
                lines.append("L " + _hex(l[r]))
                lines.append("E " + _hex(e[r]))
                lines.append("P " + _hex(out["part"][r]))
                lines.append("S " + _hex(out["scan"][r]))
    return "\n".join(lines) + "\n"


def test_policy_rules_on_a_simulated_grid(tmp_path):
    exe, vec = str(tmp_path / "policy_check"), str(tmp_path / "vectors.txt")
    with open(vec, "w") as fh:
        fh.write(_vectors())
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "policy_check.cpp"), "-o", exe])
    out = subprocess.run([exe, vec], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
