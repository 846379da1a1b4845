#!/usr/bin/env python3
"""How much of k_view's first-hit walk the live-beam queue saves, predicted on the CPU from the benchmark's own world.

    python tools/beam_work.py [cfg3] [steps]

The oracle runs bench.py's cfg-3 workload (its layout, the "active" policy) for a few steps; each beam's first-hit step comes
from its `lasers_raw` distance matched against the class's per-step distance table (host_tables.h, dumped by
tests/host/k_view_live_beams_check.cpp), a beam without a hit walks its whole path.  Per robot it counts 64-lane chunk walks:
  * old: every round of 64 beams walks chunks until its LAST beam has hit or ended;
  * live: chunk 0 of every beam, then ceil(alive / 64) rounds per later chunk.
Needs no GPU."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def beam_tables(view_m, res, beams):
    exe = os.path.join(tempfile.mkdtemp(), "k_view_live_beams_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "k_view_live_beams_check.cpp"), "-o", exe])
    out = subprocess.run([exe, str(view_m), str(view_m), str(res), str(beams), "-1.570795", "1.570795", "0", "tables"],
                         capture_output=True, text=True, check=True).stdout.split("\n")
    B, n_chunks = map(int, out[0].split())
    lens, dists = [], []
    for b in range(B):
        v = out[1 + b].split()
        lens.append(int(v[0]))
        dists.append(np.array([float(x) for x in v[1:]], np.float32))
    return n_chunks, np.array(lens), dists


def main():
    import bench
    from oracle_binding import OracleWorld
    cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg3"
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    wl = bench.WORKLOADS[cfg]
    R, P, B = wl["robots"], wl["peds"], wl["beams"]
    n_chunks, lens, dists = beam_tables(wl["view"] * wl["res"], wl["res"], B)
    grid, params, layouts = bench.make_workload(cfg, R, P, 1)
    w = OracleWorld(params, grid)
    w.reset(layouts[0])
    rng = np.random.default_rng(1)
    for _ in range(steps):
        w.step(np.stack([np.zeros(R), rng.uniform(-0.9, 0.9, R), np.zeros(R)], 1).astype(np.float32))
    snap = w.snapshot()
    w.close()
    live = (snap["is_collisions"] == 0) & (snap["is_arrives"] == 0)
    hd = snap["lasers_raw"][live].astype(np.float32)  # [robots, B]
    need = np.empty(hd.shape, np.int32)  # chunks a beam walks: up to its hit, else its whole path
    hit_chunk = np.full(hd.shape, -1, np.int32)
    for b in range(B):
        full = max(1, (lens[b] + 7) // 8)
        has = hd[:, b] < 6.0
        k = np.abs(hd[:, b, None] - dists[b][None, :]).argmin(1) if len(dists[b]) else np.zeros(len(hd), int)
        hit_chunk[has, b] = k[has] // 8
        need[:, b] = np.where(has, np.minimum(k // 8 + 1, full), full)
    n_r = need.shape[0]
    pad = (-B) % 64
    rounds = np.concatenate([need, np.ones((n_r, pad), np.int32)], 1).reshape(n_r, -1, 64)
    old = rounds.max(2).sum(1)
    new = np.full(n_r, (B + 63) // 64)
    for ch in range(1, n_chunks):
        new += (np.count_nonzero(need > ch, 1) + 63) // 64
    print("%s: %d robots walking (of %d), %d beams, %d chunks, %d steps into the run" % (cfg, n_r, R, B, n_chunks, steps))
    for ch in range(n_chunks):
        print("  first hit in chunk %d: %5.1f %% of the beams" % (ch, 100.0 * np.mean(hit_chunk == ch)))
    print("  no hit:               %5.1f %%" % (100.0 * np.mean(hit_chunk < 0)))
    print("  beams alive into chunk c (mean per robot):", [round(float(np.count_nonzero(need > ch, 1).mean()), 1) for ch in range(n_chunks)])
    print("  64-lane chunk walks per robot: old %.2f, live beams %.2f (%.1f %% fewer)" % (old.mean(), new.mean(), 100.0 * (1 - new.mean() / old.mean())))


if __name__ == "__main__":
    main()
