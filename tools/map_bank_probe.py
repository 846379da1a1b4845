#!/usr/bin/env python3
"""What the map bank (include/imgenv.h: imgenv_maps_add) costs the vec_env shape: VecImageEnv(device_reset=True) over
1024 envs x (4 robots + 3 pedestrians), in one process, alternating passes

    a  no bank                                        (the handle as it was before the bank existed)
    b  a bank of 8 maps, policy keep, every env on map 0
    c  8 maps, env k on map k % 8, policy keep        (every reset keeps its map: the sparse map restore)
    d  8 maps, policy placement                       (7 of 8 resets change the map: the full-map restore)

    python tools/map_bank_probe.py --out profiles/map_bank_vec_env.json
    python tools/map_bank_probe.py --passes a --rounds 5          # runs on a tree without the bank too (the parent commit)
    python tools/map_bank_probe.py --shape shipped --envs 256     # the shipped test.yaml geometry: 733 x 733 cells

Per pass and round: microseconds per step and env resets per step over --steps steps, after the envs have drifted out of phase
(tools/vec_env_probe.py's protocol).  The summary gives every pass's median and spread (max - min over the rounds), b / c / d
minus a, and for d the added time per env whose reset changed its map."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_MAPS = 8


def make_cfg(shape, robots, peds, obstacles, time_max, n_maps):
    """(cfg, robots per env): the YAML-schema config of one env of the shape, with ``n_maps`` maps (1: a plain 2-D map)"""
    import numpy as np
    from img_env_amd import worldgen
    if shape == "vec_env":
        grids = [worldgen.make_grid(200, 2 + 17 * m) for m in range(n_maps)]
        cfg = worldgen.make_yaml_cfg(robots, peds, grids[0], time_max=time_max, n_obstacles=obstacles, seed=5)
        if n_maps > 1:
            cfg["global_map"]["map_array"] = np.stack(grids)
        return cfg, robots
    # the reference's shipped envs/cfg/test.yaml: 110 x 110 pixels at 0.1 m resized to 733 x 733 cells, 1 robot + 4 pedestrians
    rng = np.random.default_rng(7)
    grids = []
    for m in range(n_maps):
        g = np.full((110, 110), 255, np.uint8)
        g[:5] = g[-5:] = 0
        g[:, :5] = g[:, -5:] = 0
        for _ in range(3 * (m > 0)):  # rooms 1..: a few pillars each
            r, c = rng.integers(15, 90, 2)
            g[r:r + 5, c:c + 5] = 0
        grids.append(g)
    z = np.load(os.path.join(ROOT, "tests", "golden", "spawn_ref.npz"))
    cfg = worldgen.shipped_test_yaml_cfg("unused.png", json.loads(str(z["test@1/cfg"])))
    cfg.update(seed=5, time_max=time_max)
    cfg["global_map"]["map_array"] = np.stack(grids) if n_maps > 1 else grids[0]
    return cfg, 1


def one_pass(which, args):
    """us per step and env resets per step of one pass"""
    import torch
    from img_env_amd.vec_env import VecImageEnv
    cfg, robots = make_cfg(args.shape, args.robots, args.peds, args.obstacles, args.time_max, 1 if which == "a" else N_MAPS)
    kw = {}
    if which == "b":
        kw = dict(map_policy="keep", world_maps=[0] * args.envs)
    elif which == "c":
        kw = dict(map_policy="keep", world_maps=[k % N_MAPS for k in range(args.envs)])
    elif which == "d":
        kw = dict(map_policy="placement")
    env = VecImageEnv(cfg, env_num=args.envs, seed=5, device_reset=True, **kw)
    try:
        n = len(env)
        g = torch.Generator(device="cuda").manual_seed(1)
        acts = torch.zeros(16, n, 3, device="cuda")
        acts[:, :, 0] = torch.rand(16, n, generator=g, device="cuda") * 0.6
        acts[:, :, 1] = torch.rand(16, n, generator=g, device="cuda") * 1.8 - 0.9
        env.reset()
        for s in range(args.time_max + 20):  # past the first wave of time limits: the envs drift out of phase
            env.step(acts[s % 16])
        worlds, first = env.world.autoreset_last()
        placed0 = first + len(worlds)
        maps0 = env.world_maps() if which != "a" else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(args.steps):
            env.step(acts[s % 16])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        worlds, first = env.world.autoreset_last()
        res = dict(us_per_step=1e6 * dt / args.steps, env_resets_per_step=(first + len(worlds) - placed0) / args.steps,
                   launches_last_step=env.world.launches())
        if which != "a":
            maps1 = env.world_maps()
            res["maps_in_use"] = int(len(set(maps1.tolist())))
            res["envs_on_another_map_than_before"] = int((maps0 != maps1).sum())
        return res
    finally:
        env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("vec_env", "shipped"), default="vec_env")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--robots", type=int, default=4)
    ap.add_argument("--peds", type=int, default=3)
    ap.add_argument("--obstacles", type=int, default=2)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--time-max", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", default="a,b,c,d")
    ap.add_argument("--root", default=ROOT, help="the tree whose img_env_amd is measured (a checkout of another commit)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from img_env_amd import _cabi
    passes = [p for p in args.passes.split(",") if p]
    runs = []
    for rnd in range(args.rounds):
        for which in passes:
            r = dict(round=rnd, **{"pass": which}, **one_pass(which, args))
            runs.append(r)
            print(json.dumps(r), flush=True)
    summary = {}
    for which in passes:
        v = sorted(r["us_per_step"] for r in runs if r["pass"] == which)
        resets = [r["env_resets_per_step"] for r in runs if r["pass"] == which]
        summary[which] = dict(us_per_step_rounds=v, median=v[len(v) // 2], spread=v[-1] - v[0], env_resets_per_step=sum(resets) / len(resets))
    if "a" in summary:
        for which in passes:
            if which != "a":
                summary[which]["minus_a_us"] = summary[which]["median"] - summary["a"]["median"]
    if "c" in summary and "d" in summary:
        # under the placement policy a reset keeps its map with probability 1 / N_MAPS; the rest take the full-map restore
        changing = summary["d"]["env_resets_per_step"] * (N_MAPS - 1) / N_MAPS
        summary["d"]["map_changing_resets_per_step"] = changing
        summary["d"]["added_us_per_map_changing_reset_vs_c"] = (summary["d"]["median"] - summary["c"]["median"]) / changing if changing > 0 else None
    res = dict(shape=args.shape, envs=args.envs, robots_per_env=args.robots if args.shape == "vec_env" else 1,
               peds_per_env=args.peds if args.shape == "vec_env" else 4, steps=args.steps, time_max=args.time_max, rounds=args.rounds,
               n_maps=N_MAPS,
               build_id=_cabi.load_library().imgenv_build_id().decode(), runs=runs, summary=summary)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res["summary"]))


if __name__ == "__main__":
    main()
