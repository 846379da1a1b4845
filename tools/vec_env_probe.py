#!/usr/bin/env python3
"""End-to-end rate of VecImageEnv (env_num reference envs in one handle, NeverStopWrapper-style auto-reset), with the episode
placements drawn by the Python EnvPos or inside the library (native_spawn).

    python tools/vec_env_probe.py --envs 1024 --robots 4 --peds 3

--stack IMAGE,STATE,LASER adds the frame stacks of StateBatchWrapper at those depths (the YAML keys), kept by the library
(imgenv_stack_enable); --torch-stack keeps them with torch ops on top of an unstacked VecImageEnv instead -- what a user had to
write before; --stack-compare alternates no stack / library stack / torch stack over several rounds and writes the raw figures."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class TorchStack:
    """StateBatchWrapper per env with torch ops on an unstacked VecImageEnv: shift + torch.where on the per-robot all_down mask"""

    def __init__(self, env, depths):
        import torch
        o = env.world.out
        self.env, self.fields = env, [(f, k) for f, k in zip(("sensor_maps", "vector_states", "lasers"), depths) if k > 0]
        self.stack = {f: torch.zeros((o[f].shape[0], k) + tuple(o[f].shape[1:]), dtype=o[f].dtype, device=o[f].device)
                      for f, k in self.fields}

    def reset(self):
        for f, k in self.fields:
            self.stack[f].zero_()
            self.stack[f][:, -1] = self.env.world.out[f]

    def push(self, all_down):
        import torch
        for f, k in self.fields:
            s, new = self.stack[f], self.env.world.out[f]
            if k > 1:
                keep = ~all_down.view(-1, *([1] * (s.dim() - 1)))
                s[:, :-1] = torch.where(keep, s[:, 1:], torch.zeros((), dtype=s.dtype, device=s.device))
            s[:, -1] = new
        return self.stack


def stack_depths(stack):
    """(image, state, laser) YAML keys -> effective depths (base.py:103-105)"""
    return (max(stack[0], 0), max(stack[1], 0), max(stack[2], 1) if stack[2] >= 0 else 0)


def measure(envs=1024, robots=4, peds=3, obstacles=2, steps=300, time_max=100, natives=(False, True, "device"), stack=None,
            torch_stack=False):
    """robot-steps/s of VecImageEnv over `steps` steps, after the envs have drifted out of phase.  ``stack`` = (image_batch,
    state_batch, laser_batch): with the library's frame stacks, or (``torch_stack``) the same kept by torch ops on top"""
    import torch
    from img_env_amd import worldgen
    from img_env_amd.vec_env import VecImageEnv
    grid = worldgen.make_grid(200, 2)
    out = {}
    for native in natives:
        cfg = worldgen.make_yaml_cfg(robots, peds, grid, time_max=time_max, n_obstacles=obstacles, seed=5)
        if stack is not None:
            cfg.update(image_batch=stack[0], state_batch=stack[1], laser_batch=stack[2])
        env = VecImageEnv(cfg, env_num=envs, seed=5, native_spawn=bool(native), device_reset=native == "device",
                          stack=stack is not None and not torch_stack)
        ts = TorchStack(env, stack_depths(stack)) if stack is not None and torch_stack else None
        n = len(env)
        g = torch.Generator(device="cuda").manual_seed(1)
        acts = torch.zeros(16, n, 3, device="cuda")
        acts[:, :, 0] = torch.rand(16, n, generator=g, device="cuda") * 0.6
        acts[:, :, 1] = torch.rand(16, n, generator=g, device="cuda") * 1.8 - 0.9
        t0 = time.perf_counter()
        env.reset()
        if ts:
            ts.reset()
        torch.cuda.synchronize()
        t_reset = time.perf_counter() - t0
        for s in range(time_max + 20):  # past the first wave of time limits: the envs drift out of phase as robots collide
            _, _, _, info = env.step(acts[s % 16])
            if ts:
                ts.push(info["all_down"])
        torch.cuda.synchronize()
        placed0 = sum(env.world.autoreset_last()[::-1][0:1]) + len(env.world.autoreset_last()[0]) if native == "device" else 0
        resets, t0 = 0, time.perf_counter()
        for s in range(steps):
            _, _, _, info = env.step(acts[s % 16])
            if ts:
                ts.push(info["all_down"])
            if info["reset_envs"] is not None:  # (device-side reset: nothing comes back to the host)
                resets += len(info["reset_envs"])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if native == "device":  # placements handed out meanwhile
            worlds, first = env.world.autoreset_last()
            resets = first + len(worlds) - placed0
        res = dict(robot_steps_per_s=n * steps / dt, us_per_step=1e6 * dt / steps, env_resets_per_step=resets / steps,
                   first_reset_ms=1e3 * t_reset)
        if native is True and stack is None:  # the same steps without the reset half: what NeverStopWrapper costs on top of the step
            env.auto_reset = False
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(steps):
                env.step(acts[s % 16])
            torch.cuda.synchronize()
            res["us_per_step_without_resets"] = 1e6 * (time.perf_counter() - t0) / steps
        out["device_reset" if native == "device" else ("native_spawn" if native else "python_spawn")] = res
        env.close()
    extra = {} if stack is None else dict(stack=list(stack), stack_by="torch" if torch_stack else "library")
    return dict(envs=envs, robots_per_env=robots, peds_per_env=peds, **extra, **out)


def compare_stacks(args, depths_list, rounds=3):
    """no stack / library stack / torch stack, alternating, `rounds` times, per depth setting and reset variant"""
    natives = (True, "device")
    runs = []
    for stack in depths_list:
        for rnd in range(rounds):
            for mode in ("none", "library", "torch"):
                r = measure(args.envs, args.robots, args.peds, args.obstacles, args.steps, args.time_max, natives,
                            stack=None if mode == "none" else stack, torch_stack=mode == "torch")
                for variant in ("native_spawn", "device_reset"):
                    runs.append(dict(depths=list(stack), round=rnd, mode=mode, variant=variant, us_per_step=r[variant]["us_per_step"],
                                     env_resets_per_step=r[variant]["env_resets_per_step"]))
                    print(json.dumps(runs[-1]), flush=True)
    summary = []
    for stack in depths_list:
        for variant in ("native_spawn", "device_reset"):
            row = dict(depths=list(stack), variant=variant)
            for mode in ("none", "library", "torch"):
                v = [r["us_per_step"] for r in runs if r["depths"] == list(stack) and r["variant"] == variant and r["mode"] == mode]
                row[mode] = dict(us_per_step_rounds=v, median=sorted(v)[len(v) // 2], spread=max(v) - min(v))
            row["added_us_library"] = row["library"]["median"] - row["none"]["median"]
            row["added_us_torch"] = row["torch"]["median"] - row["none"]["median"]
            summary.append(row)
    return dict(envs=args.envs, robots_per_env=args.robots, peds_per_env=args.peds, steps=args.steps, time_max=args.time_max,
                rounds=rounds, runs=runs, summary=summary)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--robots", type=int, default=4)
    ap.add_argument("--peds", type=int, default=3)
    ap.add_argument("--obstacles", type=int, default=2)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--time-max", type=int, default=100)
    ap.add_argument("--device-only", action="store_true", help="only the device-side auto-reset variant")
    ap.add_argument("--stack", default=None, metavar="IMAGE,STATE,LASER", help="frame stacks at these depths (the YAML keys)")
    ap.add_argument("--torch-stack", action="store_true", help="keep the stacks with torch ops instead of the library's kernel")
    ap.add_argument("--stack-compare", default=None, metavar="I,S,L[;I,S,L...]",
                    help="no stack / library / torch, alternating over --rounds rounds per depth setting")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="--stack-compare: also write the JSON here")
    args = ap.parse_args()
    if args.stack_compare:
        res = compare_stacks(args, [tuple(int(v) for v in d.split(",")) for d in args.stack_compare.split(";")], args.rounds)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        print(json.dumps(res["summary"]))
        return
    natives = ("device",) if args.device_only else (False, True, "device")
    stack = tuple(int(v) for v in args.stack.split(",")) if args.stack else None
    print(json.dumps(measure(args.envs, args.robots, args.peds, args.obstacles, args.steps, args.time_max, natives, stack=stack,
                             torch_stack=args.torch_stack)))


if __name__ == "__main__":
    main()
