#!/usr/bin/env python3
"""bench.py -- robot-steps/sec of the img_env step() path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run does only what the headline needs: it sets the world up, spins the clocks up, warms up, times ONE pass of exactly
K steps (no HIP event inside it) and prints the JSON line (`value`, `ms_per_step` = that pass's milliseconds per step).
`--dump-outputs DIR` then writes what the last timed step handed its caller (every `imgenv_out` array of rank 0, as float32 /
float64 .npy files; the large per-robot arrays as a fixed, seeded sample of robots, `sample_robots.npy`).  `--full` adds
everything else the line used to carry: the median of 5 passes with the dominant kernel under HIP events, the per-kernel
breakdown and roofline, the uninstrumented and with-reset passes, the CPU baseline, the secondary policies and
configurations (`episode_policy`, `spec_policy`, `full_rewrite`, `multi_world`, `vec_env`, `shipped`) and, on cfg-4, the
comparison of the crowd's first step with the oracle.

N > 1 works both ways: launched by `python -m torch.distributed.run --nproc-per-node N ...` (RANK / WORLD_SIZE in the
environment), or plainly as above -- the parent process then starts one child per GPU itself (it never touches a GPU) and
relays rank 0's JSON line.

Workload (BASELINE.json metric, configs[2] = SURVEY "cfg-3"): ONE world with 8192 robots and 200 ORCA pedestrians
(rvoscene) on a 400x400 occupancy grid, 48x48 sensor_map + 3-channel ped_map, 360-beam laser.  A step is one env.step()
of every robot: pedestrian advance, pose integrate, rasters, collision + crop + laser + stamp, observation + reward/done.
Inputs (actions) are resident in HBM.  Episodes end by the time limit (time_max = 100) and are followed by a full reset
inside the timed region, like NeverStopWrapper does.

Multi-GPU (`--gpus N`): the world's robots are sharded contiguously over the ranks; the one exchange per step is an RCCL
all-gather of the robot records between pose integration and the robot raster.  Pedestrians are
advanced redundantly on every rank.  Two BASELINE configurations:
  * `--config cfg3` (default; the `metric`'s wording, "whole node at 8192 robots"): the SAME 8192-robot world on the same
    400x400 grid at every N, 8192 / N robots per rank -- STRONG scaling;
  * `--config cfg4` (BASELINE configs[3]): 8192 robots PER GPU beside 200 social-force pedestrians (pedscene) on the 400x400
    grid at 0.5 m, i.e. 65 536 robots at N = 8 -- WEAK scaling (the layout of tests/test_gpu_parity.py::
    test_cfg4_full_size_and_shard_match_oracle: the crowd stays inside libpedsim's 10 m root square, robots are no crowd members).

Two action policies are timed, both on the same world:
  * "active"  (the reported `value`): v = 0, w ~ U(-0.9, 0.9).  Robots turn in place, so no robot
    collides or arrives and EVERY robot-step runs the full view path -- the conservative number.
  * "episode": the reference's random policy v ~ U(0, 0.6), w ~ U(-0.9, 0.9) (env_test.py:8-19).  In a
    shared world this freezes most robots within a few steps (collided robots take the early-out of
    agent.cpp:358-360), which makes steps cheaper; reported as `episode_value` with its frozen fraction.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

ROBOTS = 8192     # cfg-3: robots of the world (all GPUs together); cfg-4: robots per GPU
ROBOTS_PER_GPU = ROBOTS
N_PEDS = 200
GRID = 400
TIME_MAX = 100

#: the BASELINE configurations bench.py can time (worldgen.PRESETS holds the same numbers); `robots` is the world's robot count for
#: "strong" scaling (the same world at every GPU count), the robots PER GPU for "weak" and "replicas"
#: cfg3 res / clearance: SURVEY 8(d) density rule for 8192 robots on 400x400: R*0.25 m^2 <= 0.5*(Hg*res)^2 -> 0.25 m; starts 0.7 m
#: apart, so that two r=0.17 m footprints never share a 0.25 m cell at reset
WORKLOADS = {
    "cfg2": dict(scene="", res=0.125, clearance=1.0, relation_ped_robo=1, scaling="replicas", ped_box=None, robots=1024, peds=0, grid=400,
                 view=48, beams=360,
                 name="cfg-2: one world of %(RL)d robots per GPU (x %(N)d GPUs: independent replicas, no exchange), no pedestrians"),
    "cfg3": dict(scene="rvoscene", res=0.25, clearance=0.7, relation_ped_robo=1, scaling="strong", ped_box=None, robots=8192, peds=200,
                 grid=400, view=48, beams=360,
                 name="cfg-3: one world, %(R)d robots (%(RL)d per GPU x %(N)d GPUs%(strong)s), %(P)d ORCA peds (rvoscene)"),
    "cfg4": dict(scene="pedscene", res=0.5, clearance=0.5, relation_ped_robo=0, scaling="weak", ped_box=(0.5, 9.5), robots=8192, peds=200,
                 grid=400, view=48, beams=360,
                 name="cfg-4: one world, %(R)d robots (%(RL)d per GPU x %(N)d GPUs, weak scaling: 65536 at 8 GPUs), %(P)d social-force "
                      "peds (pedscene, inside libpedsim's 10 m root square)"),
    "cfg5": dict(scene="ervoscene", res=0.125, clearance=0.7, relation_ped_robo=1, scaling="strong", ped_box=None, robots=8192, peds=1000,
                 grid=800, view=96, beams=720,
                 name="cfg-5: one world, %(R)d robots (%(RL)d per GPU x %(N)d GPUs%(strong)s), %(P)d ERVO peds (ervoscene), the "
                      "LDS-pressure case"),
}
RES, CLEARANCE = WORKLOADS["cfg3"]["res"], WORKLOADS["cfg3"]["clearance"]


def grid_cells(n_gpus=1):
    """BASELINE's 400x400 at every GPU count (the tools' name for it)"""
    return GRID


def make_workload(cfg_name, R, P, n_layouts, robot_begin=0, robot_end=None, sort_x=False, seed0=100):
    """grid, params and reset layouts of a BASELINE configuration with R robots in the world"""
    from img_env_amd import worldgen
    wl = WORKLOADS[cfg_name]
    grid = worldgen.make_grid(wl["grid"], 0)
    layouts = [worldgen.make_layout(grid, wl["res"], R, P, seed=seed0 + s, clearance=wl["clearance"]) for s in range(n_layouts)]
    for lay in layouts:
        if wl["ped_box"] is not None:  # libpedsim's quadtree covers x in [0, 10], y in [10, 20] only (pedscene.h:18): the crowd stays in its square
            rng = np.random.default_rng(13)
            lo, hi = wl["ped_box"]
            lay.ped_pose[:, :2] = rng.uniform(lo, hi, (P, 2))
            lay.ped_traj[:, :, :2] = rng.uniform(lo, hi, lay.ped_traj[:, :, :2].shape)
            lay.ped_goal[:] = rng.uniform(lo, hi, (P, 2))
        if sort_x:
            # robots are numbered along x, so that a rank's contiguous shard is a vertical strip of the map: each rank then
            # rasterises only the robots its own strip can see (the library clips to the shard's bounding box + view reach)
            order = np.argsort(lay.robot_pose[:, 0], kind="stable")
            lay.robot_pose = lay.robot_pose[order].copy()
            lay.robot_goal = lay.robot_goal[order].copy()
    params = worldgen.make_params(R, P, res=wl["res"], view_cells=wl["view"], beams=wl["beams"], scene=wl["scene"], time_max=TIME_MAX,
                                  relation_ped_robo=wl["relation_ped_robo"], robot_begin=robot_begin,
                                  robot_end=R if robot_end is None else robot_end)
    return grid, params, layouts


def algorithmic_bytes(P, hv=48, wv=48, beams=360, max_ped=None):
    """SURVEY 8(d) per robot-step (the variant that materialises the f16 copy of the sensor map, as this build
    does), split by the kernel that moves them"""
    max_ped = P if max_ped is None else max_ped
    view = hv * wv + hv * wv + 2 * hv * wv + 4 * beams   # grid window gather + sensor_map u8 + f16 copy + lasers f32
    obs = (20 * P + 3 * 48 * 48 * 4 + 4 * (1 + 7 * max_ped)) if P > 0 else 0
    state = 128
    return dict(k_view=view, k_obs=obs, tail=state, total=view + obs + state)  # tail: the per-robot scalars, run inside k_view / k_obs


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _oracle_world(cfg_name, n_robots, n_peds, seed):
    """an oracle world of the benchmark's geometry (TEST / BASELINE infrastructure: bench.py's cpu_baseline leg only)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle_binding import OracleWorld
    grid, params, layouts = make_workload(cfg_name, n_robots, n_peds, 1, seed0=seed)
    w = OracleWorld(params, grid)
    w.reset(layouts[0])
    return w


def _oracle_run(w, n_robots, seconds, max_steps, start_at=None):
    rng = np.random.default_rng(1)
    if start_at is not None:  # all workers start together
        while time.time() < start_at:
            time.sleep(0.005)
    steps, t0 = 0, time.perf_counter()
    while True:
        a = np.stack([np.zeros(n_robots), rng.uniform(-0.9, 0.9, n_robots), np.zeros(n_robots)], 1).astype(np.float32)
        w.step(a)
        steps += 1
        if time.perf_counter() - t0 > seconds or steps >= max_steps:
            break
    return steps, time.perf_counter() - t0


def cpu_worker(args):
    """one process of the all-core CPU baseline (`bench.py --cpu-worker ...`, started by cpu_baseline): its own world of
    R / k robots beside the benchmark's 200 pedestrians on the benchmark's map -- the reference's env_num idiom (one
    single-threaded node per env, create_launch.py:57-66).  Never imports torch, never touches a GPU."""
    n = args.cpu_worker_robots
    w = _oracle_world(args.config, n, args.peds, seed=1000 + args.cpu_worker)
    steps, dt = _oracle_run(w, n, args.cpu_worker_seconds, 10 ** 9, start_at=args.cpu_worker_start)
    w.close()
    print(json.dumps(dict(worker=args.cpu_worker, robots=n, steps=steps, seconds=dt)))


def cpu_baseline(cfg_name, params, grid, layout, peds, seconds=6.0, all_core_seconds=6.0):
    """The CPU oracle (literal single-thread C restatement of the reference, `kind: "port"`) on this box's host cores:
    (a) ONE thread on the very world the GPU timed (8192 robots in one shared world), and
    (b) ALL cores the way the reference itself scales on a CPU -- one single-threaded process per core, each its own world of
        R / cores robots with the same 200 pedestrians and map (env_num independent nodes); `value` is (b)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle_binding import OracleWorld
    import subprocess
    p = dict(params)
    p["robot_begin"], p["robot_end"] = 0, p["n_robots"]
    R = p["n_robots"]
    # (one thread on the GPU's own world where a step of it takes seconds -- cfg-3 / cfg-4; a 1024-robot world of the same
    # geometry where it would take minutes: cfg-5's 1000 pedestrians and 96 x 96 views)
    R1 = R if cfg_name in ("cfg3", "cfg4") else min(R, 1024)
    if R1 == R:
        w = OracleWorld(p, grid)
        w.reset(layout)
    else:
        w = _oracle_world(cfg_name, R1, peds, seed=100)
    steps, dt = _oracle_run(w, R1, seconds, 50)
    w.close()
    single = R1 * steps / dt
    cores = os.cpu_count() or 1
    try:
        cores = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        pass
    def all_cores(per):
        start = time.time() + 6.0 + 0.02 * cores  # imports + world set-up of every worker fit in here
        procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cpu-worker", str(k), "--cpu-worker-robots", str(per),
                                   "--cpu-worker-seconds", str(all_core_seconds), "--cpu-worker-start", repr(start), "--peds", str(peds), "--config", cfg_name],
                                  stdout=subprocess.PIPE, stderr=subprocess.DEVNULL) for k in range(cores)]
        total, slowest, ok = 0.0, 0.0, 0
        for pr in procs:
            out, _ = pr.communicate()
            try:
                r = json.loads(out.decode().strip().splitlines()[-1])
            except Exception:
                continue
            total += r["robots"] * r["steps"] / r["seconds"]
            slowest = max(slowest, r["seconds"])
            ok += 1
        return total, ok, slowest

    # (b1) the benchmark's R robots split over the cores; (b2) the same with 1024 robots per world, where the per-world costs
    # (200 pedestrians, map copy) weigh less -- more robots in total than the GPU stepped, but the better robot-steps/s
    per = max(1, R // cores)
    split, ok1, t1 = all_cores(per)
    big, ok2, t2 = all_cores(1024) if per != 1024 else (split, ok1, t1)
    best = max(split, big)
    return dict(value=best if (ok1 or ok2) else None, unit="robot-steps/s", cores=max(ok1, ok2), kind="port", cpu_model=_cpu_model(),
                nproc=cores, single_thread_value=single, all_cores_split_world_value=split, all_cores_1024_robot_worlds_value=big,
                sample="all cores: %d single-threaded oracle processes side by side (one per hardware thread, the reference's env_num "
                       "idiom), each its own world + %d %s peds on the configuration's map @%.3f m, v=0 policy: %d robots per world (the "
                       "benchmark's %d split over the cores, %.1f s) and 1024 robots per world (%.1f s); value = the better of the two; "
                       "single_thread_value: 1 thread, %d steps of a %d-robot shared world of the GPU's geometry, %.1f s.  kind \"port\": the "
                       "oracle keeps ONE shared owner layer per world where the reference copies the whole map once per robot and step "
                       "(img_env.cpp:623) -- the reference itself would be slower than this figure, which therefore flatters the CPU"
                       % (max(ok1, ok2), peds, WORKLOADS[cfg_name]["scene"] or "no", WORKLOADS[cfg_name]["res"], per, R, t1, t2, steps, R1, dt))


def launch_ranks(args):
    """`python bench.py --gpus N` without a launcher: this parent (which makes no GPU call at all -- children are started
    as child processes, nothing is exec'ed over a GPU context) starts one rank per GPU and relays rank 0's line."""
    import socket
    import subprocess
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    out, _ = procs[0].communicate()
    rcs = [procs[0].returncode] + [pr.wait() for pr in procs[1:]]
    lines = [ln for ln in out.decode().splitlines() if ln.startswith("{")]
    if lines:
        print(lines[-1])
    rc = max(abs(c) for c in rcs)
    if rc or not lines:
        raise SystemExit("bench.py: ranks exited with %s%s" % (rcs, "" if lines else " and rank 0 printed no result line"))


def first_step_ped_velocities(cfg_name, peds):
    """cpu_baseline leg (the oracle, before this process touches a GPU), cfg-4 only: the velocities the CPU oracle -- linked
    against the host's glibc atan2, as the reference is -- gives the social-force crowd on the FIRST step of a handle's first
    episode.  The crowd ignores the robots, so a one-robot world holds the same crowd.  bench.py compares the library's own
    first step with it and prints how many pedestrians differ (`sfm_first_step_sign_flips`): the documented exception to the
    1e-4 bar (ped_agent.cpp:352-360: sign of a rounding residue while the whole crowd stands still)."""
    w = _oracle_world(cfg_name, 1, peds, seed=100)
    w.step(np.zeros((1, 3), np.float32))
    v = np.array(w.snapshot()["ped_state"][:, 2:4], np.float64)
    w.close()
    return v


DUMP_LIMIT = 60 << 20        # bytes of the whole dump at most
DUMP_ROBOTS = 512            # robots of the fixed sample the large per-robot arrays are cut to (fewer where they would not fit)
DUMP_WHOLE_BYTES = 4 << 20   # an array at most this large (after the dtype widening) is written whole


def dump_outputs(world, out_dir):
    """`--dump-outputs DIR`: every array imgenv_out hands the caller after the last timed step, as DIR/<name>.npy -- float64
    stays float64, int32 widens to float64, everything else (u8 / i8 / f16 / f32) to float32, all exactly.  Per-robot arrays
    larger than DUMP_WHOLE_BYTES keep the rows of a fixed, seeded sample of robots (sorted; DIR/sample_robots.npy), so that the
    dump stays under DUMP_LIMIT (~30 MB at cfg-3) and two builds are compared on the same robots."""
    os.makedirs(out_dir, exist_ok=True)
    n = world.n_local
    arrays = {}
    for name, a in sorted(world.snapshot().items()):
        arrays[name] = a.astype(np.float64 if a.dtype in (np.float64, np.int32, np.int64, np.uint32) else np.float32)
    big = [k for k, a in arrays.items() if a.nbytes > DUMP_WHOLE_BYTES and a.ndim >= 1 and a.shape[0] == n]
    whole = sum(a.nbytes for k, a in arrays.items() if k not in big)
    per_robot = sum(arrays[k].nbytes // n for k in big)
    if big:
        k_rob = max(1, min(n, DUMP_ROBOTS, (DUMP_LIMIT - whole) // max(per_robot, 1)))
        sample = np.sort(np.random.default_rng(20240613).permutation(n)[:k_rob])
        for k in big:
            arrays[k] = arrays[k][sample]
        arrays["sample_robots"] = sample.astype(np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", choices=sorted(WORKLOADS), default="cfg3", help="BASELINE configuration: cfg3 = the metric's 8192-robot "
                    "world, strong-scaled over the GPUs (default); cfg4 = 8192 robots per GPU beside 200 social-force pedestrians, weak scaling; "
                    "cfg2 = 1024 robots without pedestrians (independent replicas on N GPUs); cfg5 = 8192 robots, 1000 ERVO pedestrians, 96x96 "
                    "views, 720 beams on 800x800, strong-scaled")
    ap.add_argument("--robots-per-gpu", type=int, default=None, help="diagnostic: robots per GPU instead of the configuration's")
    ap.add_argument("--peds", type=int, default=None, help="diagnostic: pedestrians instead of the configuration's")
    ap.add_argument("--full", action="store_true", help="measure everything beyond the headline as well: per-kernel breakdown, "
                    "roofline, CPU baseline, the secondary policies and configurations, 5 passes with the dominant kernel under HIP events")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed (rank 0's "
                    "imgenv_out arrays) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baseline")
    ap.add_argument("--no-episode", action="store_true", help="(--full) skip the secondary policies (episode_policy, spec_policy) and full_rewrite")
    ap.add_argument("--no-multi-world", action="store_true", help="(--full) skip the secondary env_num-style measurements")
    ap.add_argument("--spinup", type=int, default=2000, help="untimed steps before the warm-up (clock ramp)")
    ap.add_argument("--timing-mode", type=int, default=2, help="(--full) diagnostic: 0 = no HIP events in the timed passes")
    ap.add_argument("--repeat", type=int, default=0, help="(--full) diagnostic: extra timed passes, printed to stderr")
    ap.add_argument("--passes", type=int, default=None, help="timed passes of the SAME --steps; value = the median pass "
                    "(default: 1, with --full 5)")
    ap.add_argument("--force-dist", action="store_true", help="initialise torch.distributed (RCCL) and use the "
                    "step_begin / all_gather / step_end path even with one rank (exercises the multi-GPU code on one GPU)")
    ap.add_argument("--cpu-worker", type=int, default=None, help=argparse.SUPPRESS)  # internal: one process of the all-core CPU baseline
    ap.add_argument("--cpu-worker-robots", type=int, default=32, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-worker-seconds", type=float, default=8.0, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-worker-start", type=float, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    wl = WORKLOADS[args.config]
    if args.peds is None:
        args.peds = wl["peds"]
    if args.passes is None:
        args.passes = 5 if args.full else 1
    if args.cpu_worker is not None:
        return cpu_worker(args)
    if "RANK" not in os.environ and (args.gpus > 1 or os.environ.get("IMGENV_BENCH_FORCE_LAUNCHER")):
        return launch_ranks(args)  # (the env switch lets a one-GPU box exercise the parent / child relay with --gpus 1)

    import torch
    import torch.distributed as dist
    from img_env_amd import _cabi
    from img_env_amd.world import World

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    if world_size != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (launch with torch.distributed.run)" % (args.gpus, world_size))
    replicas = wl["scaling"] == "replicas"  # every rank its own world: no shard, no exchange
    if args.robots_per_gpu:  # diagnostic override: that many robots on every rank, whatever the configuration says
        RL = args.robots_per_gpu
    elif wl["scaling"] == "strong":
        if wl["robots"] % world_size:
            raise SystemExit("bench.py: %d robots do not split over %d GPUs" % (wl["robots"], world_size))
        RL = wl["robots"] // world_size
    else:
        RL = wl["robots"]
    R = RL if replicas else RL * world_size   # robots of ONE world
    R_job = RL * world_size                   # robots the whole job steps
    P = args.peds
    res = wl["res"]
    side = wl["grid"]
    n_layouts = 2 + (args.steps + args.warmup) // (TIME_MAX + 1)
    shard = not replicas and world_size > 1
    grid, params, layouts = make_workload(args.config, R, P, min(n_layouts, 4 if R <= 16384 else 2), robot_begin=rank * RL if shard else 0,
                                          robot_end=(rank + 1) * RL if shard else R, sort_x=shard, seed0=100 + (1000 * rank if replicas else 0))

    # The CPU baseline runs FIRST, before this process makes its first GPU call: its all-core leg starts worker processes,
    # and nothing may be started from a process that holds a GPU context on this pool.
    cpu_base, oracle_first_v = None, None
    if args.full and world_size == 1 and not args.no_cpu_baseline and not args.force_dist:
        try:
            cpu_base = cpu_baseline(args.config, dict(params), grid, layouts[0], P)
        except Exception as e:
            cpu_base = {"value": None, "unit": "robot-steps/s", "cores": 0, "kind": "port", "sample": "failed: %r" % (e,)}
        if args.config == "cfg4" and P > 0:
            try:
                oracle_first_v = first_step_ped_velocities(args.config, P)
            except Exception:
                oracle_first_v = None

    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world_size > 1 or args.force_dist
    exchange = use_dist and not replicas
    comm_ranks = 0
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist.init_process_group("nccl", rank=rank, world_size=world_size, device_id=dev)

    sfm_flips = None
    if oracle_first_v is not None:  # (cfg-4, one GPU) the library's first step of its first episode against the glibc-linked oracle's
        w0 = World(dict(params), grid, device=local_rank)
        w0.reset(layouts[0])
        w0.step(torch.zeros(RL, 3, device=dev))
        v0 = w0.snapshot()["ped_state"][:, 2:4]
        w0.close()
        dv = np.abs(v0 - oracle_first_v).max(axis=1)
        sfm_flips = dict(count=int((dv > 1e-9).sum()), of=int(P), max_abs_dv=float(dv.max()),
                         what="pedestrians whose first-step velocity (first episode of a handle: the crowd at rest) differs from the CPU oracle linked "
                              "against the host's glibc atan2 -- the device's atan2 is correctly rounded, glibc's is not; ped_agent.cpp:352-360, INTEGRATION.md")

    world = World(params, grid, device=local_rank)
    if world.lib.imgenv_backend() != b"hip-gfx950":
        raise SystemExit("bench.py: %r is not the product library (experiment / profile build)" % world.lib.imgenv_backend())
    r0, r1 = (rank * RL, (rank + 1) * RL) if shard else (0, RL)
    native = False
    if exchange:
        try:  # preferred: the library runs ncclAllGather itself, on the step's stream
            world.init_comm(rank, world_size)
            native = True
        except Exception as e:  # fall back to torch.distributed's collective between step_begin / step_end
            if rank == 0:
                print("bench.py: native RCCL exchange unavailable (%s); using torch.distributed.all_gather" % e, file=sys.stderr)
        flags = [None] * world_size
        dist.all_gather_object(flags, native)
        native = all(flags)
        comm_ranks = world.comm_info()[0] if native else 0

    g = torch.Generator(device=dev).manual_seed(1 + rank)
    n_act = 16

    def make_actions(policy):
        # generated on the device: a pageable host-to-device copy here leaves a deferred un-pin behind in the HIP runtime
        # that was seen to stall kernel submission for ~30 ms a few dozen steps later
        a = torch.zeros(n_act, RL, 3, device=dev)
        if policy in ("episode", "spec"):  # env_test.py:8-19
            a[:, :, 0] = torch.rand(n_act, RL, generator=g, device=dev) * 0.6
        a[:, :, 1] = torch.rand(n_act, RL, generator=g, device=dev) * 1.8 - 0.9
        return a

    # The actions are pre-generated and resident in HBM before the timed region starts (BASELINE / SURVEY 8d); the steps are
    # plain stream-ordered imgenv_step calls -- what a trainer whose policy writes the actions on the stream makes.
    ctx = dict(world=world, time_max=TIME_MAX)
    state = dict(elapsed=0, episode=0, resets=0)

    def do_reset():
        ctx["world"].reset(layouts[state["episode"] % len(layouts)])
        state["episode"] += 1
        state["elapsed"] = 0
        state["resets"] += 1

    def do_step(a):
        w = ctx["world"]
        if exchange and not native:
            w.step_begin(a)
            dist.all_gather_into_tensor(w.records, w.records[r0:r1])
            w.step_end()
        else:
            w.step(a)
        state["elapsed"] += 1
        if state["elapsed"] > ctx["time_max"]:  # TimeLimitWrapper has set done for every robot: NeverStopWrapper resets
            do_reset()

    def run(policy, steps, warmup, timing_mode=0, which=-1):
        w = ctx["world"]
        acts = make_actions(policy)
        state["episode"] = 0
        do_reset()
        for s in range(warmup):
            do_step(acts[s % n_act])
        frozen0 = int(w.out["counters"][3].item())
        resets0 = state["resets"]
        w.timing(timing_mode, which)
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if os.environ.get("BENCH_TRACE"):  # diagnostic: where inside a pass does the time go (adds a sync every 20 steps)
            tw, marks = t0, []
            for s in range(steps):
                e0 = state["episode"]
                do_step(acts[s % n_act])
                if state["episode"] != e0:
                    marks.append(s)
                if s % 20 == 19:
                    torch.cuda.synchronize()
                    now = time.perf_counter()
                    print("  trace %s steps %d-%d: %.1f us/step%s" % (policy, s - 19, s, 1e6 * (now - tw) / 20,
                                                                  " reset@%s" % marks if marks else ""), file=sys.stderr)
                    tw, marks = now, []
        else:
            for s in range(steps):
                do_step(acts[s % n_act])
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        dt = time.perf_counter() - t0
        tm = w.timing_read()
        w.timing(0)
        if use_dist:
            t = torch.tensor([dt], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        frozen = int(w.out["counters"][3].item()) - frozen0
        state["resets_timed"] = state["resets"] - resets0
        return dt, tm, frozen / float(steps * RL)

    # pass 1 (not the headline): per-kernel breakdown, HIP events around every kernel, one sync per step;
    # the median over steps is robust against first-launch and host-submission hiccups
    def kernel_breakdown(steps=40):
        acts = make_actions("active")
        state["episode"] = 0
        do_reset()
        for s in range(5):
            do_step(acts[s % n_act])
        world.timing(1)
        prev = {k: (0.0, 0) for k in world.timing_read()}
        samples = {k: [] for k in prev}
        for s in range(steps):
            do_step(acts[s % n_act])
            cur = world.timing_read()
            for k, (ms, n) in cur.items():
                if n > prev[k][1]:
                    samples[k].append(1e3 * (ms - prev[k][0]) / (n - prev[k][1]))
            prev = cur
        world.timing(0)
        return {k: (float(np.median(v)) if v else 0.0) for k, v in samples.items()}

    # (--full only: a plain run times its pass without any HIP event and has no roofline to price)
    per_kernel_us, per_rank_kernel_us, dominant, longest_kernel, dom_id = None, None, None, None, -1
    if args.full:
        per_kernel_us = kernel_breakdown()
        # every rank's kernel times (and the exchange's duration) travel with the line: a scaling curve then explains itself
        if use_dist:
            gathered = [None] * world_size
            dist.all_gather_object(gathered, {k: round(v, 2) for k, v in per_kernel_us.items() if v})
            per_rank_kernel_us = gathered
        # dominant = the per-robot kernel with the longest launch.  k_orca is left out: it is 200 single-wave workgroups of
        # serial LP code that idle along on a side stream underneath k_view (latency, not work) and moves no per-robot bytes
        # ... and so are the move and the rasters (k_integrate, k_raster, k_move_raster: a wavefront's chain of dependent round trips over 128
        # bytes of state per robot; SURVEY 8(d) gives them no bytes to price) as long as a kernel that moves the observation's bytes ran:
        # on cfg-2 k_move_raster and k_view<..., 8> are within a microsecond of each other, and which one is "longest" is a coin toss
        latency_kernels = ("k_orca", "rccl_all_gather", "k_integrate", "k_raster", "k_move_raster", "k_remote")
        longest_kernel = max((k for k in per_kernel_us if k not in ("k_orca", "rccl_all_gather")), key=per_kernel_us.get)
        priced = [k for k in per_kernel_us if k not in latency_kernels and per_kernel_us[k] > 0]
        dominant = max(priced, key=per_kernel_us.get) if priced else longest_kernel
        dom_id = list(per_kernel_us).index(dominant)
    timing_mode = args.timing_mode if args.full else 0
    # untimed spin-up: the first ~second of sustained work after start-up runs at lower clocks than steady state
    if args.spinup > 0:
        run("active", args.spinup, 0)
    # pass 2: THE timed region; with --full HIP events only around the dominant kernel, none in a plain run
    # Several passes of exactly --steps steps each, every one bracketed by barrier + synchronize; the MEDIAN pass is the line's
    # value (boxes of the pool alternate between two step times from process to process and pass to pass, and the driver's 20-step
    # region is 2.5 ms long), min / max are reported beside it
    passes = []
    for q in range(max(1, args.passes)):
        d_q, tm_q, fr_q = run("active", args.steps, args.warmup if q == 0 else min(args.warmup, 5), timing_mode=timing_mode, which=dom_id)
        passes.append((d_q, tm_q, fr_q, state["resets_timed"]))
    if args.dump_outputs and rank == 0:
        dump_outputs(world, args.dump_outputs)
    order = sorted(range(len(passes)), key=lambda q: passes[q][0])
    dt, tm, frozen_active, resets_timed = passes[order[len(order) // 2]]
    value = R_job * args.steps / dt
    pass_values = [R_job * args.steps / p[0] for p in passes]
    # ... and the same passes once more WITHOUT the HIP events around the dominant kernel (every 8th launch carries a pair, and an
    # event operation is a dependency bubble on its stream: the timed region above pays just under 1 % for carrying the roofline's
    # measurement inside it).  Reported beside `value`, never instead of it.
    uninstrumented = None
    if args.full and args.timing_mode != 0 and world_size == 1:
        d0 = sorted(run("active", args.steps, min(args.warmup, 5), timing_mode=0)[0] for _ in range(3))[1]
        uninstrumented = dict(value=R_job * args.steps / d0, ms_per_step=1e3 * d0 / args.steps,
                              what="median of 3 more passes of the same %d steps with no HIP event in the timed region" % args.steps)
    # SURVEY 8(d) wants the auto-reset inside the timed region; a run shorter than an episode (the driver's 20 steps) never meets
    # one, so it is timed separately: the same N steps + ONE full imgenv_reset of the world
    with_reset = None
    if args.full and args.steps <= TIME_MAX:
        acts_r = make_actions("active")
        state["episode"] = 0
        do_reset()
        for s in range(min(args.warmup, 5)):
            do_step(acts_r[s % n_act])
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()
        t0r = time.perf_counter()
        for s in range(args.steps):
            do_step(acts_r[s % n_act])
        do_reset()
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        dtr = time.perf_counter() - t0r
        if use_dist:
            t = torch.tensor([dtr], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dtr = float(t.item())
        with_reset = dict(value=R_job * args.steps / dtr, ms_per_step=1e3 * dtr / args.steps,
                          what="%d steps + one full imgenv_reset of the world inside the timed region" % args.steps)
    for q in range(args.repeat if args.full else 0):
        for mode in (0, 2):
            d2, _, _ = run("active", args.steps, args.warmup, timing_mode=mode, which=dom_id)
            d3, _, _ = run("episode", args.steps, args.warmup, timing_mode=mode, which=dom_id)
            if rank == 0:
                print("repeat %d timing mode %d: active %.1f us/step, episode %.1f us/step"
                      % (q, mode, 1e6 * d2 / args.steps, 1e6 * d3 / args.steps), file=sys.stderr)
    episode = None
    if args.full and not args.no_episode:
        dte, _, frozen_ep = run("episode", args.steps, args.warmup)
        episode = dict(value=R_job * args.steps / dte, frozen_fraction=frozen_ep,
                       what="v~U(0,0.6), w~U(-0.9,0.9) at the configuration's time_max %d: a shared world freezes most robots within a few steps" % TIME_MAX)

    launches_per_step = world.launches()
    layer_mode = world.layer_mode()

    # SURVEY 8(d)'s own action distribution (env_test.py:8-19: v~U(0,0.6), w~U(-0.9,0.9)) with the frozen fraction held under
    # 10 % the way the spec says -- by the auto-reset: robots of one shared world run into each other within a few steps and
    # freeze (agent.cpp:358-360), so the episode's time limit is set to the longest T whose frozen robot-steps stay below 9 %
    # (measured on an untimed episode), and every episode ends in a full reset INSIDE the timed region.
    spec_policy = None
    if args.full and not args.no_episode and world_size == 1 and not args.force_dist:
        try:
            acts_s = make_actions("spec")
            ctx["time_max"] = 10 ** 9
            state["episode"] = 0
            do_reset()
            f0, cum = int(world.out["counters"][3].item()), []
            for t in range(40):
                do_step(acts_s[t % n_act])
                cum.append(int(world.out["counters"][3].item()) - f0)
            T = 0
            for t in range(1, 41):
                if cum[t - 1] / float(t * RL) < 0.09:
                    T = t
            spawn_frozen = None
            if T == 0:  # this layout's robots overlap at the reset already (cfg-4's 0.5 m cells): no time limit holds 10 %; said, not hidden
                spawn_frozen = cum[0] / float(RL)
                T = 10
            ctx["time_max"] = TIME_MAX
            sp = dict(params)
            sp["time_max"] = T
            w_spec = World(sp, grid, device=local_rank)
            ctx["world"], ctx["time_max"] = w_spec, T
            n_spec = max(args.steps, 3 * (T + 1))
            run("spec", 80, 0)  # (untimed: past the 64 calls during which a fresh handle's default output guard checksums and synchronises)
            res_s = sorted((run("spec", n_spec, T + 1) + (state["resets_timed"],) for _ in range(3)), key=lambda r: r[0])[1]
            spec_policy = dict(value=R_job * n_spec / res_s[0], ms_per_step=1e3 * res_s[0] / n_spec, frozen_fraction=res_s[2], time_max=T,
                               steps=n_spec, resets_in_timed_region=res_s[3], frozen_at_the_first_step=spawn_frozen,
                               what="SURVEY 8(d) actions v~U(0,0.6), w~U(-0.9,0.9); time_max = the longest episode whose frozen robot-steps stay "
                                    "below 9 %% (%d steps on this layout); a full imgenv_reset whenever the time limit runs out, inside the timed "
                                    "region; median of 3 passes" % T)
            w_spec.close()
        except Exception as e:  # a secondary number must never cost the headline line
            spec_policy = {"error": repr(e)}
        ctx["world"], ctx["time_max"] = world, TIME_MAX

    # The safe boundary: IMGENV_FLAG_FULL_REWRITE hands out copies rewritten in full by every call (the reference's ownership,
    # img_env.cpp:745-749) -- the same passes under it
    full_rewrite = None
    if args.full and not args.no_episode and world_size == 1 and not args.force_dist:
        try:
            w_fr = World(dict(params, output_guard="copy"), grid, device=local_rank)
            ctx["world"] = w_fr
            run("active", 300, 0)
            d_fr = sorted(run("active", args.steps, min(args.warmup, 5))[0] for _ in range(3))[1]
            full_rewrite = dict(value=R_job * args.steps / d_fr, ms_per_step=1e3 * d_fr / args.steps, copy_bytes_per_step=int(w_fr.arena.numel()),
                                what="the same passes on a handle created with IMGENV_FLAG_FULL_REWRITE: imgenv_outputs() hands out a second "
                                     "arena that receives a complete device-to-device copy at the end of every call; median of 3 passes")
            w_fr.close()
        except Exception as e:
            full_rewrite = {"error": repr(e)}
        ctx["world"] = world

    multi_world = None
    if args.full and world_size == 1 and args.config == "cfg3" and not args.no_multi_world and not args.force_dist:
        # secondary: the reference's own env_num idiom -- E independent worlds of R/E robots at
        # 0.125 m in ONE handle, every world with its own obstacle map, crowd and time limit, reset on its own when its
        # time limit runs out (imgenv_reset_worlds); no collective, so N GPUs simply hold N times the worlds
        world.close()
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from multiworld_probe import measure
        try:
            multi_world = [measure(E, RL // E, pw, 200, res=0.125, steps=args.steps, warmup=300, time_max=TIME_MAX, kernels=False,
                                   device=local_rank) for E, pw in ((64, 16), (RL, 0))]
        except Exception as e:  # a secondary number must never cost the headline line
            multi_world = {"error": repr(e)}

    vec_env = None
    if args.full and world_size == 1 and args.config == "cfg3" and not args.no_multi_world and not args.force_dist:
        # secondary: the trainer's end-to-end loop -- 1024 reference envs of 4 robots behind VecImageEnv (the wrapper stack's
        # outputs, NeverStopWrapper-style resets inside the library), Python call to Python return: with the device-side reset
        # (the value) and with the host in the loop
        try:
            from vec_env_probe import measure as measure_vec
            v = measure_vec(1024, 4, 3, 2, steps=args.steps, natives=(True, "device"))
            dv, hv = v["device_reset"], v["native_spawn"]
            vec_env = dict(value=dv["robot_steps_per_s"], unit="robot-steps/s", envs=1024, robots_per_env=4, peds_per_env=3,
                           mode="imgenv_step_autoreset_device: finished envs found, placed and reset by kernels alone",
                           **{k: dv[k] for k in ("us_per_step", "env_resets_per_step")},
                           host_in_the_loop=dict(value=hv["robot_steps_per_s"], us_per_step=hv["us_per_step"],
                                                 mode="imgenv_step_autoreset: placements drawn on the host while the device steps"))
        except Exception as e:
            vec_env = {"error": repr(e)}

    shipped = None
    if args.full and world_size == 1 and args.config == "cfg3" and not args.no_multi_world and not args.force_dist:
        # secondary: the geometry of the reference's shipped envs/cfg/test.yaml (BASELINE cfg-1): 400 x 400 cell views shrunk to
        # 48 x 48, 1000 beams, one robot + 4 leg pedestrians + 4 obstacles per env, VecImageEnv end to end with auto-resets
        try:
            from shipped_probe import measure as measure_shipped
            shipped = [measure_shipped(E, steps=max(args.steps, 100), device=local_rank) for E in (256, 2048)]
        except Exception as e:
            shipped = {"error": repr(e)}

    if rank == 0:
        build_id = world.lib.imgenv_build_id().decode()
        out = {
            "metric": "robot-steps/sec (whole node) at 8192 robots, 48x48 maps, 360 lasers",
            "value": value, "unit": "robot-steps/s", "n_gpus": world_size, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True,
            "scaling": "weak" if replicas else wl["scaling"], "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": (wl["name"] % dict(R=R, RL=RL, N=world_size, P=P, strong="" if world_size == 1 else
                                                      ": strong scaling, the same world at every GPU count")) +
                                   ", %dx%d grid @%.3f m, %dx%d sensor_map + 3ch ped_map, %d-beam laser, time_max %d, full reset whenever the "
                                   "time limit runs out (%d inside the %d timed steps)" % (side, side, res, wl["view"], wl["view"], wl["beams"],
                                                                                           TIME_MAX, resets_timed, args.steps),
                       "baseline_config": args.config,
                       "robots": R_job, "peds": P, "grid": side, "resolution": res, "view": wl["view"], "beams": wl["beams"],
                       "policy": "active: v=0, w~U(-0.9,0.9): every robot-step runs the full view path (spec_policy: SURVEY 8(d)'s own actions)",
                       "parallelism": (("%d independent replicas, no exchange" % world_size) if replicas else
                                       "robot-sharded x%d, RCCL all-gather of robot records (%s)" % (
                                           world_size, ("ncclAllGather inside imgenv_step, communicator of %d ranks as reported by RCCL" % comm_ranks)
                                           if native else "torch.distributed between step_begin/step_end"))
                       if use_dist else "single GPU"},
            "resets_in_timed_region": resets_timed,
            "passes": {"n": len(passes), "value_is": "median", "values": pass_values, "min": min(pass_values), "max": max(pass_values)},
            "actions": "pre-generated in HBM; plain stream-ordered imgenv_step (IMGENV_STEP_ACTIONS_READY is without effect since round 6)",
            "frozen_fraction": frozen_active,
            "build_id": build_id,
            "launches_per_step": launches_per_step,
            "layer_mode": layer_mode,
            "full": bool(args.full),
        }
    if rank == 0 and args.full:
        dom_ms, dom_n = tm[dominant]
        ab = algorithmic_bytes(P, hv=wl["view"], wv=wl["view"], beams=wl["beams"])
        kernel_bytes = ab.get(dominant, ab["total"]) * RL
        dur_s = (dom_ms / dom_n) * 1e-3 if dom_n else float("nan")
        achieved = kernel_bytes / dur_s / 1e9
        traffic, path_traffic, traffic_source = None, None, None
        # counters: profiles/pmc_<config>.json (pmc_latest.json = the headline's, its name since round 1), collected by
        # tools/profile_cfg.sh on a named build
        pmc = os.path.join(ROOT, "profiles", "pmc_latest.json" if args.config == "cfg3" else "pmc_%s.json" % args.config)
        counters_ok = False  # the committed counters describe THIS library (same sources + flags), or they are not quoted
        default_shape = world_size == 1 and RL == wl["robots"] and P == wl["peds"] and not args.force_dist
        counters = {}
        if os.path.exists(pmc) and default_shape:
            try:
                counters = json.load(open(pmc))
                pmc_id = counters.get("build_id")
                counters_ok = pmc_id == build_id
                if counters_ok:
                    traffic = counters.get(dominant, {}).get("hbm_bytes_per_launch")
                    # every kernel of a step once (k_reset_apply is not part of a step)
                    # (nor are the output guard's checksum kernels of a handle's first 64 calls, or the once-per-process gate probe)
                    path_traffic = sum(v["hbm_bytes_per_launch"] for k, v in counters.items()
                                       if k.startswith("k_") and not k.startswith(("k_reset", "k_out_", "k_gate_probe", "k_state")) and k != "k_cell_base"
                                       and isinstance(v, dict))
                    traffic_source = ("profiles/%s, collected on build %s = the library of this run: rocprofv3 --pmc FETCH_SIZE and "
                                      "--pmc WRITE_SIZE passes (separate runs, gfx950 corrections) over this same bench command -- committed "
                                      "with the build, NOT collected during this run" % (os.path.basename(pmc), pmc_id))
                else:
                    traffic_source = ("none: profiles/%s was collected on build %s, this run's library is %s (imgenv_build_id) -- "
                                      "counters of another build are not quoted" % (os.path.basename(pmc), pmc_id, build_id))
            except Exception:
                traffic = None
        # instruction-issue ceiling of the dominant kernel: wavefronts x vector instructions per wavefront (SQ_INSTS_VALU of the
        # committed counter passes) x cycles per wave64 instruction (tools/micro/valu_issue.hip on this chip: 4.2 for everything
        # but plain add / and, which take 2.4) over 1024 SIMDs
        issue = None
        try:
            cnt = counters.get(dominant, {}) if counters_ok else {}
            if cnt.get("valu_per_wave"):
                waves, vpw = cnt["waves_per_launch"], cnt["valu_per_wave"]
                lo, hi = (waves * vpw * c / (1024 * 2.4e9) * 1e6 for c in (2.4, 4.2))
                issue = {"valu_per_wave": vpw, "waves_per_launch": waves, "cycles_model": "4.2 cycles per wave64 VALU instruction per SIMD "
                         "(2.4 for v_add_u32 / v_and_b32), 1024 SIMDs at 2.4 GHz: profiles/r3_valu_issue.txt", "ceiling_us": hi,
                         "ceiling_us_if_all_were_adds": lo, "frac": hi / (dur_s * 1e6), "source": "profiles/%s (SQ passes)" % os.path.basename(pmc)}
        except Exception:
            issue = None
        out.update({
            "uninstrumented": uninstrumented,
            "with_reset": with_reset,
            "spec_policy": spec_policy,
            "full_rewrite": full_rewrite,
            "shipped": shipped,
            "multi_world": multi_world,
            "vec_env": vec_env,
            "episode_policy": episode,
            "kernel_us": per_kernel_us,
            "per_rank_kernel_us": per_rank_kernel_us,  # N > 1: every rank's kernels and `rccl_all_gather`, the in-library exchange
            "roofline": {"bound": "hbm", "kernel": dominant, "longest_kernel_by_events": longest_kernel, "achieved": achieved, "peak": 8000.0, "unit": "GB/s",
                         "frac": achieved / 8000.0, "traffic": traffic, "traffic_source": traffic_source,
                         # the same fraction from the COUNTERS' bytes of the dominant kernel: what it really moved (a kernel that
                         # updates its output sparsely -- k_obs and the ped_map -- moves far less than the algorithmic figure)
                         "frac_by_counters": (traffic / dur_s / 1e9 / 8000.0) if traffic else None,
                         # HBM bytes of ALL kernels of one step (same counters) and what that is per second at the measured rate
                         "path_traffic_bytes_per_step": path_traffic,
                         "path_traffic_frac": (path_traffic / (dt / args.steps) / 1e9 / 8000.0) if path_traffic else None,
                         "algorithmic_bytes_per_robot_step": ab, "kernel_avg_us": dur_s * 1e6,
                         "units_per_launch": RL,
                         # SURVEY 8(d)'s algorithmic bytes of the whole path over the whole step time.  NOT evidence of HBM use:
                         # k_obs updates the ped_map sparsely and writes ~6 KB per robot, not the 37 KB the formula counts --
                         # path_traffic_frac above is the counter-based figure
                         "path_algorithmic_gbps": ab["total"] * value / world_size / 1e9,
                         "issue": issue},
        })
        if sfm_flips is not None:
            out["sfm_first_step_sign_flips"] = sfm_flips
        if cpu_base is not None:
            out["cpu_baseline"] = cpu_base
    world.close()
    if use_dist:
        dist.destroy_process_group()
    if rank == 0:
        # the JSON line is the LAST thing on stdout: RCCL prints its version banner through C stdio, whose buffer would otherwise
        # only be flushed at exit, behind the line
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
