#!/usr/bin/env python3
"""End-to-end rate of VecImageEnv (env_num reference envs in one handle, NeverStopWrapper-style auto-reset), with the episode
placements drawn by the Python EnvPos or inside the library (native_spawn).

    python tools/vec_env_probe.py --envs 1024 --robots 4 --peds 3

--stack IMAGE,STATE,LASER adds the frame stacks of StateBatchWrapper at those depths (the YAML keys), kept by the library
(imgenv_stack_enable); --torch-stack keeps them with torch ops on top of an unstacked VecImageEnv instead -- what a user had to
write before; --stack-compare alternates no stack / library stack / torch stack over several rounds and writes the raw figures.

--episodes adds the per-robot episode statistics of TestEpisodeWrapper kept by the library (imgenv_episodes_enable);
--torch-episodes keeps the same figures with EpisodeStats and torch ops on top of a plain VecImageEnv; --episodes-compare
alternates no statistics / library / torch over several rounds and writes the raw figures.  --episode-log adds the per-episode
log on top of the statistics (imgenv_episode_log_enable: one more launch per reset chain); --episode-log-compare alternates no
statistics / statistics / statistics + log over several rounds -- the device_reset variant runs a reset chain with every step, so
its difference between the last two is what the log's launch costs a reset chain.  --final-obs-compare alternates the final
observations (VecImageEnv(final_obs=True), imgenv_final_obs_enable: one more launch per reset chain) off / on in the same way.
--normalise-compare alternates, with the device-side reset, the running normalisation of vector_states and rewards off / kept by
the library (VecImageEnv(normalise={...}), imgenv_normalise_enable: two more launches per chain) / kept by TorchNormalise's torch ops.
--policy-compare alternates, with the device-side reset, wrappers=True and rollout=--horizon, the hop from logits over 11 actions
to the stepped env done by the policy head (VecImageEnv(policy={...}).policy_step: one launch instead of the decode's) / by
torch.distributions.Categorical (sample, log_prob, entropy, three stores into [T, n] tensors, then step on the indices).
--loss-compare alternates, in one process, PPO's loss of one real minibatch of --batch rows -- from logits over 11 actions and
values on the device to the gradients on them -- done by VecImageEnv(policy=dict(seed=s, loss=True)).policy_loss and backward()
(imgenv_policy_loss: three launches) / by the same loss in torch ops and autograd; the two gradients are compared first.

--rollout-compare runs device_reset steps three ways, one process per measurement, alternating over several rounds: no rollout
storage, the library's (VecImageEnv(rollout=--horizon), imgenv_rollout_enable: one more launch per chain, a new window every
--horizon steps) and the same arrays kept by torch on top of the first (buf[t].copy_(x) per field and scalar, the final rows taken
whole from final_obs=True); then the advantage pass (imgenv_rollout_gae) against a torch loop over t for a rollout of 128 steps.

--minibatch-compare times one PPO epoch of minibatches of --batch transitions over a full window of --horizon device_reset steps,
two ways, one process per measurement, alternating over several rounds: the library's (VecImageEnv(minibatch=B):
imgenv_rollout_index + _stats + _shuffle and one gather launch per minibatch, no host read) and the same tensors from torch ops on
the library's ring (nonzero on is_clean, masked mean / std, randperm, one index_select per field and scalar).

--sequences-compare times one epoch of SEQUENCE minibatches (--seq-length steps x --seq-batch sequences, time-major, two 512-byte
state arrays) over the same window the same two ways: the library's (VecImageEnv(sequences=dict(...)): imgenv_rollout_seq_index +
_seq_shuffle and one gather launch per minibatch) and torch ops on the library's ring (chunk flags by reshape / any, nonzero,
randperm, one index_select per field and scalar).

--ped-draw-compare runs device_reset steps with rollout=--horizon and the default fields two ways, one process per measurement,
alternating over several rounds: ped_maps stored in the ring / drawn at gather time from the stored pedestrian vectors
(rollout_draw_ped_maps=True; --parent-tree adds the stored path of another checkout); per variant the time per step, the device time
per minibatch of --batch transitions, the ring's bytes and, drawn, k_ped_draw alone against a copy of the bytes it writes.

--wrappers table|clip feeds the policy's raw output (indices into a 28-row table, or float rows to be clipped) to
VecImageEnv(wrappers=True): decode, speeds, normalised pedestrian vectors and close_to_human kept by the library;
--torch-wrappers keeps the same with torch ops on top of a plain VecImageEnv; --wrappers-compare alternates pre-decoded actions
with nothing enabled / library / torch over several rounds, for the table and for the clip, and writes the raw figures.

--tracks-compare (with --peds 10) runs the dataset pedestrian scene -- recorded crowds of --records records per pedestrian --
three ways, alternating over several rounds: a Python loop that reads all_down and uploads the finished envs' tracks in explicit
batches (what a handle without a track bank can do), native_spawn with the bank (imgenv_tracks_add) and device_reset with it.

--scenarios-compare runs a fixed list of --scenarios recorded episodes (the reference's cfg_type: bag): "python_loop" (imgenv_step, a
host read of all_down, reset_worlds with layouts from the list -- the only way without a scenario bank), "scenarios"
(device_reset=True, scenarios=...), "sampler" (device_reset=True drawing fresh placements) and, with --parent-tree DIR, "parent"
(the sampler variant with img_env_amd imported from another, built checkout: the commit before the bank).  Every variant of every
round is a process of its own (--scenarios-variant), alternating."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv[1:-1]:  # (its value follows it) import img_env_amd from another checkout (A/B against another commit, same tool)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
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


class TorchEpisodes:
    """TestEpisodeWrapper per robot with torch ops on a plain VecImageEnv: ``EpisodeStats.add`` every step, then the fold of the
    envs that restarted as ``torch.where`` on the per-robot all_down mask (no host synchronisation: the best a user could write)"""
    FIGURES = ("w_variance", "w_zero", "v_acc", "w_acc", "v_jerk", "w_jerk", "v_avg", "w_avg")
    CODES = (5, 10, 1, 2, 3)

    def __init__(self, env, min_steps=3):
        import torch
        from img_env_amd.envs import EpisodeStats
        n, dev = len(env), env.world.device
        self.env, self.min_steps = env, int(min_steps)
        self.stats = EpisodeStats(n, float(env.cfg["control_hz"]), dev)
        f64 = lambda *shape: torch.zeros(*shape, n, dtype=torch.float64, device=dev)  # noqa: E731
        i64 = lambda *shape: torch.zeros(*shape, n, dtype=torch.int64, device=dev)  # noqa: E731
        self.steps, self.ep_len, self.ep_return = i64(), i64(), f64()
        self.ends, self.figure_sums = i64(6), f64(8)
        self.episodes, self.short_episodes, self.speed_steps, self.arrive_steps, self.len_sum = i64(), i64(), i64(), i64(), i64()
        self.v_sum, self.w_sum, self.return_sum = f64(), f64(), f64()

    def reset(self):
        """every env has just been reset for the first time: nothing to fold"""
        self.steps.zero_()
        self.ep_len.zero_()
        self.ep_return.zero_()

    def push(self, actions, rewards, info):
        import torch
        st = self.stats
        clean = info["is_clean"] != 0
        zero = torch.zeros((), dtype=torch.float64, device=actions.device)
        v, w = torch.where(clean, actions[:, 0].double(), zero), torch.where(clean, actions[:, 1].double(), zero)
        self.steps += 1
        self.v_sum += v
        self.w_sum += w.abs()
        st.add(v, w)
        self.ep_return += rewards
        self.ep_len += clean
        down, codes = info["all_down"], info["dones_info"]
        counted = down & (self.steps > self.min_steps)
        c = counted.to(torch.int64)
        bins = torch.full_like(codes, 5)
        for b, code in enumerate(self.CODES):
            bins = torch.where(codes == code, b, bins)
        self.ends.scatter_add_(0, bins.view(1, -1).long(), c.view(1, -1))
        self.episodes += c
        self.short_episodes += (down & ~counted).to(torch.int64)
        self.speed_steps += c * self.steps
        self.arrive_steps += c * (codes == 5) * self.steps
        n = st.n.clamp(min=1)
        n1, n2 = (st.n - 1).clamp(min=1), (st.n - 2).clamp(min=1)
        mean_w = st.sum_w / n
        fig = torch.stack([st.sum_ww / n - mean_w * mean_w, st.w_zero, st.sum_abs_acc[0] / n1, st.sum_abs_acc[1] / n1,
                           st.sum_abs_jerk[0] / n2, st.sum_abs_jerk[1] / n2, st.sum_v / n, st.sum_absw / n])
        fig = torch.where(torch.arange(8, device=fig.device).view(-1, 1) == 1, fig, torch.round(fig * 1e4) / 1e4)
        self.figure_sums += torch.where(counted, fig, zero)
        self.return_sum += torch.where(counted, self.ep_return, zero)
        self.len_sum += c * self.ep_len
        for name in ("n", "sum_v", "sum_w", "sum_ww", "sum_absw", "w_zero"):
            setattr(st, name, torch.where(counted, zero, getattr(st, name)))
        for name in ("sum_abs_acc", "sum_abs_jerk", "prev", "prev2"):
            setattr(st, name, [torch.where(counted, zero, t) for t in getattr(st, name)])
        self.steps = torch.where(down, 0, self.steps)
        self.ep_len = torch.where(down, 0, self.ep_len)
        self.ep_return = torch.where(down, zero, self.ep_return)

    def statistics(self):
        """the keys of ``VecImageEnv.episode_statistics()``; synchronises"""
        ends = [int(x) for x in self.ends.sum(dim=1).cpu()]
        fig = dict(zip(self.FIGURES, (float(x) for x in self.figure_sums.sum(dim=1).cpu())))
        n, steps = max(1, int(self.episodes.sum())), max(1, int(self.speed_steps.sum()))
        return dict(arrive_rate=ends[0] / n, static_coll_rate=ends[2] / n, ped_coll_rate=ends[3] / n, other_coll_rate=ends[4] / n,
                    avg_arrive_steps=int(self.arrive_steps.sum()) / max(1, ends[0]), stuck_rate=ends[1] / n,
                    avg_v=float(self.v_sum.sum()) / steps, avg_w=float(self.w_sum.sum()) / steps, avg_w_variance=fig["w_variance"] / n,
                    avg_v_jerk=fig["v_jerk"] / n, avg_w_jerk=fig["w_jerk"] / n, avg_w_zero=fig["w_zero"] / n, aborted_rate=ends[5] / n,
                    episodes=int(self.episodes.sum()), short_episodes=int(self.short_episodes.sum()),
                    avg_return=float(self.return_sum.sum()) / n, avg_len=int(self.len_sum.sum()) / n)


TABLE28 = [[v, w] for v in (0.0, 0.2, 0.4, 0.6) for w in (-0.9, -0.6, -0.3, 0.0, 0.3, 0.6, 0.9)]  # the shape of the shipped YAMLs' table
WRAPPER_LIST = ["VelActionWrapper", "TimeLimitWrapper", "SensorsPaperRewardWrapper", "InfoLogWrapper", "MultiRobotCleanWrapper",
                "StatePedVectorWrapper"]


class TorchWrappers:
    """what ``VecImageEnv(wrappers=True)`` hands out, kept with torch ops around a plain VecImageEnv: ``VelActionWrapper.action``'s
    torch path (img_env_amd/envs.py) in front of the step; behind it the speeds masked by the step's ``is_clean``, the pedestrian
    vectors normalised under a mask of the per-row counts (no ``.item()``: no host synchronisation) and ``ped_min_dists < 1``"""

    def __init__(self, env):
        import torch
        from img_env_amd import _cabi
        from img_env_amd.envs import VelActionWrapper
        self.env, dev = env, env.world.device
        self.vel = VelActionWrapper(None, env.cfg)
        self.max_ped = int(env.cfg["max_ped"])
        self.avg = torch.tensor(_cabi.PED_NORM_AVG, dtype=torch.float64, device=dev)
        self.std = torch.tensor(_cabi.PED_NORM_STD, dtype=torch.float64, device=dev)
        self.slots = torch.arange(self.max_ped, device=dev).view(1, -1, 1)

    def action(self, raw):
        return self.vel.action(raw)

    def after(self, a, info):
        import torch
        o = self.env.world.out
        speeds = a[:, :2] * info["is_clean"].unsqueeze(1).to(a.dtype)
        p = o["ped_vector_states"]
        body = p[:, 1:].view(p.shape[0], self.max_ped, 7)
        normed = ((body.double() - self.avg) / self.std).float()
        n = p[:, 0].clamp(max=self.max_ped).long().view(-1, 1, 1)
        norm = torch.cat([p[:, :1], torch.where(self.slots < n, normed, body).view(p.shape[0], -1)], dim=1)
        close = o["ped_min_dists"] < 1
        return speeds, norm, close


class TorchNormalise:
    """VecNormalize's bookkeeping with torch ops on the arrays ``step`` hands out, as a trainer would write it: float64 running
    mean / variance of vector_states and of the discounted returns over the rows that count, the normalised copies, no host
    read.  (It cannot see the rows a device-side reset restarted: their first observations never enter its statistics.)"""

    def __init__(self, env, gamma=0.99, clip_obs=10.0, clip_reward=10.0, eps=1e-8):
        import torch
        n, D = len(env), env.world.out["vector_states"].shape[1]
        f64 = dict(dtype=torch.float64, device="cuda")
        self.o = [torch.full((), 1e-4, **f64), torch.zeros(D, **f64), torch.ones(D, **f64)]
        self.r = [torch.full((), 1e-4, **f64), torch.zeros((), **f64), torch.ones((), **f64)]
        self.returns = torch.zeros(n, **f64)
        self.gamma, self.clip_obs, self.clip_reward, self.eps = gamma, clip_obs, clip_reward, eps

    @staticmethod
    def _update(s, x, w):
        c = w.sum()
        bm = (x * w).sum(0) / c.clamp(min=1)
        m2 = (((x - bm) ** 2) * w).sum(0)
        delta, tot = bm - s[1], s[0] + c
        s[1] = s[1] + delta * c / tot
        s[2] = (s[2] * s[0] + m2 + delta * delta * s[0] * c / tot) / tot
        s[0] = tot

    def push(self, state, rew, dones, info):
        import torch
        w = info["is_clean"].to(torch.float64)
        x = state.vector_states.to(torch.float64)
        self.returns = torch.where(w > 0, self.returns * self.gamma + rew, self.returns)
        self._update(self.o, x, w[:, None])
        self._update(self.r, self.returns, w)
        self.returns = torch.where(dones > 0, torch.zeros_like(self.returns), self.returns)
        obs = ((x - self.o[1]) / torch.sqrt(self.o[2] + self.eps)).clamp(-self.clip_obs, self.clip_obs).float()
        return obs, (rew / torch.sqrt(self.r[2] + self.eps)).clamp(-self.clip_reward, self.clip_reward)


def stack_depths(stack):
    """(image, state, laser) YAML keys -> effective depths (base.py:103-105)"""
    return (max(stack[0], 0), max(stack[1], 0), max(stack[2], 1) if stack[2] >= 0 else 0)


def measure(envs=1024, robots=4, peds=3, obstacles=2, steps=300, time_max=100, natives=(False, True, "device"), stack=None,
            torch_stack=False, episodes=None, wrappers=None, final_obs=False, normalise=None):
    """robot-steps/s of VecImageEnv over `steps` steps, after the envs have drifted out of phase.  ``stack`` = (image_batch,
    state_batch, laser_batch): with the library's frame stacks, or (``torch_stack``) the same kept by torch ops on top;
    ``episodes`` = "library" | "torch" | "log": with the per-robot episode statistics, kept by the library or by ``TorchEpisodes``,
    or the library's with the episode log (a ring of 65536 records) on top;
    ``wrappers`` = (kind, by): kind "table" | "clip", by "none" (pre-decoded actions, nothing enabled) | "library"
    (``wrappers=True`` fed the raw output) | "torch" (``TorchWrappers`` fed the raw output); ``final_obs``: with the final
    observations kept by the library (``VecImageEnv(final_obs=True)``: one more launch per reset chain); ``normalise`` =
    "library" | "torch": with the running normalisation of vector_states and rewards, kept by the library
    (``VecImageEnv(normalise={})``) or by ``TorchNormalise``"""
    import torch
    from img_env_amd import worldgen
    from img_env_amd.vec_env import VecImageEnv
    grid = worldgen.make_grid(200, 2)
    out = {}
    for native in natives:
        cfg = worldgen.make_yaml_cfg(robots, peds, grid, time_max=time_max, n_obstacles=obstacles, seed=5)
        if stack is not None:
            cfg.update(image_batch=stack[0], state_batch=stack[1], laser_batch=stack[2])
        if wrappers is not None:
            cfg.update(max_ped=10, wrapper=list(WRAPPER_LIST), discrete_action=wrappers[0] == "table", discrete_actions=TABLE28)
        env = VecImageEnv(cfg, env_num=envs, seed=5, native_spawn=bool(native), device_reset=native == "device",
                          stack=stack is not None and not torch_stack, episode_stats=episodes in ("library", "log"),
                          episode_log=(1 << 16) if episodes == "log" else 0,
                          wrappers=wrappers is not None and wrappers[1] == "library", final_obs=final_obs,
                          normalise=dict(obs=True, reward=True) if normalise == "library" else None)
        tn = TorchNormalise(env) if normalise == "torch" else None
        te = TorchEpisodes(env) if episodes == "torch" else None
        ts = TorchStack(env, stack_depths(stack)) if stack is not None and torch_stack else None
        n = len(env)
        g = torch.Generator(device="cuda").manual_seed(1)
        acts = torch.zeros(16, n, 3, device="cuda")
        acts[:, :, 0] = torch.rand(16, n, generator=g, device="cuda") * 0.6
        acts[:, :, 1] = torch.rand(16, n, generator=g, device="cuda") * 1.8 - 0.9
        tw = None
        if wrappers is not None:
            # the policy's raw output: indices, or (v, w) a third of which lie outside the clip range; "none" steps what they decode to
            from img_env_amd.envs import VelActionWrapper
            if wrappers[0] == "table":
                raw = torch.randint(0, len(TABLE28), (16, n), generator=g, device="cuda")
            else:
                raw = torch.stack([torch.rand(16, n, generator=g, device="cuda") * 0.9 - 0.15,
                                   torch.rand(16, n, generator=g, device="cuda") * 2.7 - 1.35], dim=2)
            if wrappers[1] == "none":
                vel = VelActionWrapper(None, cfg)
                acts = torch.stack([vel.action(raw[k]) for k in range(16)]).float().contiguous()
            else:
                acts = raw
                tw = TorchWrappers(env) if wrappers[1] == "torch" else None
        kept = None

        def step(a):
            nonlocal kept
            if tn is not None:
                res = env.step(a)
                kept = tn.push(res[0], res[1], res[2], res[3])
                return res
            if tw is None:
                return env.step(a)
            a = tw.action(a)
            res = env.step(a)
            kept = tw.after(a, res[3])
            return res
        t0 = time.perf_counter()
        env.reset()
        if ts:
            ts.reset()
        if te:
            te.reset()
        torch.cuda.synchronize()
        t_reset = time.perf_counter() - t0
        for s in range(time_max + 20):  # past the first wave of time limits: the envs drift out of phase as robots collide
            _, rew, _, info = step(acts[s % 16])
            if ts:
                ts.push(info["all_down"])
            if te:
                te.push(acts[s % 16], rew, info)
        torch.cuda.synchronize()
        placed0 = sum(env.world.autoreset_last()[::-1][0:1]) + len(env.world.autoreset_last()[0]) if native == "device" else 0
        resets, t0 = 0, time.perf_counter()
        for s in range(steps):
            _, rew, _, info = step(acts[s % 16])
            if ts:
                ts.push(info["all_down"])
            if te:
                te.push(acts[s % 16], rew, info)
            if info["reset_envs"] is not None:  # (device-side reset: nothing comes back to the host)
                resets += len(info["reset_envs"])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if native == "device":  # placements handed out meanwhile
            worlds, first = env.world.autoreset_last()
            resets = first + len(worlds) - placed0
        res = dict(robot_steps_per_s=n * steps / dt, us_per_step=1e6 * dt / steps, env_resets_per_step=resets / steps,
                   first_reset_ms=1e3 * t_reset)
        if episodes is not None:  # (after the clock has stopped: this synchronises)
            res["episodes_counted"] = (te.statistics() if te else env.episode_statistics())["episodes"]
            if episodes == "log":
                res["episodes_logged"] = env.episode_log()["n_written"]
        if native is True and stack is None and episodes is None:  # the same steps without the reset half: what NeverStopWrapper costs on top of the step
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
    if episodes is not None:
        extra["episodes_by"] = episodes
    if wrappers is not None:
        extra["wrappers"], extra["wrappers_by"] = wrappers
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


def compare_episodes(args, rounds=3):
    """no statistics / library / torch_episodes, alternating, `rounds` times, per reset variant"""
    natives = (True, "device")
    runs = []
    for rnd in range(rounds):
        for mode in ("none", "library", "torch_episodes"):
            r = measure(args.envs, args.robots, args.peds, args.obstacles, args.steps, args.time_max, natives,
                        episodes=None if mode == "none" else mode.split("_")[0])
            for variant in ("native_spawn", "device_reset"):
                runs.append(dict(round=rnd, mode=mode, variant=variant, us_per_step=r[variant]["us_per_step"],
                                 env_resets_per_step=r[variant]["env_resets_per_step"],
                                 episodes_counted=r[variant].get("episodes_counted")))
                print(json.dumps(runs[-1]), flush=True)
    summary = []
    for variant in ("native_spawn", "device_reset"):
        row = dict(variant=variant)
        for mode in ("none", "library", "torch_episodes"):
            v = [r["us_per_step"] for r in runs if r["variant"] == variant and r["mode"] == mode]
            row[mode] = dict(us_per_step_rounds=v, median=sorted(v)[len(v) // 2], spread=max(v) - min(v))
        row["added_us_library"] = row["library"]["median"] - row["none"]["median"]
        row["added_us_torch"] = row["torch_episodes"]["median"] - row["none"]["median"]
        summary.append(row)
    return dict(envs=args.envs, robots_per_env=args.robots, peds_per_env=args.peds, steps=args.steps, time_max=args.time_max,
                rounds=rounds, runs=runs, summary=summary)


def compare_episode_log(args, rounds=3):
    """no statistics / statistics / statistics + episode log, alternating, `rounds` times, per reset variant"""
    natives = (True, "device")
    modes = (("none", None), ("statistics", "library"), ("log", "log"))
    runs = []
    for rnd in range(rounds):
        for mode, episodes in modes:
            r = measure(args.envs, args.robots, args.peds, args.obstacles, args.steps, args.time_max, natives, episodes=episodes)
            for variant in ("native_spawn", "device_reset"):
                runs.append(dict(round=rnd, mode=mode, variant=variant, us_per_step=r[variant]["us_per_step"],
                                 env_resets_per_step=r[variant]["env_resets_per_step"],
                                 episodes_logged=r[variant].get("episodes_logged")))
                print(json.dumps(runs[-1]), flush=True)
    summary = []
    for variant in ("native_spawn", "device_reset"):
        row = dict(variant=variant)
        for mode, _ in modes:
            v = [r["us_per_step"] for r in runs if r["variant"] == variant and r["mode"] == mode]
            row[mode] = dict(us_per_step_rounds=v, median=sorted(v)[len(v) // 2], spread=max(v) - min(v))
        row["added_us_statistics"] = row["statistics"]["median"] - row["none"]["median"]
        row["added_us_log"] = row["log"]["median"] - row["statistics"]["median"]
        summary.append(row)
    return dict(envs=args.envs, robots_per_env=args.robots, peds_per_env=args.peds, steps=args.steps, time_max=args.time_max,
                rounds=rounds, runs=runs, summary=summary)


def compare_final_obs(args, rounds=3):
    """the final observations off / on, alternating, `rounds` times, per reset variant: the feature-off rounds are the baseline"""
    natives = (True, "device")
    runs = []
    for rnd in range(rounds):
        for mode in ("off", "on"):
            r = measure(args.envs, args.robots, args.peds, args.obstacles, args.steps, args.time_max, natives, final_obs=mode == "on")
            for variant in ("native_spawn", "device_reset"):
                runs.append(dict(round=rnd, mode=mode, variant=variant, us_per_step=r[variant]["us_per_step"],
                                 env_resets_per_step=r[variant]["env_resets_per_step"]))
                print(json.dumps(runs[-1]), flush=True)
    summary = []
    for variant in ("native_spawn", "device_reset"):
        row = dict(variant=variant)
        for mode in ("off", "on"):
            v = [r["us_per_step"] for r in runs if r["variant"] == variant and r["mode"] == mode]
            row[mode] = dict(us_per_step_rounds=v, median=sorted(v)[len(v) // 2], spread=max(v) - min(v))
        row["added_us"] = row["on"]["median"] - row["off"]["median"]
        summary.append(row)
    return dict(envs=args.envs, robots_per_env=args.robots, peds_per_env=args.peds, steps=args.steps, time_max=args.time_max,
                rounds=rounds, runs=runs, summary=summary)


def compare_normalise(args, rounds=3):
    """the running normalisation off / kept by the library / kept with torch ops, alternating, `rounds` times in one process, with
    the device-side reset: the feature-off rounds are the baseline"""
    runs = []
    for rnd in range(rounds):
        for mode in ("off", "library", "torch"):
            r = measure(args.envs, args.robots, args.peds, args.obstacles, args.steps, args.time_max, ("device",),
                        normalise=None if mode == "off" else mode)["device_reset"]
            runs.append(dict(round=rnd, mode=mode, variant="device_reset", us_per_step=r["us_per_step"], env_resets_per_step=r["env_resets_per_step"]))
            print(json.dumps(runs[-1]), flush=True)
    row = dict(variant="device_reset")
    for mode in ("off", "library", "torch"):
        v = [r["us_per_step"] for r in runs if r["mode"] == mode]
        row[mode] = dict(us_per_step_rounds=v, median=sorted(v)[len(v) // 2], spread=max(v) - min(v))
    row["added_us_library"] = row["library"]["median"] - row["off"]["median"]
    row["added_us_torch"] = row["torch"]["median"] - row["off"]["median"]
    return dict(envs=args.envs, robots_per_env=args.robots, peds_per_env=args.peds, steps=args.steps, time_max=args.time_max,
                rounds=rounds, runs=runs, summary=[row])


def compare_wrappers(args, rounds=3):
    """pre-decoded actions with nothing enabled / wrappers=True / torch ops, alternating, `rounds` times, for the table and the
    clip, per reset variant"""
    natives = (True, "device")
    runs = []
    for kind in ("table", "clip"):
        for rnd in range(rounds):
            for mode in ("none", "library", "torch"):
                r = measure(args.envs, args.robots, args.peds, args.obstacles, args.steps, args.time_max, natives, wrappers=(kind, mode))
                for variant in ("native_spawn", "device_reset"):
                    runs.append(dict(kind=kind, round=rnd, mode=mode, variant=variant, us_per_step=r[variant]["us_per_step"],
                                     env_resets_per_step=r[variant]["env_resets_per_step"]))
                    print(json.dumps(runs[-1]), flush=True)
    summary = []
    for kind in ("table", "clip"):
        for variant in ("native_spawn", "device_reset"):
            row = dict(kind=kind, variant=variant)
            for mode in ("none", "library", "torch"):
                v = [r["us_per_step"] for r in runs if r["kind"] == kind and r["variant"] == variant and r["mode"] == mode]
                row[mode] = dict(us_per_step_rounds=v, median=sorted(v)[len(v) // 2], spread=max(v) - min(v))
            row["added_us_library"] = row["library"]["median"] - row["none"]["median"]
            row["added_us_torch"] = row["torch"]["median"] - row["none"]["median"]
            summary.append(row)
    return dict(envs=args.envs, robots_per_env=args.robots, peds_per_env=args.peds, steps=args.steps, time_max=args.time_max,
                rounds=rounds, runs=runs, summary=summary)


POLICY_TABLE = [[v, w] for v in (0.0, 0.3, 0.6) for w in (-0.9, 0.0, 0.9)] + [[0.15, 0.0], [0.45, 0.0]]  # 11 actions


def measure_policy(variant, envs=1024, robots=4, peds=3, obstacles=2, steps=300, time_max=100, horizon=32):
    """us per step of ``VecImageEnv(..., wrappers=True, rollout=horizon)`` with the device-side reset, from logits over 11 discrete
    actions to the stepped env, with the sample, its log-probability and entropy and the [T, n] action / log-prob / value columns
    kept by the library ("library": ``policy=dict(seed=s)``, ``policy_step``) or by torch ("torch": ``torch.distributions.Categorical``
    -- sample, log_prob, entropy -- three ``buf[t].copy_`` and ``step`` on the sampled indices).  A new window every ``horizon`` steps."""
    import torch
    from img_env_amd import worldgen
    from img_env_amd.vec_env import VecImageEnv
    grid = worldgen.make_grid(200, 2)
    cfg = worldgen.make_yaml_cfg(robots, peds, grid, time_max=time_max, n_obstacles=obstacles, seed=5)
    cfg.update(discrete_action=True, discrete_actions=POLICY_TABLE)
    T, n, A = horizon, envs * robots, len(POLICY_TABLE)
    env = VecImageEnv(cfg, env_num=envs, seed=5, device_reset=True, wrappers=True, rollout=T, rollout_final=n,
                      policy=dict(seed=7) if variant == "library" else None)
    g = torch.Generator(device="cuda").manual_seed(1)
    logits = torch.randn(16, n, A, generator=g, device="cuda")
    values = torch.randn(16, n, generator=g, device="cuda")
    buf = None
    if variant == "torch":
        buf = dict(act=torch.zeros(T, n, device="cuda"), logp=torch.zeros(T, n, device="cuda"), value=torch.zeros(T + 1, n, device="cuda"))
    cursor, launches = [0], [0]

    def step(s):
        t = cursor[0]
        if t == T:
            env.rollout_begin()
            t = 0
        l, v = logits[s % 16], values[s % 16]
        if variant == "library":
            env.policy_step(logits=l, values=v)
        else:
            dist = torch.distributions.Categorical(logits=l)
            a = dist.sample()
            logp, ent = dist.log_prob(a), dist.entropy()  # noqa: F841 (the entropy is what the loss takes; computed, not stored)
            buf["act"][t].copy_(a)
            buf["logp"][t].copy_(logp)
            buf["value"][t].copy_(v)
            env.step(a)
        cursor[0] = t + 1
    env.reset()
    for s in range(time_max + 20):  # the drift phase: past the first wave of time limits
        step(s)
    launches[0] = env.world.launches()
    torch.cuda.synchronize()
    worlds, first = env.world.autoreset_last()
    placed0, t0 = first + len(worlds), time.perf_counter()
    for s in range(steps):
        step(s)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    worlds, first = env.world.autoreset_last()
    env.close()
    return dict(us_per_step=1e6 * dt / steps, env_resets_per_step=(first + len(worlds) - placed0) / steps, horizon=T, actions=A,
                step_launches=launches[0])


def compare_policy(args, rounds=3):
    """the policy head against torch.distributions on the same commit, alternating, `rounds` times in one process"""
    runs = []
    for rnd in range(rounds):
        for variant in ("library", "torch"):
            r = measure_policy(variant, args.envs, args.robots, args.peds, args.obstacles, args.steps, args.time_max, args.horizon)
            runs.append(dict(round=rnd, variant=variant, **r))
            print(json.dumps(runs[-1]), flush=True)
    summary = {}
    for variant in ("library", "torch"):
        v = [r["us_per_step"] for r in runs if r["variant"] == variant]
        summary[variant] = dict(us_per_step_rounds=v, median=sorted(v)[len(v) // 2], spread=max(v) - min(v),
                                step_launches=[r["step_launches"] for r in runs if r["variant"] == variant][0])
    summary["torch_minus_library_us"] = summary["torch"]["median"] - summary["library"]["median"]
    return dict(envs=args.envs, robots_per_env=args.robots, peds_per_env=args.peds, steps=args.steps, time_max=args.time_max,
                horizon=args.horizon, rounds=rounds, runs=runs, summary=summary)


def track_sets(n_sets, peds, records, dt, seed=3, box=(3.0, 22.0)):
    """n_sets recorded crowds of `peds` straight walks of `records` records each: [peds, records, 5] rows (x, y, yaw, vx, vy)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    sets = []
    for _ in range(n_sets):
        d = np.zeros((peds, records, 5))
        for j in range(peds):
            x0, y0 = rng.uniform(box[0], box[1], 2)
            vx, vy = rng.uniform(-0.3, 0.3, 2)
            q = np.arange(records)
            d[j, :, 0], d[j, :, 1], d[j, :, 2] = x0 + vx * dt * q, y0 + vy * dt * q, np.arctan2(vy, vx)
            d[j, 1:, 3], d[j, 1:, 4] = vx, vy
        sets.append(d)
    return sets


def measure_tracks(variant, envs=1024, robots=4, peds=10, records=50, obstacles=2, steps=300, time_max=100, n_sets=8):
    """us per step of a dataset-scene VecImageEnv that never stops.  variant "python_loop": what exists without a track bank --
    imgenv_step, a host read of all_down, the finished envs' placements drawn by the library's host sampler and their recorded
    tracks uploaded in explicit batches (imgenv_reset_worlds); "native_spawn" / "device_reset": the bank (imgenv_tracks_add),
    sets drawn with the placements"""
    import torch
    from img_env_amd import _cabi, spawn, worldgen
    from img_env_amd.vec_env import VecImageEnv
    grid = worldgen.make_grid(200, 2)
    cfg = worldgen.make_yaml_cfg(robots, peds, grid, scene="dataset", time_max=time_max, n_obstacles=obstacles, seed=5)
    sets = track_sets(n_sets, peds, records, float(cfg["control_hz"]))
    loop = variant == "python_loop"
    env = VecImageEnv(cfg, env_num=envs, seed=5, native_spawn=variant != "python_loop", device_reset=variant == "device_reset",
                      auto_reset=not loop, ped_tracks=None if loop else sets, tracks_policy="keep" if loop else "placement")
    n = len(env)
    g = torch.Generator(device="cuda").manual_seed(1)
    acts = torch.zeros(16, n, 3, device="cuda")
    acts[:, :, 0] = torch.rand(16, n, generator=g, device="cuda") * 0.6
    acts[:, :, 1] = torch.rand(16, n, generator=g, device="cuda") * 1.8 - 0.9
    state = dict(episodes=0, resets=0)
    spawn_cfg = spawn.make_spawn_cfg(cfg)

    def fresh(k_list):
        lays = []
        for _ in k_list:
            seed = env._spawn_seed + state["episodes"]
            state["episodes"] += 1
            lays.append(spawn.init_ped_dataset(spawn.native_spawn(cfg, seed, spawn_cfg), sets[_cabi.tracks_for_placement(seed, n_sets)]))
        return lays

    def step(a):
        if not loop:
            info = env.step(a)[3]
            if info["reset_envs"] is not None:
                state["resets"] += len(info["reset_envs"])
            return
        o = env.world.step(a)
        down = (o["dones"].view(envs, robots) > 0).all(dim=1)
        finished = torch.nonzero(down).flatten().tolist()  # the host read in front of every reset
        if finished:
            env.reset_envs(finished, fresh(finished))
            state["resets"] += len(finished)
    if loop:
        env.reset(fresh(range(envs)))
    else:
        env.reset()
    for s in range(time_max + 20):  # past the first wave of time limits
        step(acts[s % 16])
    torch.cuda.synchronize()
    placed0 = sum(env.world.autoreset_last()[::-1][0:1]) + len(env.world.autoreset_last()[0]) if variant == "device_reset" else 0
    state["resets"], t0 = 0, time.perf_counter()
    for s in range(steps):
        step(acts[s % 16])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if variant == "device_reset":
        worlds, first = env.world.autoreset_last()
        state["resets"] = first + len(worlds) - placed0
    env.close()
    return dict(us_per_step=1e6 * dt / steps, env_resets_per_step=state["resets"] / steps, bytes_per_world_reset=peds * records * 48)


def compare_tracks(args, rounds=3):
    """python_loop / native_spawn / device_reset over recorded crowds, alternating, `rounds` times"""
    variants = ("python_loop", "native_spawn", "device_reset")
    runs = []
    for rnd in range(rounds):
        for variant in variants:
            r = measure_tracks(variant, args.envs, args.robots, args.peds, args.records, args.obstacles, args.steps, args.time_max)
            runs.append(dict(round=rnd, variant=variant, **r))
            print(json.dumps(runs[-1]), flush=True)
    summary = {}
    for variant in variants:
        v = [r["us_per_step"] for r in runs if r["variant"] == variant]
        summary[variant] = dict(us_per_step_rounds=v, median=sorted(v)[len(v) // 2], spread=max(v) - min(v))
    return dict(envs=args.envs, robots_per_env=args.robots, peds_per_env=args.peds, records=args.records, steps=args.steps,
                time_max=args.time_max, rounds=rounds, runs=runs, summary=summary)


def measure_scenarios(variant, envs=1024, robots=4, peds=3, obstacles=2, steps=300, time_max=100, n_scenarios=500):
    """us per VecImageEnv.step of an RVO VecImageEnv that never stops, over a fixed list of recorded episodes ("python_loop",
    "scenarios") or over fresh placements ("sampler"; also what another checkout is asked for)"""
    import torch
    from img_env_amd import spawn, worldgen
    from img_env_amd.vec_env import VecImageEnv
    grid = worldgen.make_grid(200, 2)
    cfg = worldgen.make_yaml_cfg(robots, peds, grid, time_max=time_max, n_obstacles=obstacles, seed=5)
    loop, banked = variant == "python_loop", variant == "scenarios"
    bank = None
    if loop or banked:
        spawn_cfg = spawn.make_spawn_cfg(cfg)
        bank = [spawn.native_spawn(cfg, 1000 + k, spawn_cfg) for k in range(n_scenarios)]
    if banked:
        env = VecImageEnv(cfg, env_num=envs, seed=5, device_reset=True, scenarios=bank)
    elif loop:
        env = VecImageEnv(cfg, env_num=envs, seed=5, auto_reset=False)
    else:
        env = VecImageEnv(cfg, env_num=envs, seed=5, device_reset=True)
    n = len(env)
    g = torch.Generator(device="cuda").manual_seed(1)
    acts = torch.zeros(16, n, 3, device="cuda")
    acts[:, :, 0] = torch.rand(16, n, generator=g, device="cuda") * 0.6
    acts[:, :, 1] = torch.rand(16, n, generator=g, device="cuda") * 1.8 - 0.9
    state = dict(next=0, resets=0)

    def from_list(count):  # the queue: reset_index % len(reset_reqs)
        lays = [bank[(state["next"] + q) % n_scenarios] for q in range(count)]
        state["next"] += count
        return lays

    def step(a):
        if not loop:
            env.step(a)
            return
        o = env.world.step(a)
        down = (o["dones"].view(envs, robots) > 0).all(dim=1)
        finished = torch.nonzero(down).flatten().tolist()  # the host read in front of every reset
        if finished:
            env.reset_envs(finished, from_list(len(finished)))
            state["resets"] += len(finished)
    if loop:
        env.reset(from_list(envs))
    else:
        env.reset()
    for s in range(time_max + 20):  # the drift phase: past the first wave of time limits
        step(acts[s % 16])
    torch.cuda.synchronize()
    placed0 = 0
    if not loop:
        worlds, first = env.world.autoreset_last()
        placed0 = first + len(worlds)
    state["resets"], t0 = 0, time.perf_counter()
    for s in range(steps):
        step(acts[s % 16])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if not loop:
        worlds, first = env.world.autoreset_last()
        state["resets"] = first + len(worlds) - placed0
    env.close()
    return dict(us_per_step=1e6 * dt / steps, env_resets_per_step=state["resets"] / steps)


def compare_scenarios(args, rounds=3):
    """python_loop / scenarios / sampler (/ parent), alternating, `rounds` times; one process per measurement"""
    import subprocess
    variants = ["python_loop", "scenarios", "sampler"] + (["parent"] if args.parent_tree else [])
    base = [sys.executable, os.path.abspath(__file__), "--envs", str(args.envs), "--robots", str(args.robots), "--peds", str(args.peds),
            "--obstacles", str(args.obstacles), "--steps", str(args.steps), "--time-max", str(args.time_max), "--scenarios", str(args.scenarios)]
    runs = []
    for rnd in range(rounds):
        for variant in variants:
            cmd = base + ["--scenarios-variant", "sampler" if variant == "parent" else variant]
            if variant == "parent":
                cmd += ["--tree", args.parent_tree]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise RuntimeError("%s: exit %d\n%s" % (" ".join(cmd), out.returncode, out.stderr[-2000:]))
            runs.append(dict(round=rnd, variant=variant, **json.loads(out.stdout.strip().splitlines()[-1])))
            print(json.dumps(runs[-1]), flush=True)
    summary = {}
    for variant in variants:
        v = [r["us_per_step"] for r in runs if r["variant"] == variant]
        summary[variant] = dict(us_per_step_rounds=v, median=sorted(v)[len(v) // 2], spread=max(v) - min(v))
    return dict(envs=args.envs, robots_per_env=args.robots, peds_per_env=args.peds, scenarios=args.scenarios, steps=args.steps,
                time_max=args.time_max, rounds=rounds, runs=runs, summary=summary)


def torch_gae(r, values, final_values, gamma, lam, n, F):
    """imgenv_rollout_gae's rule as a torch loop over t (include/imgenv.h), on the ring's tensors"""
    import torch
    adv, ret = torch.zeros_like(r["rewards"]), torch.zeros_like(r["rewards"])
    gae, gl, zero = torch.zeros_like(values[0]), gamma * lam, torch.zeros_like(values[0])
    for t in range(n - 1, -1, -1):
        e = r["final_idx"][t + 1]
        done, has, clean = r["dones"][t] != 0, e >= 0, r["is_clean"][t] != 0
        terminal = done & (r["dones_info"][t] != 10)
        kept = torch.where(has & (e < F), final_values[e.clamp(0, F - 1).long()], zero)
        nv = torch.where(terminal, zero, torch.where(has, kept, values[t + 1]))
        delta = r["rewards"][t] + gamma * nv - values[t]
        gae = torch.where(clean, delta + torch.where(done | has, zero, gl * gae), zero)
        adv[t] = gae
        ret[t] = torch.where(clean, gae + values[t], zero)
    return adv, ret


def measure_rollout(variant, envs=1024, robots=4, peds=3, obstacles=2, steps=300, time_max=100, horizon=32):
    """us per VecImageEnv.step (device_reset=True) with the rollout kept by nobody ("none"), by the library ("library":
    ``rollout=horizon``, a new window every ``horizon`` steps) or by torch on top of "none" ("torch": ``buf[t].copy_(x)`` per field and
    scalar, the final rows and ``all_down`` taken whole from ``final_obs=True`` -- without a host read nobody outside the library
    knows which rows they are); "gae": the device's advantage pass against ``torch_gae`` over a rollout of 128 steps"""
    import torch
    from img_env_amd import worldgen
    from img_env_amd.vec_env import VecImageEnv
    grid = worldgen.make_grid(200, 2)
    cfg = worldgen.make_yaml_cfg(robots, peds, grid, time_max=time_max, n_obstacles=obstacles, seed=5)
    fields = ("sensor_maps", "vector_states", "lasers", "ped_vector_states", "ped_maps")
    gae = variant == "gae"
    T = 128 if gae else horizon
    n = envs * robots
    env = VecImageEnv(cfg, env_num=envs, seed=5, device_reset=True, final_obs=variant == "torch",
                      rollout=T if variant in ("library", "gae") else 0, rollout_final=4 * n if gae else n,
                      rollout_fields=["vector_states"] if gae else None)
    g = torch.Generator(device="cuda").manual_seed(1)
    acts = torch.zeros(16, n, 3, device="cuda")
    acts[:, :, 0] = torch.rand(16, n, generator=g, device="cuda") * 0.6
    acts[:, :, 1] = torch.rand(16, n, generator=g, device="cuda") * 1.8 - 0.9
    buf = None
    if variant == "torch":
        o, f = env.world.out, env.world.final_obs
        buf = {"obs_" + k: torch.zeros((T + 1,) + tuple(o[k].shape), dtype=o[k].dtype, device="cuda") for k in fields}
        buf.update({"final_" + k: torch.zeros((T,) + tuple(f[k].shape), dtype=f[k].dtype, device="cuda") for k in fields})
        buf.update(actions=torch.zeros(T, n, 3, device="cuda"), rewards=torch.zeros(T, n, device="cuda"),
                   dones=torch.zeros(T, n, dtype=torch.uint8, device="cuda"), is_clean=torch.zeros(T, n, dtype=torch.uint8, device="cuda"),
                   dones_info=torch.zeros(T, n, dtype=torch.int32, device="cuda"), all_down=torch.zeros(T, n, dtype=torch.bool, device="cuda"))
    cursor = [0]

    def step(a):
        t = cursor[0]
        if t == T:  # the next window starts from the last slot
            if variant == "library":
                env.rollout_begin()
            elif buf is not None:
                for k in fields:
                    buf["obs_" + k][0].copy_(buf["obs_" + k][T])
            t = 0
        _, rew, done, info = env.step(a)
        if buf is not None:
            o, f = env.world.out, env.world.final_obs
            for k in fields:
                buf["obs_" + k][t + 1].copy_(o[k])
                buf["final_" + k][t].copy_(f[k])
            buf["actions"][t].copy_(a)
            buf["rewards"][t].copy_(rew)
            buf["dones"][t].copy_(done)
            buf["is_clean"][t].copy_(info["is_clean"])
            buf["dones_info"][t].copy_(info["dones_info"])
            buf["all_down"][t].copy_(info["all_down"])
        cursor[0] = t + 1
    env.reset()
    if gae:
        for s in range(T):
            env.step(acts[s % 16])
        r = env.rollout()
        F = r["final_row"].shape[0]
        values, fv = torch.randn(T + 1, n, generator=g, device="cuda"), torch.randn(F, generator=g, device="cuda")
        res = {}
        for name, fn in (("device", lambda: env.rollout_advantages(values, fv, 0.99, 0.95)), ("torch", lambda: torch_gae(r, values, fv, 0.99, 0.95, T, F))):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                out = fn()
            torch.cuda.synchronize()
            res["us_per_pass_" + name] = 1e6 * (time.perf_counter() - t0) / 20
            res[name] = out
        res["max_abs_diff"] = float((res.pop("device")[0] - res.pop("torch")[0]).abs().max())  # (the torch loop's order of operations is its own)
        env.close()
        return dict(horizon=T, rows=n, **res)
    for s in range(time_max + 20):  # the drift phase: past the first wave of time limits
        step(acts[s % 16])
    torch.cuda.synchronize()
    worlds, first = env.world.autoreset_last()
    placed0, t0 = first + len(worlds), time.perf_counter()
    for s in range(steps):
        step(acts[s % 16])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    worlds, first = env.world.autoreset_last()
    env.close()
    return dict(us_per_step=1e6 * dt / steps, env_resets_per_step=(first + len(worlds) - placed0) / steps, horizon=T)


def compare_rollout(args, rounds=3):
    """none / library / torch, alternating, `rounds` times, then the advantage pass once; one process per measurement"""
    import subprocess
    base = [sys.executable, os.path.abspath(__file__), "--envs", str(args.envs), "--robots", str(args.robots), "--peds", str(args.peds),
            "--obstacles", str(args.obstacles), "--steps", str(args.steps), "--time-max", str(args.time_max), "--horizon", str(args.horizon)]

    def one(variant):
        out = subprocess.run(base + ["--rollout-variant", variant], capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            raise RuntimeError("%s: exit %d\n%s" % (variant, out.returncode, out.stderr[-2000:]))
        return json.loads(out.stdout.strip().splitlines()[-1])
    variants, runs = ("none", "library", "torch"), []
    for rnd in range(rounds):
        for variant in variants:
            runs.append(dict(round=rnd, variant=variant, **one(variant)))
            print(json.dumps(runs[-1]), flush=True)
    summary = {}
    for variant in variants:
        v = [r["us_per_step"] for r in runs if r["variant"] == variant]
        summary[variant] = dict(us_per_step_rounds=v, median=sorted(v)[len(v) // 2], spread=max(v) - min(v))
    summary["added_us_library"] = summary["library"]["median"] - summary["none"]["median"]
    summary["added_us_torch"] = summary["torch"]["median"] - summary["none"]["median"]
    summary["gae"] = one("gae")
    print(json.dumps(summary["gae"]), flush=True)
    return dict(envs=args.envs, robots_per_env=args.robots, peds_per_env=args.peds, steps=args.steps, time_max=args.time_max,
                horizon=args.horizon, rounds=rounds, runs=runs, summary=summary)


def measure_minibatch(variant, envs=1024, robots=4, peds=3, obstacles=2, time_max=100, horizon=32, batch=4096, epochs=5):
    """us per PPO epoch's worth of minibatches over a full window of ``horizon`` device_reset steps, all five single-frame fields, four
    caller scalars (adv, ret, values, old log-probabilities), the advantages normalised over the transitions that count:
    "library": ``VecImageEnv.rollout_minibatches`` (index + statistics + shuffle + one gather per minibatch, no host read);
    "torch": the same tensors from torch ops on the library's ring -- ``nonzero`` on ``is_clean`` (a host synchronisation), masked
    mean / std, ``randperm``, one ``index_select`` per field and scalar and minibatch"""
    import torch
    from img_env_amd import worldgen
    from img_env_amd.vec_env import VecImageEnv
    grid = worldgen.make_grid(200, 2)
    cfg = worldgen.make_yaml_cfg(robots, peds, grid, time_max=time_max, n_obstacles=obstacles, seed=5)
    T, n, B = horizon, envs * robots, batch
    env = VecImageEnv(cfg, env_num=envs, seed=5, device_reset=True, rollout=T, rollout_final=n, minibatch=B if variant == "library" else 0,
                      minibatch_buffers=2)
    g = torch.Generator(device="cuda").manual_seed(1)
    acts = torch.zeros(16, n, 3, device="cuda")
    acts[:, :, 0] = torch.rand(16, n, generator=g, device="cuda") * 0.6
    acts[:, :, 1] = torch.rand(16, n, generator=g, device="cuda") * 1.8 - 0.9
    env.reset()
    windows = max(1, -(-(time_max + 20) // T))  # past the first wave of time limits, ending on a full window
    for s in range(windows * T):
        if s and s % T == 0:
            env.rollout_begin()
        env.step(acts[s % 16])
    values = torch.randn(T + 1, n, generator=g, device="cuda")
    adv, ret = env.rollout_advantages(values, None, 0.99, 0.95)
    logp = torch.randn(T, n, generator=g, device="cuda")
    r = env.rollout()
    fields = [k[4:] for k in r if k.startswith("obs_")]

    def library(seed):
        count = 0
        for mb in env.rollout_minibatches({"adv": adv, "ret": ret, "values": values, "logp": logp}, seed, normalise="adv"):
            count += 1
        return count

    def torch_epoch(seed):
        clean = r["is_clean"][:T].reshape(-1)
        valid = torch.nonzero(clean).flatten()  # (the host waits here: the size of the result)
        a = adv.reshape(-1)[valid]
        mean, inv = a.mean(), torch.rsqrt(a.var(unbiased=False) + 1e-8)
        order = valid[torch.randperm(valid.numel(), device="cuda", generator=g)]
        flat = {k: r["obs_" + k].flatten(0, 1) for k in fields}
        ring = {k: r[k].flatten(0, 1) for k in ("actions", "rewards", "dones", "dones_info")}
        mine = {"adv": adv.reshape(-1), "ret": ret.reshape(-1), "values": values.reshape(-1), "logp": logp.reshape(-1)}
        count = 0
        for j in range(-(-valid.numel() // B)):
            idx = order[j * B:(j + 1) * B]
            mb = {k: v.index_select(0, idx) for k, v in flat.items()}
            mb.update({k: v.index_select(0, idx) for k, v in ring.items()})
            mb.update({k: v.index_select(0, idx) for k, v in mine.items()})
            mb["adv"] = (mb["adv"] - mean) * inv
            count += 1
        return count
    fn = library if variant == "library" else torch_epoch
    fn(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for e in range(epochs):
        count = fn(e + 1)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    valid_n = int((r["is_clean"][:T] != 0).sum().item())
    row_bytes = sum(r["obs_" + k][0, 0].numel() * r["obs_" + k].element_size() for k in fields)
    env.close()
    return dict(us_per_epoch=1e6 * dt / epochs, minibatches=count, batch=B, horizon=T, rows=n, transitions=T * n, valid=valid_n,
                row_bytes=row_bytes, fields=fields)


def compare_minibatch(args, rounds=3):
    """library / torch, alternating, `rounds` times; one process per measurement"""
    import subprocess
    base = [sys.executable, os.path.abspath(__file__), "--envs", str(args.envs), "--robots", str(args.robots), "--peds", str(args.peds),
            "--obstacles", str(args.obstacles), "--time-max", str(args.time_max), "--horizon", str(args.horizon), "--batch", str(args.batch)]
    variants, runs = ("library", "torch"), []
    for rnd in range(rounds):
        for variant in variants:
            out = subprocess.run(base + ["--minibatch-variant", variant], capture_output=True, text=True, timeout=900)
            if out.returncode != 0:
                raise RuntimeError("%s: exit %d\n%s" % (variant, out.returncode, out.stderr[-2000:]))
            runs.append(dict(round=rnd, variant=variant, **json.loads(out.stdout.strip().splitlines()[-1])))
            print(json.dumps(runs[-1]), flush=True)
    summary = {}
    for variant in variants:
        v = [x["us_per_epoch"] for x in runs if x["variant"] == variant]
        summary[variant] = dict(us_per_epoch_rounds=v, median=sorted(v)[len(v) // 2], spread=max(v) - min(v))
    summary["torch_minus_library_us"] = summary["torch"]["median"] - summary["library"]["median"]
    return dict(envs=args.envs, robots_per_env=args.robots, peds_per_env=args.peds, time_max=args.time_max, horizon=args.horizon,
                batch=args.batch, rounds=rounds, runs=runs, summary=summary)


def measure_sequences(variant, envs=1024, robots=4, peds=3, obstacles=2, time_max=100, horizon=32, length=16, batch=256, epochs=5):
    """us per epoch's worth of SEQUENCE minibatches (``length`` steps x ``batch`` sequences, time-major) over a full window of
    ``horizon`` device_reset steps, all five single-frame fields, four caller scalars and two 512-byte state arrays:
    "library": ``VecImageEnv.rollout_sequences`` (index + shuffle + one gather per minibatch, no host read);
    "torch": the same time-major tensors from torch ops on the library's ring -- chunk flags by ``reshape`` / ``any``, ``nonzero`` (a
    host synchronisation), ``randperm``, one ``index_select`` per field and scalar and minibatch"""
    import torch
    from img_env_amd import worldgen
    from img_env_amd.vec_env import VecImageEnv
    grid = worldgen.make_grid(200, 2)
    cfg = worldgen.make_yaml_cfg(robots, peds, grid, time_max=time_max, n_obstacles=obstacles, seed=5)
    T, n, L, Bs = horizon, envs * robots, length, batch
    if T % L:
        raise ValueError("--horizon must be a multiple of --seq-length here (the torch route reshapes the window)")
    env = VecImageEnv(cfg, env_num=envs, seed=5, device_reset=True, rollout=T, rollout_final=n,
                      sequences=dict(length=L, batch=Bs, buffers=2, state_bytes=(512, 512)) if variant == "library" else None)
    g = torch.Generator(device="cuda").manual_seed(1)
    acts = torch.zeros(16, n, 3, device="cuda")
    acts[:, :, 0] = torch.rand(16, n, generator=g, device="cuda") * 0.6
    acts[:, :, 1] = torch.rand(16, n, generator=g, device="cuda") * 1.8 - 0.9
    env.reset()
    windows = max(1, -(-(time_max + 20) // T))  # past the first wave of time limits, ending on a full window
    for s in range(windows * T):
        if s and s % T == 0:
            env.rollout_begin()
        env.step(acts[s % 16])
    values = torch.randn(T + 1, n, generator=g, device="cuda")
    adv, ret = env.rollout_advantages(values, None, 0.99, 0.95)
    logp = torch.randn(T, n, generator=g, device="cuda")
    states = [torch.randn(T + 1, n, 128, generator=g, device="cuda") for _ in range(2)]
    r = env.rollout()
    fields = [k[4:] for k in r if k.startswith("obs_")]
    C = T // L
    steps = torch.arange(L, device="cuda")

    def library(seed):
        count = 0
        for mb in env.rollout_sequences({"adv": adv, "ret": ret, "values": values, "logp": logp}, seed, states=states):
            count += 1
        return count

    def torch_epoch(seed):
        flags = (r["is_clean"][:T].reshape(C, L, n) != 0).any(dim=1).reshape(-1)
        valid = torch.nonzero(flags).flatten()  # (the host waits here: the size of the result)
        order = valid[torch.randperm(valid.numel(), device="cuda", generator=g)]
        flat = {k: r["obs_" + k].flatten(0, 1) for k in fields}
        ring = {k: r[k].flatten(0, 1) for k in ("actions", "rewards", "dones", "dones_info", "is_clean")}
        mine = {"adv": adv.reshape(-1), "ret": ret.reshape(-1), "values": values.reshape(-1), "logp": logp.reshape(-1)}
        first = r["final_idx"].reshape(-1)
        count = 0
        for j in range(-(-C * n // Bs)):
            q = order[j * Bs:(j + 1) * Bs]
            k0 = (q // n) * (L * n) + q % n
            idx = (k0[None, :] + steps[:, None] * n).reshape(-1)  # time-major [L, Bs]
            mb = {k: v.index_select(0, idx) for k, v in flat.items()}
            mb.update({k: v.index_select(0, idx) for k, v in ring.items()})
            mb.update({k: v.index_select(0, idx) for k, v in mine.items()})
            mb["mb_first"] = first.index_select(0, idx) >= 0
            mb["state0"], mb["state1"] = (s.flatten(0, 1).index_select(0, k0) for s in states)
            count += 1
        return count
    fn = library if variant == "library" else torch_epoch
    fn(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for e in range(epochs):
        count = fn(e + 1)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    flags = (r["is_clean"][:T].reshape(C, L, n) != 0).any(dim=1)
    row_bytes = sum(r["obs_" + k][0, 0].numel() * r["obs_" + k].element_size() for k in fields)
    env.close()
    return dict(us_per_epoch=1e6 * dt / epochs, minibatches=count, length=L, batch=Bs, horizon=T, rows=n, sequences=C * n, valid=int(flags.sum().item()),
                row_bytes=row_bytes, fields=fields)


def compare_sequences(args, rounds=3):
    """library / torch, alternating, `rounds` times; one process per measurement, each under its own time limit"""
    import subprocess
    base = [sys.executable, os.path.abspath(__file__), "--envs", str(args.envs), "--robots", str(args.robots), "--peds", str(args.peds),
            "--obstacles", str(args.obstacles), "--time-max", str(args.time_max), "--horizon", str(args.horizon), "--seq-length", str(args.seq_length),
            "--seq-batch", str(args.seq_batch)]
    variants, runs = ("library", "torch"), []
    for rnd in range(rounds):
        for variant in variants:
            out = subprocess.run(base + ["--sequences-variant", variant], capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                raise RuntimeError("%s: exit %d\n%s" % (variant, out.returncode, out.stderr[-2000:]))
            runs.append(dict(round=rnd, variant=variant, **json.loads(out.stdout.strip().splitlines()[-1])))
            print(json.dumps(runs[-1]), flush=True)
    summary = {}
    for variant in variants:
        v = [x["us_per_epoch"] for x in runs if x["variant"] == variant]
        summary[variant] = dict(us_per_epoch_rounds=v, median=sorted(v)[len(v) // 2], spread=max(v) - min(v))
    summary["torch_minus_library_us"] = summary["torch"]["median"] - summary["library"]["median"]
    lib = [x for x in runs if x["variant"] == "library"][0]
    # the gathers' algorithmic bytes (read + written) per second of the library's whole epoch -- index and shuffle included
    per_step = lib["row_bytes"] + 12 + 4 + 1 + 4 + 1 + 4 + 4 * 4
    moved = 2 * lib["minibatches"] * (lib["length"] * lib["batch"] * per_step + lib["batch"] * 1024)
    summary["library_gather_bytes_per_epoch"] = moved
    summary["library_tb_per_s"] = moved / (summary["library"]["median"] * 1e-6) / 1e12
    return dict(envs=args.envs, robots_per_env=args.robots, peds_per_env=args.peds, time_max=args.time_max, horizon=args.horizon,
                length=args.seq_length, batch=args.seq_batch, rounds=rounds, runs=runs, summary=summary)


def measure_ped_draw(variant, envs=1024, robots=4, peds=3, obstacles=2, steps=300, time_max=100, horizon=32, batch=4096):
    """One process of --ped-draw-compare: device_reset steps with ``rollout=horizon`` and the default fields, ``ped_maps`` stored
    ("stored"; also what "parent" runs, from another checkout) or drawn at gather time ("drawn": ``rollout_draw_ped_maps=True``).
    (a) us per step, windows restarted every ``horizon`` steps; (b) us per minibatch of ``batch`` transitions, device time between
    two events around 20 gathers (the drawn variant: gather + k_ped_draw), of every field on this handle and of the maps alone on
    a second one made afterwards (a handle's minibatch fields are chosen once); (c) "drawn": k_ped_draw alone over ``batch`` rows
    of the ring, against the bytes it writes and a copy of as many; the ring's bytes"""
    import torch
    from img_env_amd import worldgen
    from img_env_amd.vec_env import VecImageEnv
    grid = worldgen.make_grid(200, 2)
    cfg = worldgen.make_yaml_cfg(robots, peds, grid, time_max=time_max, n_obstacles=obstacles, seed=5)
    T, n, B = horizon, envs * robots, batch
    extra = dict(rollout_draw_ped_maps=True) if variant == "drawn" else {}
    env = VecImageEnv(cfg, env_num=envs, seed=5, device_reset=True, rollout=T, rollout_final=n, **extra)
    w = env.world
    g = torch.Generator(device="cuda").manual_seed(1)
    acts = torch.zeros(16, n, 3, device="cuda")
    acts[:, :, 0] = torch.rand(16, n, generator=g, device="cuda") * 0.6
    acts[:, :, 1] = torch.rand(16, n, generator=g, device="cuda") * 1.8 - 0.9
    cursor = [0]

    def step(a):
        if cursor[0] == T:
            env.rollout_begin()
            cursor[0] = 0
        env.step(a)
        cursor[0] += 1
    env.reset()
    for s in range(time_max + 20):  # the drift phase: past the first wave of time limits
        step(acts[s % 16])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(steps):
        step(acts[s % 16])
    torch.cuda.synchronize()
    res = dict(us_per_step=1e6 * (time.perf_counter() - t0) / steps, horizon=T, rows=n, batch=B,
               ring_bytes=sum(t.numel() * t.element_size() for t in w.rollout.values()))
    while cursor[0] < T:  # a full window for the minibatches
        step(acts[cursor[0] % 16])

    def device_us(fn, reps=20):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(reps):
            fn(k)
        b.record()
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(b) / reps
    maps = "ped_maps_drawn" if variant == "drawn" else "ped_maps"
    w.enable_minibatch(B, 2, None)
    w.rollout_index()
    w.rollout_shuffle(7)
    count = -(-T * n // B)
    res["us_per_minibatch_all_fields"] = device_us(lambda k=0: w.rollout_minibatch(k % count, k % 2))
    res["valid"] = w.rollout_valid_count()
    res["maps_field"] = maps
    if variant == "drawn":
        ring = w.rollout["obs_ped_vector_states"].view(-1, w.rollout["obs_ped_vector_states"].shape[-1])
        out = torch.empty((B,) + tuple(w.minibatch["mb_ped_maps"].shape[2:]), device="cuda")
        rows = w.minibatch["order"][:B].clamp(min=0).contiguous()
        res["us_ped_draw_alone_shuffled_rows"] = device_us(lambda k=0: w.draw_ped_maps(ring, rows, out))
        res["us_ped_draw_alone_first_rows"] = device_us(lambda k=0: w.draw_ped_maps(ring[:B], None, out))
        res["ped_draw_bytes_written"] = out.numel() * 4
        src, dst = torch.empty_like(out), torch.empty_like(out)
        res["us_copy_same_bytes"] = device_us(lambda k=0: dst.copy_(src))  # (a device-to-device copy: reads and writes that many bytes)
        res["maps_not_zero"] = int((out.view(B, -1) != 0).any(dim=1).sum().item())
    env.close()
    # the maps alone: a second handle, one full window, the minibatch of that one field
    env = VecImageEnv(cfg, env_num=envs, seed=5, device_reset=True, rollout=T, rollout_final=n, **extra)
    w = env.world
    env.reset()
    for s in range(T):
        env.step(acts[s % 16])
    w.enable_minibatch(B, 2, [maps])
    w.rollout_index()
    w.rollout_shuffle(7)
    res["us_per_minibatch_maps_alone"] = device_us(lambda k=0: w.rollout_minibatch(k % count, k % 2))
    env.close()
    return res


def compare_ped_draw(args, rounds=3):
    """stored / drawn (/ parent: the stored path from --parent-tree, a built checkout of the parent commit), alternating, `rounds`
    times; one process per measurement"""
    import subprocess
    base = [sys.executable, os.path.abspath(__file__), "--envs", str(args.envs), "--robots", str(args.robots), "--peds", str(args.peds),
            "--obstacles", str(args.obstacles), "--steps", str(args.steps), "--time-max", str(args.time_max), "--horizon", str(args.horizon),
            "--batch", str(args.batch)]
    variants, runs = ["stored", "drawn"] + (["parent"] if args.parent_tree else []), []
    for rnd in range(rounds):
        for variant in variants:
            cmd = base + ["--ped-draw-variant", "stored" if variant == "parent" else variant]
            if variant == "parent":
                cmd += ["--tree", args.parent_tree]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if out.returncode != 0:
                raise RuntimeError("%s: exit %d\n%s" % (variant, out.returncode, out.stderr[-2000:]))
            runs.append(dict(round=rnd, variant=variant, **json.loads(out.stdout.strip().splitlines()[-1])))
            print(json.dumps(runs[-1]), flush=True)
    summary = {}
    for variant in variants:
        mine = [x for x in runs if x["variant"] == variant]
        summary[variant] = {}
        for key in ("us_per_step", "us_per_minibatch_all_fields", "us_per_minibatch_maps_alone", "us_ped_draw_alone_shuffled_rows", "us_ped_draw_alone_first_rows", "us_copy_same_bytes"):
            v = [x[key] for x in mine if key in x]
            if v:
                summary[variant][key] = dict(rounds=v, median=sorted(v)[len(v) // 2], spread=max(v) - min(v))
        summary[variant]["ring_bytes"] = mine[0]["ring_bytes"]
    summary["step_saving_us"] = summary["stored"]["us_per_step"]["median"] - summary["drawn"]["us_per_step"]["median"]
    summary["minibatch_drawn_minus_stored_us"] = (summary["drawn"]["us_per_minibatch_all_fields"]["median"] -
                                                  summary["stored"]["us_per_minibatch_all_fields"]["median"])
    summary["minibatch_maps_alone_drawn_minus_stored_us"] = (summary["drawn"]["us_per_minibatch_maps_alone"]["median"] -
                                                             summary["stored"]["us_per_minibatch_maps_alone"]["median"])
    return dict(envs=args.envs, robots_per_env=args.robots, peds_per_env=args.peds, steps=args.steps, time_max=args.time_max,
                horizon=args.horizon, batch=args.batch, rounds=rounds, runs=runs, summary=summary)


def compare_loss(args, rounds=3, window=0.6):
    """PPO's loss of one minibatch, from logits and values on the device to the gradients on them: ``VecImageEnv.policy_loss`` and
    ``backward()`` ("library": three launches and the autograd hand-over; "library_raw": ``World.policy_loss`` alone, whose
    outputs are the gradients) / the same loss in torch ops and autograd ("torch"), on the same commit, alternating, `rounds`
    times in one process.  The minibatch is a real one: a window of ``--horizon`` policy steps over 11 actions, advantages from the
    library, ``--batch`` rows, the clipped value loss and an entropy bonus.  us per loss; every measurement runs as many losses
    back to back as fill `window` seconds (counted from a short calibration run of the variant), then synchronises once: the
    figure is the cost of a loss in a stream of losses, the host's enqueue included, not a single call's latency."""
    import numpy as np
    import torch
    from img_env_amd import worldgen
    from img_env_amd.vec_env import VecImageEnv
    grid = worldgen.make_grid(200, 2)
    A, T, n, B = 11, args.horizon, args.envs * args.robots, args.batch
    table = [[0.06 * k, 0.18 * (k - 5)] for k in range(A)]
    cfg = worldgen.make_yaml_cfg(args.robots, args.peds, grid, time_max=args.time_max, n_obstacles=args.obstacles, seed=5, discrete_action=True,
                                 discrete_actions=table)
    env = VecImageEnv(cfg, env_num=args.envs, seed=5, device_reset=True, wrappers=True, rollout=T, rollout_final=n, minibatch=B,
                      policy=dict(seed=7, loss=True))
    g = torch.Generator(device="cuda").manual_seed(1)
    env.reset()
    for s in range(T):
        env.policy_step(logits=torch.randn(n, A, generator=g, device="cuda"), values=torch.randn(n, generator=g, device="cuda"))
    env.policy_value(torch.randn(n, generator=g, device="cuda"))
    ro = env.rollout()
    adv, ret = env.rollout_advantages(ro["pol_value"], None, 0.99, 0.95)
    scalars = dict(action=ro["pol_raw"][0], old_logp=ro["pol_logp"], old_value=ro["pol_value"], adv=adv, ret=ret)
    mb = next(iter(env.rollout_minibatches(scalars, 3, normalise="adv")))
    logits = (torch.randn(B, A, generator=g, device="cuda") * 0.5).requires_grad_()
    values = (mb["old_value"] + 0.3 * torch.randn(B, generator=g, device="cuda")).requires_grad_()
    clip, clip_vf, vf, ent = 0.2, 0.2, 0.5, 0.01
    act = mb["action"].to(torch.int64)

    def library():
        logits.grad = values.grad = None
        loss, _ = env.policy_loss(mb, logits=logits, values=values, clip=clip, vf_coef=vf, ent_coef=ent, clip_vf=clip_vf)
        loss.backward()

    def library_raw():
        env.world.policy_loss(logits.detach(), values.detach(), mb["action"], mb["old_logp"], mb["adv"], mb["ret"], mb["mb_weight"],
                              old_value=mb["old_value"], clip=clip, clip_vf=clip_vf, vf_coef=vf, ent_coef=ent)

    def torch_ops():
        logits.grad = values.grad = None
        w = mb["mb_weight"]
        ls = torch.log_softmax(logits, 1)
        logp = ls.gather(1, act[:, None])[:, 0]
        H = -(ls.exp() * ls).sum(1)
        r = (logp - mb["old_logp"]).exp()
        pg = -torch.min(r * mb["adv"], r.clamp(1 - clip, 1 + clip) * mb["adv"])
        vc = mb["old_value"] + (values - mb["old_value"]).clamp(-clip_vf, clip_vf)
        vl = 0.5 * torch.max((values - mb["ret"]) ** 2, (vc - mb["ret"]) ** 2)
        W = w.sum().clamp(min=1)
        loss = (w * (pg + vf * vl - ent * H)).sum() / W
        loss.backward()
    fns = dict(library=library, library_raw=library_raw, torch=torch_ops)
    # the two agree before they are timed
    library()
    got = (logits.grad.clone(), values.grad.clone())
    torch_ops()
    agree = dict(d_logits=float((got[0] - logits.grad).abs().max().item()), d_values=float((got[1] - values.grad).abs().max().item()),
                 weight_sum=float(mb["mb_weight"].sum().item()))
    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    iters = {}
    for variant, fn in fns.items():  # warm up, then size the window
        timed(fn, 50)
        iters[variant] = max(300, int(window * 200 / timed(fn, 200)))
    runs = []
    for rnd in range(rounds):
        for variant, fn in fns.items():
            timed(fn, 20)
            dt = timed(fn, iters[variant])
            runs.append(dict(round=rnd, variant=variant, us_per_loss=1e6 * dt / iters[variant], losses=iters[variant], seconds=dt))
            print(json.dumps(runs[-1]), flush=True)
    env.close()
    summary = {}
    for variant in fns:
        v = [x["us_per_loss"] for x in runs if x["variant"] == variant]
        summary[variant] = dict(us_per_loss_rounds=v, median=float(np.median(v)), spread=max(v) - min(v))
    summary["torch_minus_library_us"] = summary["torch"]["median"] - summary["library"]["median"]
    summary["sum_of_spreads_us"] = summary["torch"]["spread"] + summary["library"]["spread"]
    summary["agreement"] = agree
    return dict(envs=args.envs, robots_per_env=args.robots, actions=A, horizon=T, batch=B, window_s=window, losses=iters, rounds=rounds, runs=runs, summary=summary)


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
    ap.add_argument("--episodes", action="store_true", help="per-robot episode statistics kept by the library")
    ap.add_argument("--torch-episodes", action="store_true", help="the same statistics kept with EpisodeStats and torch ops")
    ap.add_argument("--episodes-compare", action="store_true",
                    help="no statistics / library / torch_episodes, alternating over --rounds rounds")
    ap.add_argument("--episode-log", action="store_true", help="the statistics and the per-episode log kept by the library")
    ap.add_argument("--episode-log-compare", action="store_true",
                    help="no statistics / statistics / statistics + episode log, alternating over --rounds rounds")
    ap.add_argument("--final-obs-compare", action="store_true",
                    help="the final observations (VecImageEnv(final_obs=True)) off / on, alternating over --rounds rounds")
    ap.add_argument("--wrappers", default=None, choices=("table", "clip"), help="the policy's raw output decoded by the library (wrappers=True)")
    ap.add_argument("--torch-wrappers", action="store_true", help="with --wrappers: the same kept with torch ops on a plain VecImageEnv")
    ap.add_argument("--policy-compare", action="store_true",
                    help="logits -> sampled action -> step: the policy head (policy_step) / torch.distributions, alternating over --rounds rounds")
    ap.add_argument("--wrappers-compare", action="store_true",
                    help="pre-decoded actions / library / torch, alternating over --rounds rounds, table and clip")
    ap.add_argument("--normalise-compare", action="store_true",
                    help="running normalisation off / library / torch ops, alternating over --rounds rounds, device-side reset")
    ap.add_argument("--tracks-compare", action="store_true",
                    help="dataset scene: explicit track batches from a Python loop / native_spawn with a track bank / device_reset with "
                         "it, alternating over --rounds rounds (use --peds 10)")
    ap.add_argument("--records", type=int, default=50, help="--tracks-compare: records per recorded pedestrian")
    ap.add_argument("--scenarios-compare", action="store_true",
                    help="a fixed list of recorded episodes: a Python loop with reset_worlds / device_reset with the scenario bank / "
                         "device_reset with the sampler (/ the sampler of --parent-tree), alternating over --rounds rounds")
    ap.add_argument("--scenarios", type=int, default=500, help="--scenarios-compare: recorded episodes in the list")
    ap.add_argument("--scenarios-variant", default=None, choices=("python_loop", "scenarios", "sampler"), help="one measurement of --scenarios-compare")
    ap.add_argument("--parent-tree", default=None, help="--scenarios-compare: a built checkout of another commit, measured as variant \"parent\"")
    ap.add_argument("--rollout-compare", action="store_true",
                    help="device_reset steps with no rollout storage / the library's (rollout=T) / the same arrays kept by torch copies, "
                         "alternating over --rounds rounds, and the advantage pass against a torch loop; one process per measurement")
    ap.add_argument("--rollout-variant", default=None, choices=("none", "library", "torch", "gae"), help="one measurement of --rollout-compare")
    ap.add_argument("--horizon", type=int, default=32, help="--rollout-compare: transitions per window")
    ap.add_argument("--minibatch-compare", action="store_true",
                    help="one PPO epoch of minibatches over a full window: the library's (VecImageEnv(minibatch=B)) / the same tensors "
                         "from torch ops, alternating over --rounds rounds; one process per measurement")
    ap.add_argument("--minibatch-variant", default=None, choices=("library", "torch"), help="one measurement of --minibatch-compare")
    ap.add_argument("--batch", type=int, default=4096, help="--minibatch-compare: transitions per minibatch")
    ap.add_argument("--sequences-compare", action="store_true",
                    help="one epoch of sequence minibatches over a full window: the library against torch ops on its ring, alternating rounds")
    ap.add_argument("--sequences-variant", default=None, choices=("library", "torch"), help="one measurement of --sequences-compare")
    ap.add_argument("--seq-length", type=int, default=16, help="--sequences-compare: steps per sequence")
    ap.add_argument("--seq-batch", type=int, default=256, help="--sequences-compare: sequences per minibatch")
    ap.add_argument("--ped-draw-compare", action="store_true",
                    help="rollout=--horizon with ped_maps stored / drawn at gather time (/ the parent's, --parent-tree): us per step, per minibatch, k_ped_draw alone")
    ap.add_argument("--ped-draw-variant", default=None, choices=("stored", "drawn"), help="one measurement of --ped-draw-compare")
    ap.add_argument("--loss-compare", action="store_true",
                    help="PPO's loss of a minibatch and its gradients: policy_loss / torch ops and autograd, alternating over --rounds rounds in one process")
    ap.add_argument("--tree", default=None, help="import img_env_amd from this checkout instead of the tool's own")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="--stack-compare / --episodes-compare: also write the JSON here")
    args = ap.parse_args()
    if args.scenarios_variant:
        print(json.dumps(measure_scenarios(args.scenarios_variant, args.envs, args.robots, args.peds, args.obstacles, args.steps, args.time_max,
                                           args.scenarios)))
        return
    if args.minibatch_variant:
        print(json.dumps(measure_minibatch(args.minibatch_variant, args.envs, args.robots, args.peds, args.obstacles, args.time_max, args.horizon,
                                           args.batch)))
        return
    if args.sequences_variant:
        print(json.dumps(measure_sequences(args.sequences_variant, args.envs, args.robots, args.peds, args.obstacles, args.time_max, args.horizon,
                                           args.seq_length, args.seq_batch)))
        return
    if args.sequences_compare:
        res = compare_sequences(args, args.rounds)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        print(json.dumps(res["summary"]))
        return
    if args.ped_draw_variant:
        print(json.dumps(measure_ped_draw(args.ped_draw_variant, args.envs, args.robots, args.peds, args.obstacles, args.steps, args.time_max,
                                          args.horizon, args.batch)))
        return
    if args.ped_draw_compare:
        res = compare_ped_draw(args, args.rounds)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        print(json.dumps(res["summary"]))
        return
    if args.loss_compare:
        res = compare_loss(args, args.rounds)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        print(json.dumps(res["summary"]))
        return
    if args.minibatch_compare:
        res = compare_minibatch(args, args.rounds)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        print(json.dumps(res["summary"]))
        return
    if args.rollout_variant:
        print(json.dumps(measure_rollout(args.rollout_variant, args.envs, args.robots, args.peds, args.obstacles, args.steps, args.time_max,
                                         args.horizon)))
        return
    if args.rollout_compare:
        res = compare_rollout(args, args.rounds)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        print(json.dumps(res["summary"]))
        return
    if args.scenarios_compare:
        res = compare_scenarios(args, args.rounds)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        print(json.dumps(res["summary"]))
        return
    if args.tracks_compare:
        res = compare_tracks(args, args.rounds)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        print(json.dumps(res["summary"]))
        return
    if args.wrappers_compare:
        res = compare_wrappers(args, args.rounds)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        print(json.dumps(res["summary"]))
        return
    if args.policy_compare:
        res = compare_policy(args, args.rounds)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        print(json.dumps(res["summary"]))
        return
    if args.normalise_compare:
        res = compare_normalise(args, args.rounds)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        print(json.dumps(res["summary"]))
        return
    if args.final_obs_compare:
        res = compare_final_obs(args, args.rounds)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        print(json.dumps(res["summary"]))
        return
    if args.episode_log_compare:
        res = compare_episode_log(args, args.rounds)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        print(json.dumps(res["summary"]))
        return
    if args.episodes_compare:
        res = compare_episodes(args, args.rounds)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        print(json.dumps(res["summary"]))
        return
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
                             torch_stack=args.torch_stack, episodes="torch" if args.torch_episodes else "log" if args.episode_log else "library" if args.episodes else None,
                             wrappers=(args.wrappers, "torch" if args.torch_wrappers else "library") if args.wrappers else None)))


if __name__ == "__main__":
    main()
