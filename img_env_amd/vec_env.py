"""``VecImageEnv``: ``env_num`` copies of one reference YAML env in ONE library handle.

The reference trains on ``env_num`` env processes (create_launch.py:57-66 starts one C++ node per env, the trainer calls
``make_env(cfg)`` once per env and steps them side by side), each wrapped in the stack
``VelActionWrapper -> TimeLimitWrapper -> SensorsPaperRewardWrapper -> InfoLogWrapper -> MultiRobotCleanWrapper ->
NeverStopWrapper`` (envs/cfg/*.yaml ``wrapper:``).  Here all envs are worlds of one ``World`` (``imgenv_cfg.n_worlds``),
stepped by one set of kernel launches; the library's fused outputs ARE that wrapper stack (``rewards``, ``dones``,
``dones_info``, ``is_clean``), and the envs whose robots are all done are reset together in one
``imgenv_reset_worlds`` call (NeverStopWrapper, base.py:198-211), each from its own ``EnvPos`` spawn stream.

Robots are numbered env-major: env k owns rows ``[k * robot_total, (k + 1) * robot_total)`` of every tensor.
"""
import numpy as np

from . import _cabi, config, spawn
from .envs import ContinuousAction, ImageState

_PER_AGENT = ("robot_shape", "robot_size", "robot_sensor_cfg", "robot_size_last", "ped_shape", "ped_size", "ped_max_speed")


def stack_params(params, env_num):
    """the parameter dict of ``env_num`` copies of one world (per-robot / per-pedestrian rows repeat, env-major)"""
    p = dict(params)
    for k in _PER_AGENT:
        p[k] = np.concatenate([np.asarray(params[k])] * env_num, axis=0)
    p["n_robots"], p["n_peds"], p["n_worlds"] = params["n_robots"] * env_num, params["n_peds"] * env_num, env_num
    return p


_LOSS_FN = []


def _loss_function():
    """the ``torch.autograd.Function`` behind ``VecImageEnv.policy_loss`` (made once: torch is imported late): forward runs the
    library's three launches and returns ``stats[0]``, backward scales the library's gradients by the incoming one"""
    if not _LOSS_FN:
        import torch

        class PolicyLoss(torch.autograd.Function):
            @staticmethod
            def forward(ctx, run, fresh, params, values, log_std=None):
                out = run(params.detach(), values.detach(), None if log_std is None else log_std.detach())
                ctx.out, ctx.fresh, ctx.serial = out, fresh, fresh(None)
                ctx.shapes = (params.shape, values.shape, None if log_std is None else log_std.shape)
                return out["stats"][0].clone()

            @staticmethod
            def backward(ctx, grad):
                ctx.fresh(ctx.serial)
                out, (ps, vs, lss) = ctx.out, ctx.shapes
                grads = [None, None, (out["d_params"] * grad).reshape(ps), (out["d_values"] * grad).reshape(vs)]
                if lss is not None:
                    grads.append((out["d_log_std_shared" if len(lss) == 1 else "d_log_std"] * grad).reshape(lss))
                return tuple(grads)
        _LOSS_FN.append(PolicyLoss)
    return _LOSS_FN[0]


class VecImageEnv:
    """``reset() -> ImageState``; ``step(actions) -> (ImageState, rewards, dones, info)`` over ``env_num * robot_total`` robots.

    ``info``: ``dones_info`` (InfoLogWrapper codes, 10 = time limit), ``is_clean`` (MultiRobotCleanWrapper), ``arrive``,
    ``collision``, ``all_down`` (per robot: its env is finished) and ``reset_envs`` (the envs that were reset after this step:
    their rows of the returned state are already the new episode's first observation, as with NeverStopWrapper).
    ``wrappers=True``: ``step`` takes the policy's own output (indices or raw float rows) and ``info`` gains ``speeds`` and, with
    pedestrians, ``bool_get_close_to_human`` (of the state handed out: an env that restarted shows its new episode's).
    ``final_obs=True``: ``info`` gains ``final_observation`` (Gym's: the state the restarted envs' last action led to, in the rows
    where ``all_down`` is set; other rows hold older captures) and ``final_count``.
    ``rollout=T``: the trainer's ``[T, n, ...]`` storage and the advantage pass inside the library: ``rollout()``,
    ``rollout_begin()``, ``rollout_advantages(values, final_values, gamma, lam)``.  ``rollout_draw_ped_maps=True``: the storage
    keeps no ``ped_maps`` (78 % of a default slot) but the pedestrian vectors they are a function of; the minibatches draw
    ``mb_ped_maps`` from those, ``rollout_ped_maps(t)`` and ``rollout_final_ped_maps()`` draw a slot and the final list.
    ``minibatch=B`` (with ``rollout=T``): the PPO epoch's minibatches gathered by the library, without a host read:
    ``rollout_minibatches(scalars, seed, normalise)``.
    ``sequences=dict(length=L, batch=Bs, buffers=1, state_bytes=())`` (with ``rollout=T``): minibatches of whole sequences for a
    recurrent policy, time-major ``[L, Bs, ...]``: ``rollout_sequences(scalars, seed, states)``, ``sequence_rows(mb)``.
    ``normalise=dict(...)``: running normalisation of ``vector_states`` and of the reward inside the library (VecNormalize): the
    state and the reward handed out are the normalised ones, ``info`` gains ``raw_vector_states`` and ``raw_rewards``.
    ``policy=dict(seed=s)`` (with ``wrappers=True``): the action sampled from the network's logits (or mean and log-std) inside
    the library: ``policy_sample(...)``, ``policy_step(...)``, ``policy_value(values)``, ``policy_draw``.  ``policy=dict(seed=s,
    loss=True)`` (with ``minibatch=B``) adds PPO's loss and its gradients on the device: ``policy_loss(mb, ...)``.
    """

    def __init__(self, cfg, env_num=None, seed=None, auto_reset=True, native_spawn=False, device_reset=False, stack=False,
                 map_policy="keep", world_maps=None, episode_stats=False, episode_min_steps=3, wrappers=False,
                 ped_tracks=None, tracks_policy="keep", tracks_repeat=1, info_track_sets=False, scenarios=None, scenario_policy="queue",
                 episode_log=0, final_obs=False, rollout=0, rollout_final=None, rollout_fields=None, minibatch=0, minibatch_buffers=1,
                 normalise=None, policy=None, rollout_draw_ped_maps=False, sequences=None):
        import torch
        from .world import World
        if int(minibatch or 0) > 0 and int(rollout or 0) <= 0:
            raise ValueError("minibatch=B needs rollout=T")
        if sequences is not None and int(rollout or 0) <= 0:
            raise ValueError("sequences=dict(length=L, batch=Bs) needs rollout=T")
        if sequences is not None and (set(sequences) - {"length", "batch", "buffers", "state_bytes"} or not {"length", "batch"} <= set(sequences)):
            raise ValueError("sequences: dict(length=L, batch=Bs, buffers=1, state_bytes=())")
        if rollout_draw_ped_maps and int(rollout or 0) <= 0:
            raise ValueError("rollout_draw_ped_maps=True needs rollout=T")
        if policy is not None and not wrappers:
            raise ValueError("policy=dict(seed=s) needs wrappers=True")
        if policy is not None and set(policy) - {"seed", "loss"}:
            raise ValueError("policy: unknown %s (known: seed, loss)" % sorted(set(policy) - {"seed", "loss"}))
        if policy is not None and policy.get("loss") and not minibatch:
            raise ValueError("policy=dict(loss=True) needs minibatch=B")
        self.cfg = cfg
        self.env_num = int(env_num if env_num is not None else cfg.get("env_num", 1))
        # ped_tracks: the recorded crowds of ``ped_sim.type: dataset`` as a bank inside the handle (imgenv_tracks_add) -- a list of
        # sets ([P, T, 5] rows x, y, yaw, vx, vy, or (series, lengths) pairs) or "yaml" for envs.dataset_track_sets(cfg), which also
        # fixes ped_sim.total from the first world as the reference's wrapper does.  Every reset mode then works for a dataset YAML
        # (Python spawn, native_spawn, device_reset): a reset takes the env's pedestrians from the bank.  tracks_policy: "keep"
        # (set_world_tracks chooses), "placement" (drawn with the placement's seed; native_spawn / device_reset) or "cycle" (the
        # reference wrapper's order, tracks_repeat = repeated_time_per_env).  None: a dataset VecImageEnv behaves as before.
        if ped_tracks is not None and cfg["ped_sim"].get("type") != "dataset":
            raise ValueError("ped_tracks needs ped_sim.type: dataset")
        if tracks_policy not in _cabi.TRACK_POLICIES:
            raise ValueError("tracks_policy: keep | placement | cycle")
        if scenarios is not None and scenario_policy not in ("queue", "placement"):
            raise ValueError("scenario_policy: queue | placement")
        if scenarios is not None and auto_reset and not device_reset:
            raise ValueError("scenarios need device_reset=True or auto_reset=False (the host-side auto-reset keeps sampling)")
        if isinstance(ped_tracks, str):
            if ped_tracks != "yaml":
                raise ValueError('ped_tracks: a list of sets or "yaml"')
            from .envs import dataset_track_sets
            ped_tracks = dataset_track_sets(cfg)
            cfg["ped_sim"]["total"] = int(ped_tracks[0][0].shape[0])
        self.params = config.params_from_cfg(cfg)
        self.grid = config.load_map(cfg)
        self.robot_total = self.params["n_robots"]  # per env, as in the reference
        self.ped_total = self.params["n_peds"]
        self.auto_reset = auto_reset
        seed = cfg.get("seed") if seed is None else seed
        self.env_poses = [spawn.EnvPos(cfg, seed=None if seed is None else seed + k) for k in range(self.env_num)]
        # native_spawn: the placements of an episode are drawn inside the library (csrc/spawn_host.h: EnvPos' rules, its own
        # random stream) -- the Python EnvPos costs 40-170 us per small env, twenty times the device's whole step
        # device_reset: NeverStopWrapper without the host in the loop (imgenv_step_autoreset_device): finished envs are found,
        # placed and reset by kernels alone, ``step`` returns without synchronising and ``info["reset_envs"]`` is None --
        # ``info["all_down"]`` (a device tensor, per robot) says which envs started over
        self.device_reset = bool(device_reset)
        self.native_spawn = bool(native_spawn) or self.device_reset
        native_spawn = self.native_spawn
        self._spawn_cfg = spawn.make_spawn_cfg(cfg) if native_spawn else None
        self._spawn_seed = (0x9E3779B97F4A7C15 * (1 + (seed or 0))) & 0xFFFFFFFFFFFFFFFF
        self._episodes = 0
        # device-side resets number their placements seed0 + k on their own: a stream 2^63 away from the host-side resets'
        # (_spawn_seed + episodes so far), so that an env reset by the host never replays an episode the device handed out
        self._device_seed0 = (self._spawn_seed + (1 << 63)) & 0xFFFFFFFFFFFFFFFF
        self._extent = max(self.grid.shape[-2:]) * float(cfg["global_map"]["resolution"])
        if not cfg.get("keep_view_maps", False):
            # ImageState has no full-size view: where the view is shrunk into the sensor_map (the shipped 400 x 400 -> 48 x 48)
            # the library then only evaluates the view cells the shrink reads (IMGENV_FLAG_NO_VIEW_MAPS)
            self.params["flags"] = int(self.params.get("flags", 0)) | _cabi.FLAG_NO_VIEW_MAPS
        self.world = World(stack_params(self.params, self.env_num), self.grid, device=cfg.get("device", 0))
        self._all_down = self.world.out["step_all_down"].view(torch.bool) if native_spawn else None
        # Several maps (global_map.map_file a list, map_array 3-D): the maps of the handle's bank.  world_maps[k] is the map env k
        # starts on; None spreads them k % n_maps -- the reference's layout of several YAMLs with env_num envs each
        # (create_launch.py:57-65).  map_policy "keep": an env stays on its map until set_world_maps moves it; "placement": every
        # new episode draws its map with its placement (imgenv_maps_policy), which needs the placements to be drawn inside the
        # library (native_spawn or device_reset).
        if map_policy not in _cabi.MAP_POLICIES:
            raise ValueError("map_policy: keep | placement")
        if map_policy == "placement" and not self.native_spawn:
            raise ValueError('map_policy="placement" needs native_spawn=True or device_reset=True')
        self.n_maps = self.world.n_maps
        self.map_policy = map_policy
        if world_maps is None:
            world_maps = [k % self.n_maps for k in range(self.env_num)]
        if len(world_maps) != self.env_num:
            raise ValueError("world_maps: one map id per env")
        if self.n_maps > 1 or any(int(m) != 0 for m in world_maps):
            self.world.set_world_maps(range(self.env_num), world_maps)
        self.world.set_maps_policy(map_policy)
        self.tracks_policy = tracks_policy
        self.info_track_sets = bool(info_track_sets)  # info["track_sets"]: world_tracks() with every step -- it synchronises
        if ped_tracks is not None:
            if tracks_policy == "placement" and not self.native_spawn:
                raise ValueError('tracks_policy="placement" needs native_spawn=True or device_reset=True')
            self.world.tracks_add(ped_tracks)
            self.world.tracks_policy(tracks_policy, tracks_repeat)
        elif tracks_policy != "keep" or self.info_track_sets:
            raise ValueError("tracks_policy / info_track_sets need ped_tracks")
        self.n_track_sets = self.world.n_track_sets
        # scenarios: a fixed list of recorded episodes (the reference's cfg_type: bag, yaml_env.py:223-244) as a bank inside the
        # handle (imgenv_scenarios_add) -- a list of layouts, e.g. spawn.record_scenarios(cfg, n, seed).  reset() gives env k episode
        # k % N; with device_reset=True the device-side reset then continues the queue (scenario_policy "queue": the k-th env reset
        # from then on replays episode (env_num + k) % N) or draws an episode with every placement ("placement").  With
        # auto_reset=False the caller chooses: reset_envs(envs, scenario_ids=...).  None: nothing changes.
        self.n_scenarios = 0
        self.scenario_policy = scenario_policy
        if scenarios is not None:
            self.world.scenarios_add(scenarios)
            self.n_scenarios = self.world.n_scenarios
        # stack: StateBatchWrapper (base.py:97-150) inside the library, per env (imgenv_stack_enable): every state handed out
        # carries each robot's last cfg["image_batch"] sensor maps, cfg["state_batch"] vector states and
        # max(cfg["laser_batch"], 1) laser scans of its env's current episode, zero-padded after the env's reset -- whoever reset it,
        # the host or the device.  If the YAML's wrapper list ends in ObsStateTmp / ObsLaserStateTmp (filter_states.py:6-20) the
        # state is that wrapper's list of three tensors.  Opt-in: False hands out single frames, as before.
        self.stack = bool(stack)
        self._filter = None
        if self.stack:
            self.world.enable_stack(int(cfg.get("image_batch", 0)), int(cfg.get("state_batch", 0)), int(cfg.get("laser_batch", -1)))
            names = [w for w in (cfg.get("wrapper") or []) if w in ("ObsStateTmp", "ObsLaserStateTmp")]
            self._filter = names[-1] if names else None
        # episode_stats: TestEpisodeWrapper (evaluation_wrapper/TestEpisodeWrapper.py:8-119) inside the library, per robot of every
        # env (imgenv_episodes_enable): how episodes end, steps to arrive, returns, lengths and the path figures of the commands,
        # kept by one small launch per chain -- also where the device resets the envs and the host never sees an episode end.
        # Opt-in: False launches nothing.
        # episode_log=N: besides the totals, one record per finished episode in a ring of N records on the device
        # (imgenv_episode_log_enable): how it ended, its steps, return and figures, and the map / track set / scenario / placement it
        # ran on -- one more small launch per RESET chain, none per step.  Implies episode_stats.  episode_log() reads it.
        self._log_capacity = int(episode_log or 0)
        self._log_cursor = 0
        self.episode_stats = bool(episode_stats) or self._log_capacity > 0
        if self.episode_stats:
            self.world.enable_episodes(int(episode_min_steps), float(cfg["control_hz"]))
        if self._log_capacity > 0:
            self.world.enable_episode_log(self._log_capacity)

        # wrappers: the input side of the YAML's wrapper list and its two small output wrappers inside the library.
        #   VelActionWrapper (base.py:37-66): ``step`` takes what the policy emits -- a 1-D integer array of indices into
        #   cfg["discrete_actions"] (discrete_action: True) or a 2-D float array [n, act_dim], clipped by cfg["continuous_actions"]
        #   where discrete_action is False -- and decodes it with one launch in front of the step (imgenv_actions_decode);
        #   info["speeds"] is the decoded (v, w) masked by the is_clean of before the step (base.py:58, 81-83).
        #   StatePedVectorWrapper (base.py:19-34), iff the YAML lists it: the state's ped_vector_states is the normalised array.
        #   info["bool_get_close_to_human"] (base.py:250-252), iff the envs have pedestrians.
        # Opt-in: False takes float32 [n, 3] = (v, w, beep) and launches nothing more, as before.
        self.wrappers = bool(wrappers)
        self._ped_norm = self._close = False
        if self.wrappers:
            act_dim = int(cfg.get("act_dim", 2))
            if cfg.get("discrete_action"):
                self.world.enable_actions(discrete_actions=cfg["discrete_actions"], act_dim=act_dim)
            else:
                self.world.enable_actions(continuous_actions=cfg["continuous_actions"], act_dim=act_dim)
            self._ped_norm = "StatePedVectorWrapper" in (cfg.get("wrapper") or [])
            self._close = self.ped_total > 0
            if self._ped_norm or self._close:
                self.world.enable_obs_post(ped_norm=self._ped_norm, close=self._close)
        # normalise: Stable-Baselines3's VecNormalize inside the library (imgenv_normalise_enable) -- a dict of obs, reward, gamma,
        # clip_obs, clip_reward, eps (defaults: True, True, 0.99, 10, 10, 1e-8).  The state's vector_states (and its stack) are then
        # the normalised arrays and the returned reward the normalised one; info["raw_vector_states"] / info["raw_rewards"] are the
        # untouched ones.  The running statistics count the robots that are not frozen, also where the device resets the envs;
        # episode statistics and the episode log keep the raw rewards.  normalise_training(False) freezes them for evaluation,
        # normalise_stats() / load_normalise_stats() carry them through a checkpoint.  At most two more launches per chain; nothing
        # synchronises.  Opt-in: None allocates and launches nothing.
        self.normalise = dict(normalise) if normalise else None
        self._norm_obs = self._norm_reward = False
        if self.normalise is not None:
            self.world.enable_normalise(**self.normalise)
            self._norm_obs, self._norm_reward = bool(self.normalise.get("obs", True)), bool(self.normalise.get("reward", True))
        # final_obs: Gym's final_observation (imgenv_final_obs_enable).  Every reset first copies the rows it is about to overwrite
        # -- the observation the env's last action led to, which a trainer needs to bootstrap a time-out -- into arrays of their
        # own: info["final_observation"] is the state in the form ``step`` hands out (stacks, filter list and normalised pedestrian
        # vector included) over those arrays, info["final_count"] how often each robot's row has been captured.  With auto_reset
        # the rows where info["all_down"] is set are this step's; the others hold older captures.  With auto_reset=False the rows
        # of whatever reset / reset_envs last covered.  One more launch per RESET chain, none per step; nothing synchronises.
        # Opt-in: False allocates and launches nothing.
        self.final_obs = bool(final_obs)
        if self.final_obs:
            fields = [n for n in list(_cabi.FINAL_BITS)[:9] if n != "lasers" or self.params.get("use_laser")]
            if self.stack and any(d >= 2 for d in self.world.stack_depths):
                fields.append("stacks")
            if self._ped_norm:
                fields.append("ped_vector_norm")
            if self._norm_obs:
                fields.append("norm_states")
            self.world.enable_final_obs(fields)
        # rollout=T: the trainer's [T, n, ...] storage inside the library (imgenv_rollout_enable).  After reset() every step also
        # stores its transition (action, reward, done, dones_info, is_clean) in slot t and the state it hands out in slot t + 1 of
        # rollout()'s tensors, and every reset -- Python spawn, native_spawn, device_reset or the caller's reset_envs -- first moves
        # the rows it overwrites into a final list of rollout_final entries (default: one per robot and slot), found through
        # final_idx.  rollout_advantages() is the GAE pass over it.  After T steps ``step`` raises until rollout_begin() starts the
        # next window from the last slot.  rollout_fields: names of _cabi.ROLLOUT_BITS; None = what the state handed out consists of
        # -- the single-frame fields (the whole stacks with stack=True, instead of the frames they cover; the normalised pedestrian
        # vector where the YAML lists StatePedVectorWrapper, instead of the raw one).  One more launch per chain; nothing
        # synchronises.  Opt-in: 0 allocates and launches nothing.
        self.rollout_horizon = int(rollout or 0)
        if self.rollout_horizon > 0:
            if rollout_fields is None:
                stacked = {"sensor_maps": 0, "vector_states": 1, "lasers": 2} if self.stack else {}
                fields = [n for n in list(_cabi.ROLLOUT_BITS)[:5] if (n != "lasers" or self.params.get("use_laser"))
                          and not (n in stacked and self.world.stack_depths[stacked[n]] >= 2) and not (n == "ped_vector_states" and self._ped_norm)]
                if self.stack and any(d >= 2 for d in self.world.stack_depths):
                    fields.append("stacks")
                if self._ped_norm:
                    fields.append("ped_vector_norm")
                if self._norm_obs:  # (the normalised state instead of the raw one)
                    fields = [n for n in fields if n != "vector_states"]
                if rollout_draw_ped_maps:  # the raw vector the maps are drawn from instead of the maps (beside the normalised one, if any)
                    fields = [n for n in fields if n not in ("ped_maps", "ped_vector_states")] + ["ped_vector_states", "ped_maps_drawn"]
            else:
                fields = rollout_fields
            if self.normalise is not None:  # the two bits follow the handle's normalisation: the ring holds what ``step`` hands out
                bits = (_cabi.ROLLOUT_NORM_STATES if self._norm_obs else 0) | (_cabi.ROLLOUT_NORM_REWARDS if self._norm_reward else 0)
                fields = (int(fields) if isinstance(fields, (int, np.integer)) else _cabi.make_rollout_cfg(1, 1, fields).fields) | bits
            final = int(rollout_final) if rollout_final is not None else (self.rollout_horizon + 1) * len(self)
            self.world.enable_rollout(self.rollout_horizon, final, fields)
        # minibatch=B: the minibatches of a PPO epoch out of that storage (imgenv_rollout_minibatch_enable): the transitions that
        # count (is_clean), their statistics, a fresh order and the gather of B of them into minibatch_buffers sets of contiguous
        # tensors -- rollout_minibatches().  Nothing is launched by steps or resets; nothing synchronises.  Opt-in: 0 allocates nothing.
        self.minibatch_batch = int(minibatch or 0)
        if self.minibatch_batch > 0:
            self.world.enable_minibatch(self.minibatch_batch, int(minibatch_buffers))
        # sequences=dict(...): the same window cut into chunks of L steps per robot for a recurrent policy (imgenv_rollout_seq_enable):
        # which chunks count, a fresh order over them and the gather of Bs of them into time-major tensors -- rollout_sequences().
        # Nothing is launched by steps or resets; nothing synchronises.  Opt-in: None allocates and launches nothing.
        self.sequences = dict(sequences) if sequences is not None else None
        if self.sequences is not None:
            self.world.enable_sequences(int(self.sequences["length"]), int(self.sequences["batch"]), int(self.sequences.get("buffers", 1)),
                                        None, tuple(self.sequences.get("state_bytes", ())))
        # policy=dict(seed=s) (with wrappers=True): the hop from the network's output to the action inside the library
        # (imgenv_policy_enable) -- categorical over cfg["discrete_actions"] where discrete_action is True, a diagonal Gaussian over
        # cfg["continuous_actions"] where not.  policy_sample() draws the action from logits / mean and log_std with a counter-based
        # generator keyed by (seed, policy_draw, robot), hands out its log-probability and entropy and leaves the decoded rows
        # where ``step`` would have put them; policy_step() is that and the step in one call; with rollout=T the action, its
        # log-probability and the value are kept in the window's slot (rollout()["pol_raw" | "pol_logp" | "pol_value"]) and
        # policy_value() adds the bootstrap value.  One launch instead of the decode's; nothing synchronises.  Opt-in: None
        # allocates and launches nothing.
        self.policy = dict(policy) if policy is not None else None
        self.policy_draw = 0  # the next call's draw number: part of a checkpoint, settable
        self._sampled = None
        if self.policy is not None:
            self._policy_cat = bool(cfg.get("discrete_action"))
            self.world.enable_policy("categorical" if self._policy_cat else "gaussian", int(self.policy.get("seed", 0)),
                                     store=self.rollout_horizon > 0)
            # loss=True: PPO's loss of a minibatch and its gradients on the network's outputs (imgenv_policy_loss_enable), three
            # launches instead of torch's chain of small ones and its autograd -- policy_loss().  Opt-in as well.
            if self.policy.get("loss"):
                rows = self.minibatch_batch  # (a sequence minibatch flattened by sequence_rows() has L Bs rows)
                if self.sequences is not None:
                    rows = max(rows, self.world.seq_length * self.world.seq_batch)
                self.world.enable_policy_loss(rows)

    def _need_policy(self):
        if self.policy is None:
            raise RuntimeError("VecImageEnv was made without policy=dict(seed=s)")

    def policy_sample(self, logits=None, mean=None, log_std=None, values=None, deterministic=False, store=True):
        """The action of every robot from the network's output: ``logits`` float32 ``[n, A]`` (discrete_action: True) or ``mean``
        ``[n, C]`` and ``log_std`` ``[C]`` / ``[n, C]``; ``values`` float32 ``[n]`` or None is kept with it where ``rollout=T``
        stores (``store=False``: an evaluation call that leaves the window alone).  Returns ``dict(actions, index | raw, logp,
        entropy)``: library-owned tensors, rewritten by the next call.  Uses draw number ``policy_draw`` and advances it."""
        self._need_policy()
        if (logits is None) != (not self._policy_cat):
            raise ValueError("policy_sample: %s" % ("logits" if self._policy_cat else "mean and log_std"))
        w = self.world
        actions = w.policy_sample(logits if self._policy_cat else mean, log_std, values, draw=self.policy_draw,
                                  deterministic=deterministic, store=store)
        self.policy_draw += 1
        key = "index" if self._policy_cat else "raw"
        return {"actions": actions, key: w.policy[key], "logp": w.policy["logp"], "entropy": w.policy["entropy"]}

    def policy_step(self, logits=None, mean=None, log_std=None, values=None, deterministic=False):
        """``policy_sample`` and ``step`` on the sampled actions, without a second decode: ``step``'s tuple, ``info["policy"]`` is
        what ``policy_sample`` returns"""
        sampled = self.policy_sample(logits, mean, log_std, values, deterministic)
        self._sampled = sampled["actions"]
        try:
            state, rewards, dones, info = self.step(None)
        finally:
            self._sampled = None
        info["policy"] = sampled
        return state, rewards, dones, info

    def policy_value(self, values):
        """``values`` float32 ``[n]`` into ``rollout()["pol_value"][t]``, t the transitions stored so far: after the window's last
        step, the bootstrap value of the state it led to (``IMGENV_POLICY_VALUE_ONLY``)"""
        self._need_policy()
        if self.rollout_horizon <= 0:
            raise RuntimeError("VecImageEnv was made without rollout=T")
        self.world.policy_value(values)

    def policy_loss(self, mb, logits=None, mean=None, log_std=None, values=None, clip=0.2, vf_coef=0.5, ent_coef=0.0, clip_vf=None,
                    keys=None):
        """PPO's loss of one minibatch on the device (``imgenv_policy_loss``): ``mb`` is a dict from ``rollout_minibatches``,
        ``logits`` ``[B, A]`` (or ``mean`` ``[B, C]`` and ``log_std`` ``[C]`` / ``[B, C]``) and ``values`` ``[B]`` are the
        network's outputs for ``mb``'s observations under its present parameters.  Returns ``(loss, info)``: ``loss`` is a 0-dim
        tensor whose ``backward()`` hands the library's closed-form gradients, times the incoming one, to ``logits`` / ``mean``,
        ``log_std`` and ``values`` -- ``loss.backward(); optimizer.step()`` as with a loss written in torch ops; call it before
        the next ``policy_loss`` (the gradients live in library-owned tensors that the next call rewrites; RuntimeError
        otherwise).  ``info``: ``loss``, ``pg_loss``, ``value_loss``, ``entropy``, ``approx_kl``, ``clip_fraction`` and
        ``weight_sum`` (0-dim views of ``stats``), ``n_bad``, and the row tensors ``logp``, ``row_entropy``, ``ratio``, ``pg``,
        ``vl``.  Nothing synchronises.  ``clip_vf``: the clipped value loss (needs the old values among the scalars).

        ``keys`` names ``mb``'s scalars: ``dict(action="action", old_logp="old_logp", old_value="old_value", adv="adv",
        ret="ret")``; for a Gaussian head ``action`` is the sequence of its C column names.  A PPO loop passes, with ``ro =
        rollout()`` and ``adv, ret = rollout_advantages(ro["pol_value"])``::

            scalars = dict(action=ro["pol_raw"][0], old_logp=ro["pol_logp"], old_value=ro["pol_value"], adv=adv, ret=ret)
            for mb in vec.rollout_minibatches(scalars, seed, normalise="adv"):
                logits, values = net(mb["mb_vector_states"])
                loss, info = vec.policy_loss(mb, logits=logits, values=values, clip_vf=0.2)
                optimizer.zero_grad(); loss.backward(); optimizer.step()

        (Gaussian: ``action0=ro["pol_raw"][0], action1=ro["pol_raw"][1], ...`` and ``keys=dict(action=("action0", "action1"))``.)
        A minibatch carries at most 6 scalars: a Gaussian head with C = 3 has 3 + old_logp + adv + ret already, so ``clip_vf``
        with C = 3 raises ValueError."""
        import torch
        self._need_policy()
        w = self.world
        if w.policy_loss_out is None:
            raise RuntimeError("VecImageEnv was made without policy=dict(seed=s, loss=True)")
        if (logits is None) != (not self._policy_cat) or values is None:
            raise ValueError("policy_loss: %s and values" % ("logits" if self._policy_cat else "mean and log_std"))
        names = dict(action="action", old_logp="old_logp", old_value="old_value", adv="adv", ret="ret")
        names.update(keys or {})
        C = w._pol_params
        if not self._policy_cat and C == 3 and clip_vf is not None:
            raise ValueError("policy_loss: clip_vf with a Gaussian head of 3 columns needs 7 scalars (3 action columns, old_logp, "
                             "old_value, adv, ret) and a minibatch carries %d" % _cabi.MB_MAX_SCALARS)
        if self._policy_cat:
            action = mb[names["action"]]
        else:
            cols = names["action"]
            action = [mb[k] for k in ((cols,) if isinstance(cols, str) else cols)]
        params = logits if self._policy_cat else mean
        old_value = mb[names["old_value"]] if clip_vf is not None else None

        def run(params, values, ls):
            return w.policy_loss(params, values.reshape(-1), action, mb[names["old_logp"]], mb[names["adv"]], mb[names["ret"]],
                                 mb["mb_weight"], log_std=ls, old_value=old_value, clip=clip, clip_vf=clip_vf, vf_coef=vf_coef,
                                 ent_coef=ent_coef)

        def fresh(serial):
            # (the World counts the calls it queued, whoever made them: forward notes its own, backward compares)
            if serial is not None and w.policy_loss_serial != serial:
                raise RuntimeError("policy_loss: backward() after a later policy_loss call has rewritten the gradients")
            return w.policy_loss_serial

        args = (params, values) if self._policy_cat else (params, values, log_std)
        if any(not isinstance(t, torch.Tensor) for t in args):
            raise ValueError("policy_loss: the network's outputs are torch tensors")
        loss = _loss_function().apply(run, fresh, *args)
        out = w.policy_loss_out
        info = {k: out["stats"][q] for q, k in enumerate(_cabi.PLOSS_STATS)}
        B = int(params.shape[0])
        info.update(n_bad=out["n_bad"], logp=out["logp"][:B], row_entropy=out["entropy"][:B], ratio=out["ratio"][:B], pg=out["pg"][:B],
                    vl=out["vl"][:B])
        return loss, info

    def rollout(self):
        """``{"n": transitions stored, "resets": reset chains stored, **World.rollout}``: the device tensors as they are -- no
        synchronisation; ordered on the current stream behind the last reset / step.  ``final_n[resets & 1]`` counts the final entries."""
        if self.rollout_horizon <= 0:
            raise RuntimeError("VecImageEnv was made without rollout=T")
        n, resets = self.world.rollout_cursor()
        out = dict(self.world.rollout, n=n, resets=resets)
        if self.policy is not None:  # the policy head's columns of the same window
            out.update({k: t for k, t in self.world.policy.items() if k.startswith("pol_")})
        return out

    def rollout_ped_maps(self, t):
        """``[n, 3, Hp, Wp]``: the pedestrian maps of slot ``t`` of a storage made with ``rollout_draw_ped_maps=True``, drawn from
        its ``obs_ped_vector_states[t]`` -- what ``obs_ped_maps[t]`` would hold.  One launch; nothing synchronises."""
        w = self.world
        if self.rollout_horizon <= 0 or not w.rollout_draws_ped_maps:
            raise RuntimeError("VecImageEnv was made without rollout=T, rollout_draw_ped_maps=True")
        if not 0 <= int(t) <= self.rollout_horizon:
            raise ValueError("rollout_ped_maps: slot %d of 0 .. %d" % (t, self.rollout_horizon))
        return w.draw_ped_maps(w.rollout["obs_ped_vector_states"][int(t)])

    def rollout_final_ped_maps(self):
        """``[rollout_final, 3, Hp, Wp]``: the pedestrian maps of the final list, drawn from ``final_ped_vector_states`` -- what
        ``final_ped_maps`` would hold; entries from ``final_n`` on are zeros (the list is zeroed memory).  One launch; nothing
        synchronises."""
        w = self.world
        if self.rollout_horizon <= 0 or not w.rollout_draws_ped_maps:
            raise RuntimeError("VecImageEnv was made without rollout=T, rollout_draw_ped_maps=True")
        return w.draw_ped_maps(w.rollout["final_ped_vector_states"])

    def rollout_begin(self):
        """start the next window: the last slot becomes slot 0 (``imgenv_rollout_begin``)"""
        if self.rollout_horizon <= 0:
            raise RuntimeError("VecImageEnv was made without rollout=T")
        self.world.rollout_begin()

    def rollout_advantages(self, values, final_values=None, gamma=0.99, lam=0.95):
        """``(adv, ret)`` float32 ``[T, n]`` of the stored transitions (``imgenv_rollout_gae``): ``values`` float32 ``[T + 1, n]``,
        the value of every slot's state; ``final_values`` float32 ``[rollout_final]`` or None, the value of every final entry"""
        if self.rollout_horizon <= 0:
            raise RuntimeError("VecImageEnv was made without rollout=T")
        return self.world.rollout_gae(values, final_values, gamma, lam)

    def rollout_minibatches(self, scalars, seed, normalise=None, eps=1e-8):
        """One epoch over the stored transitions that count (``is_clean != 0``), in a fresh order drawn from ``seed``: indexes once,
        computes the statistics of ``scalars[normalise]`` over exactly those transitions where ``normalise`` names a scalar, shuffles,
        then yields ``ceil(n * R / B)`` dicts of views -- the ``mb_*`` tensors of ``World.minibatch`` (``mb_<field>``, ``mb_actions``,
        ``mb_rewards``, ``mb_dones``, ``mb_dones_info``, ``mb_index``, ``mb_weight``) and every scalar under the caller's own name
        (float32 ``[B]``; the normalised one as ``(x - mean) / sqrt(var + eps)``).  ``scalars``: a dict of up to 6 float32 tensors
        ``[T, n]`` or ``[T + 1, n]``.  Slots behind the valid list have ``mb_weight`` 0 and zeros everywhere: a loss is
        ``(per_sample * w).sum() / w.sum().clamp(min=1)``; the trailing minibatches may be all such slots, since nobody on the host
        knows the count.  The buffers alternate: a dict is valid until ``minibatch_buffers`` further ones have been drawn.
        Nothing synchronises; everything is ordered on the current stream.  No step or reset while the generator runs."""
        if self.minibatch_batch <= 0:
            raise RuntimeError("VecImageEnv was made without minibatch=B")
        names = list(scalars)
        if normalise is not None and normalise not in scalars:
            raise ValueError("normalise: one of the scalars' names")
        w = self.world
        n, _ = w.rollout_cursor()
        w.rollout_index()
        if normalise is not None:
            w.rollout_stats(scalars[normalise], eps)
        w.rollout_shuffle(seed)
        B, tensors = self.minibatch_batch, [scalars[k] for k in names]
        return self._minibatches(names, tensors, None if normalise is None else names.index(normalise), -(-n * len(self) // B))

    def _minibatches(self, names, tensors, normalise, count):
        w = self.world
        for j in range(count):
            mb = w.rollout_minibatch(j, j % w.minibatch_buffers, tensors, normalise)
            rows = mb.pop("mb_scalars")
            for s, name in enumerate(names):
                mb[name] = rows[s]
            yield mb

    def rollout_sequences(self, scalars, seed, states=(), normalise=None, eps=1e-8):
        """One epoch over the stored window as sequences for a recurrent policy: robot ``row``'s steps ``c * L .. c * L + L - 1`` are
        sequence ``q = c * n_robots + row`` (chunks aligned to the window; an episode boundary inside one is marked by ``mb_first``,
        where the network resets its state).  Indexes the sequences with at least one transition that counts, shuffles them with
        ``seed`` and yields ``ceil(C * n_robots / Bs)`` dicts of time-major views ``[L, Bs, ...]`` -- the ``mb_*`` tensors of
        ``World.sequences`` and every scalar under the caller's own name (float32 ``[L, Bs]``).  ``mb_weight`` is 0 for a step that
        does not count or does not exist; ``mb_seq_state0`` / ``1`` ``[Bs, state_bytes]`` hold ``states[a]``'s row at each sequence's
        first step (``states``: tensors ``[T or T + 1, n, ...]``, the recurrent state the rollout saw there).  ``normalise`` names a
        scalar that comes out as ``(x - mean) / sqrt(var + eps)`` with the statistics over the valid TRANSITIONS (``minibatch=B``'s
        ``rollout_index`` + ``rollout_stats``: ValueError without ``minibatch``).  The buffers alternate; nothing synchronises.  No step
        or reset while the generator runs."""
        if self.sequences is None:
            raise RuntimeError("VecImageEnv was made without sequences=dict(length=L, batch=Bs)")
        names = list(scalars)
        if normalise is not None and normalise not in scalars:
            raise ValueError("normalise: one of the scalars' names")
        if normalise is not None and self.minibatch_batch <= 0:
            raise ValueError("rollout_sequences: normalise needs minibatch >= 1 (the statistics over the valid transitions are the minibatches')")
        w = self.world
        n, _ = w.rollout_cursor()
        norm = None
        if normalise is not None:
            w.rollout_index()
            norm = w.rollout_stats(scalars[normalise], eps)
        w.rollout_seq_index()
        w.rollout_seq_shuffle(seed)
        count = -(-(-(-n // w.seq_length)) * len(self) // w.seq_batch)
        return self._sequences(names, [scalars[k] for k in names], None if normalise is None else names.index(normalise), norm, list(states), count)

    def _sequences(self, names, tensors, normalise, norm, states, count):
        w = self.world
        for j in range(count):
            mb = w.rollout_seq_minibatch(j, j % w.seq_buffers, tensors, normalise, norm, states)
            rows = mb.pop("mb_scalars")
            for s, name in enumerate(names):
                mb[name] = rows[s]
            yield mb

    def sequence_rows(self, mb):
        """a dict from ``rollout_sequences`` with every ``[L, Bs, ...]`` tensor as its flat ``[L * Bs, ...]`` view (row ``l * Bs + i``;
        the per-sequence ``mb_seq``, ``mb_seq_len`` and ``mb_seq_state*`` as they are): ``policy_loss(sequence_rows(mb), ...)``"""
        if self.sequences is None:
            raise RuntimeError("VecImageEnv was made without sequences=dict(length=L, batch=Bs)")
        L, Bs = self.world.seq_length, self.world.seq_batch
        return {k: (t.reshape((L * Bs,) + tuple(t.shape[2:])) if k not in ("mb_seq", "mb_seq_len") and not k.startswith("mb_seq_state") else t)
                for k, t in mb.items()}

    def episode_tensors(self):
        """the per-robot device tensors of the statistics (``World.episodes``: ``ends`` [6, n], ``episodes``, ``last_episode``,
        ``last_return`` ...), as they are -- no synchronisation; ordered on the current stream behind the last reset / step"""
        if not self.episode_stats:
            raise RuntimeError("VecImageEnv was made without episode_stats=True")
        return self.world.episodes

    def episode_statistics(self):
        """The keys of the reference's ``TestEpisodeWrapper`` print-out (TestEpisodeWrapper.py:87-117) over all robots of all envs
        and their counted episodes so far -- the reference divides by ``max_episodes``, which is the number of counted episodes when
        it prints -- plus ``aborted_rate``, ``episodes``, ``short_episodes``, ``avg_return`` and ``avg_len``.  SYNCHRONISES: it waits
        for the stream and copies a few small tensors to the host."""
        import torch
        e = {k: v.sum(dim=-1) for k, v in self.episode_tensors().items()
             if k in ("ends", "episodes", "short_episodes", "speed_steps", "arrive_steps", "len_sum", "v_sum", "w_sum", "figure_sums",
                      "return_sum")}
        torch.cuda.current_stream(self.world.device).synchronize()
        e = {k: v.cpu().numpy() for k, v in e.items()}
        ends = dict(zip(_cabi.EP_ENDS, (int(c) for c in e["ends"])))
        fig = dict(zip(_cabi.EP_FIGURE_NAMES, (float(x) for x in e["figure_sums"])))
        n, steps = max(1, int(e["episodes"])), max(1, int(e["speed_steps"]))
        return dict(arrive_rate=ends["arrive"] / n, static_coll_rate=ends["static_collision"] / n, ped_coll_rate=ends["ped_collision"] / n,
                    other_coll_rate=ends["other_collision"] / n, avg_arrive_steps=int(e["arrive_steps"]) / max(1, ends["arrive"]),
                    stuck_rate=ends["timeout"] / n, avg_v=float(e["v_sum"]) / steps, avg_w=float(e["w_sum"]) / steps,
                    avg_w_variance=fig["w_variance"] / n, avg_v_jerk=fig["v_jerk"] / n, avg_w_jerk=fig["w_jerk"] / n,
                    avg_w_zero=fig["w_zero"] / n, aborted_rate=ends["aborted"] / n, episodes=int(e["episodes"]),
                    short_episodes=int(e["short_episodes"]), avg_return=float(e["return_sum"]) / n, avg_len=int(e["len_sum"]) / n)

    def episode_log(self, since=None):
        """The finished episodes' records as a dict of numpy columns: ``seq``, ``placement`` (uint64; ~0: none), ``robot``,
        ``world``, ``code``, ``steps``, ``len``, ``counted``, ``episode``, ``map``, ``tracks``, ``scenario`` (int32), ``ep_return``
        and the eight figures ``w_variance ... w_avg`` (float64), in log order; plus the scalars ``oldest`` and ``n_written``.
        ``since=None`` continues behind the last call's records (a cursor kept here); an integer starts at that ``seq``.  Records
        the ring has overwritten are gone: the first ``seq`` returned is then ``oldest``.  SYNCHRONISES: it waits for the stream
        and copies the records to the host (``imgenv_episode_log_read``)."""
        if self._log_capacity <= 0:
            raise RuntimeError("VecImageEnv was made without episode_log=N")
        first = self._log_cursor if since is None else int(since)
        rec, oldest, written = self.world.read_episode_log(first)
        self._log_cursor = written
        out = {k: np.ascontiguousarray(rec[k]) for k in rec.dtype.names if k != "figures"}
        for q, name in enumerate(_cabi.EP_FIGURE_NAMES):
            out[name] = np.ascontiguousarray(rec["figures"][:, q])
        out["oldest"], out["n_written"] = oldest, written
        return out

    def clear_episode_statistics(self):
        """every total and the open episodes' sums back to zero (``imgenv_episodes_clear``), ordered on the current stream"""
        if not self.episode_stats:
            raise RuntimeError("VecImageEnv was made without episode_stats=True")
        self.world.clear_episodes()

    def __len__(self):
        return self.env_num * self.robot_total

    def _state(self, final=False):
        o = self.world.out
        if final:  # the same form over the final arrays (a handle without a laser keeps no final lasers: the live placeholder)
            f = self.world.final_obs
            o = {name: f.get(name, t) for name, t in o.items()}
        ped_vector = (f if final else self.world.obs_post)["ped_vector_norm"] if self._ped_norm else o["ped_vector_states"]
        norm = (f if final else self.world.normalise) if self._norm_obs else None
        if norm is not None:  # normalise: the state's vector_states is the normalised array
            o = dict(o, vector_states=norm["norm_vector_states"])
        if not self.stack:
            return ImageState(o["vector_states"], o["sensor_maps"], o["is_collisions"], o["is_arrives"], o["lasers"],
                              ped_vector, o["ped_maps"], o["step_ds"], o["ped_min_dists"])
        k = self.world.stack
        if final:  # a stack of depth 1 is the field itself, in the stack's shape
            k = {name: f["stack_" + name] if "stack_" + name in f else o[name].view(t.shape) for name, t in k.items()}
        if norm is not None and "vector_states" in k:  # ... and so is its stack (depth 1: the normalised array itself)
            k = dict(k, vector_states=norm["norm_state_stack"] if "norm_state_stack" in norm else o["vector_states"].view(k["vector_states"].shape))
        vector_states, sensor_maps, lasers = (k.get(f_, o[f_]) for f_ in ("vector_states", "sensor_maps", "lasers"))
        if self._filter == "ObsStateTmp":
            return [sensor_maps, vector_states, o["ped_maps"]]
        if self._filter == "ObsLaserStateTmp":
            return [lasers, vector_states, o["ped_maps"]]
        return ImageState(vector_states, sensor_maps, o["is_collisions"], o["is_arrives"], lasers,
                          ped_vector, o["ped_maps"], o["step_ds"], o["ped_min_dists"])

    def reset(self, layouts=None):
        """every env starts a new episode (ImageEnv.reset per env, yaml_env.py:296-317); with ``rollout=T`` a new window starts"""
        state = self._reset(layouts)
        if self.rollout_horizon > 0:
            self.world.rollout_begin()
        return state

    def _reset(self, layouts=None):
        if layouts is None and self.n_scenarios:  # env k replays episode k % N; the device continues the queue from env_num on
            self.world.reset_worlds_scenarios(range(self.env_num), [k % self.n_scenarios for k in range(self.env_num)])
            if self.device_reset:
                self.world.scenarios_policy(self.scenario_policy, first=self.env_num)
            return self._state()
        if layouts is None and self.native_spawn:
            return self.reset_envs(range(self.env_num))
        if layouts is None:
            layouts = [ep.reset(self._extent) for ep in self.env_poses]
        self.world.reset(list(layouts))
        return self._state()

    def reset_envs(self, envs, layouts=None, scenario_ids=None):
        envs = [int(k) for k in envs]
        if scenario_ids is not None:  # env envs[q] starts the bank's episode scenario_ids[q]
            if layouts is not None or not self.n_scenarios:
                raise ValueError("scenario_ids need a VecImageEnv made with scenarios, and no layouts beside them")
            self.world.reset_worlds_scenarios(envs, scenario_ids)
            return self._state()
        if layouts is None and self.native_spawn:
            seeds = [self._spawn_seed + self._episodes + q for q in range(len(envs))]
            self._episodes += len(envs)
            self.world.reset_worlds_spawn(envs, self._spawn_cfg, seeds)
            return self._state()
        if layouts is None:
            layouts = [self.env_poses[k].reset(self._extent) for k in envs]
        self.world.reset_worlds(envs, layouts)
        return self._state()

    def _info(self, info):
        """what ``wrappers=True`` adds: library-owned tensors, rewritten by the next decode / chain"""
        if self.wrappers:
            info["speeds"] = self.world.action_outputs["speeds"]
            if self._close:
                info["bool_get_close_to_human"] = self.world.obs_post["close_to_human"]
        if self.info_track_sets:
            info["track_sets"] = self.world.world_tracks()
        if self.final_obs:
            info["final_observation"] = self._state(final=True)
            info["final_count"] = self.world.final_obs["final_count"]
        if self._norm_obs:
            info["raw_vector_states"] = self.world.out["vector_states"]
        return info

    def _rewards(self, rewards, info):
        """normalise: the reward handed out is the normalised one (library-owned, rewritten by the next step)"""
        if not self._norm_reward:
            return rewards
        info["raw_rewards"] = rewards
        return self.world.normalise["norm_rewards"]

    def normalise_training(self, on):
        """True: steps and resets update the running statistics (the default); False: they only apply them (evaluation)"""
        self.world.normalise_training(on)

    def normalise_stats(self):
        """the running statistics and returns as a dict of host values (``World.normalise_stats``); synchronises"""
        return self.world.normalise_stats()

    def load_normalise_stats(self, stats):
        """what ``normalise_stats()`` returned, of this env or another one of the same shape; synchronises"""
        self.world.load_normalise_stats(stats)

    def _actions(self, actions):
        if self._sampled is not None:  # policy_step: the policy head has already written the decoded rows
            return self._sampled
        if self.wrappers:  # the policy's output: indices [n] or float rows [n, act_dim], decoded on the device
            return self.world.decode_actions(actions)
        if isinstance(actions, (list, tuple)) and len(actions) and isinstance(actions[0], ContinuousAction):
            actions = np.array([[a.v, a.w, a.beep] for a in actions], np.float32)  # float32 wire (Agent.msg:8-10)
        return actions

    def _step_native(self, actions):
        """step + NeverStopWrapper inside the library (``imgenv_step_autoreset``): the finished envs are found on the device,
        their placements drawn on the host in C++, the per-robot results of the step itself kept in ``out['step_*']`` --
        no tensor work on the Python side"""
        o, finished = self.world.step_autoreset(self._actions(actions), self._spawn_cfg, self._spawn_seed + self._episodes)
        self._episodes += len(finished)
        info = {"dones_info": o["step_dones_info"], "is_clean": o["step_is_clean"], "arrive": o["step_is_arrives"],
                "collision": o["step_is_collisions"], "all_down": self._all_down, "reset_envs": finished}
        return self._state(), self._rewards(o["step_rewards"], info), o["step_dones"], self._info(info)

    def _step_device(self, actions):
        o = self.world.step_autoreset_device(self._actions(actions), self._spawn_cfg, self._device_seed0)
        info = {"dones_info": o["step_dones_info"], "is_clean": o["step_is_clean"], "arrive": o["step_is_arrives"],
                "collision": o["step_is_collisions"], "all_down": self._all_down, "reset_envs": None}
        return self._state(), self._rewards(o["step_rewards"], info), o["step_dones"], self._info(info)

    def step(self, actions):
        import torch
        if self.device_reset and self.auto_reset:
            return self._step_device(actions)
        if self.native_spawn and self.auto_reset:
            return self._step_native(actions)
        o = self.world.step(self._actions(actions))
        E, R = self.env_num, self.robot_total
        all_down = (o["dones"].view(E, R) > 0).all(dim=1)
        info = {"dones_info": o["dones_info"], "is_clean": o["is_clean"], "arrive": o["is_arrives"],
                "collision": o["is_collisions"], "all_down": all_down.repeat_interleave(R), "reset_envs": []}
        rewards, dones = o["rewards"], o["dones"]
        if self.auto_reset:
            finished = torch.nonzero(all_down).flatten().tolist()  # the one host read per step (NeverStopWrapper reads it too)
            if finished:
                # the reset rewrites the finished envs' rows in place: hand out this step's values, not the new episode's
                rewards, dones = rewards.clone(), dones.clone()
                info["dones_info"], info["is_clean"] = o["dones_info"].clone(), o["is_clean"].clone()
                info["arrive"], info["collision"] = o["is_arrives"].clone(), o["is_collisions"].clone()
                self.reset_envs(finished)
                info["reset_envs"] = finished
        return self._state(), self._rewards(rewards, info), dones, self._info(info)

    def world_maps(self):
        """the map each env's current episode runs on (numpy int32 ``[env_num]``); synchronises the stream"""
        return self.world.world_maps()

    def set_world_maps(self, envs, ids):
        """env ``envs[q]`` moves to map ``ids[q]`` at its next reset"""
        self.world.set_world_maps(envs, ids)

    def world_tracks(self):
        """the track set each env's current episode replays, -1 where its reset brought its own (numpy int32 ``[env_num]``);
        synchronises the stream"""
        return self.world.world_tracks()

    def world_scenarios(self):
        """the recorded episode each env's current episode replays, -1 where its reset did not come from the bank (numpy int32
        ``[env_num]``); synchronises the stream"""
        return self.world.world_scenarios()

    def set_world_tracks(self, envs, ids):
        """env ``envs[q]`` replays set ``ids[q]`` from its next bank-fed reset on (tracks_policy "keep")"""
        self.world.set_world_tracks(envs, ids)

    def end_ep(self, robot_res=None):
        return True

    def close(self):
        self.world.close()
