"""``World``: one img_env world living on one GPU, a thin Python object over the C ABI.

torch is plumbing only: it owns the output arena (so every output is a zero-copy ``torch.Tensor``
view of library-written HBM), provides the stream, and runs the RCCL all-gather of a robot-sharded
world.  All simulation work happens in ``csrc/libimgenv_hip.so``.
"""
import ctypes as C
import os
import types

import numpy as np

from . import _cabi

_TORCH_DTYPES = None


def _torch_dtype(np_dtype):
    global _TORCH_DTYPES
    import torch
    if _TORCH_DTYPES is None:
        _TORCH_DTYPES = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
                         np.dtype(np.float16): torch.float16, np.dtype(np.uint8): torch.uint8,
                         np.dtype(np.int8): torch.int8, np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}
    return _TORCH_DTYPES[np.dtype(np_dtype)]


class _DeviceArray:
    """library-owned device memory as the CUDA array interface describes it: ``torch.as_tensor`` makes a zero-copy view of it"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2,
                                         "strides": None}


class World:
    """create -> reset(layout) -> step(actions) ... ; ``out`` maps output names to device tensors."""

    def __init__(self, params, grid, device=0):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("img_env_amd.World needs a ROCm GPU (there is no CPU fallback)")
        self.lib = _cabi.load_library()
        self.device = torch.device("cuda", device if isinstance(device, int) else device.index)
        self.params = dict(params)
        self.params["device"] = self.device.index
        # Output ownership.  The reference hands out fresh copies with every step (ROS responses); this library hands out its
        # working copies, read-only by contract (include/imgenv.h).  params["output_guard"] (or IMGENV_OUTPUT_GUARD in the
        # environment, which wins): "first" (THE DEFAULT) = IMGENV_FLAG_CHECK_OUTPUTS_FIRST, a write by the caller during the
        # handle's first 64 calls fails the next call, loudly, and the guard then switches itself off; "check" = the same for
        # good (IMGENV_FLAG_CHECK_OUTPUTS); "copy" = IMGENV_FLAG_FULL_REWRITE, `out` is then a second arena rewritten in full by
        # every call; "none" = the bare C-ABI default.
        guard = os.environ.get("IMGENV_OUTPUT_GUARD") or self.params.pop("output_guard", None) or "first"
        self.params.pop("output_guard", None)
        if guard not in ("none", "first", "check", "copy"):
            raise ValueError("output_guard: none | first | check | copy")
        if guard == "check":
            self.params["flags"] = int(self.params.get("flags", 0)) | _cabi.FLAG_CHECK_OUTPUTS
        elif guard == "copy":
            self.params["flags"] = int(self.params.get("flags", 0)) | _cabi.FLAG_FULL_REWRITE
        elif guard == "first" and not int(self.params.get("flags", 0)) & (_cabi.FLAG_CHECK_OUTPUTS | _cabi.FLAG_FULL_REWRITE):
            self.params["flags"] = int(self.params.get("flags", 0)) | _cabi.FLAG_CHECK_OUTPUTS_FIRST
        self.output_guard = guard
        # grid: one 2-D map, or a 3-D array / list of equal-shaped 2-D maps -- the first is the map of imgenv_create, the rest
        # join it in the handle's bank (imgenv_maps_add); every world starts on map 0
        if isinstance(grid, (list, tuple)) or np.ndim(grid) == 3:
            maps = [np.ascontiguousarray(m, np.uint8) for m in grid]
            if not maps or any(m.ndim != 2 or m.shape != maps[0].shape for m in maps):
                raise ValueError("grid: a 2-D map or a stack of equal-shaped 2-D maps")
            self.grids = np.ascontiguousarray(np.stack(maps))
        else:
            self.grids = np.ascontiguousarray(grid, np.uint8)[None]
        self.grid = self.grids[0]
        self.n_maps = len(self.grids)
        cfg, self._keep = _cabi.make_cfg(self.params)
        nbytes = self.lib.imgenv_arena_bytes(C.byref(cfg))
        if nbytes <= 0:
            raise ValueError("imgenv_arena_bytes rejected the configuration")
        with torch.cuda.device(self.device):
            self.arena = torch.zeros(int(nbytes), dtype=torch.uint8, device=self.device)
        cfg.out_arena = self.arena.data_ptr()
        cfg.out_arena_bytes = nbytes
        self.cfg = cfg
        h = C.c_void_p()
        rc = self.lib.imgenv_create(C.byref(cfg), self.grid.ctypes.data, self.grid.shape[0], self.grid.shape[1],
                                    C.byref(h))
        if rc != 0:
            raise ValueError("imgenv_create: %s" % self.lib.imgenv_last_error().decode())
        self.h = h
        self.n_robots, self.n_peds = cfg.n_robots, cfg.n_peds
        self.n_worlds = max(1, cfg.n_worlds)
        self._trace = [0.0, 0] if os.environ.get("IMGENV_TRACE_RESET") else None  # seconds inside imgenv_reset_worlds, calls
        self._finished_buf = None
        o = _cabi.Out()
        self._check(self.lib.imgenv_outputs(self.h, C.byref(o)), "imgenv_outputs")
        self.n_local = o.n_local
        self._out_header = o
        base = self.arena.data_ptr()
        self.out = {}
        for name, (dt, shape) in _cabi.out_layout(o, self.n_peds, cfg.ped_image_size[0], cfg.ped_image_size[1]).items():
            if not getattr(o, name):  # an optional output this handle does not produce
                continue
            off = getattr(o, name) - base
            n = int(np.prod(shape)) * np.dtype(dt).itemsize
            self.out[name] = self.arena[off:off + n].view(_torch_dtype(dt)).view(*shape)
        rec, bpr = C.c_void_p(), C.c_int64()
        self._check(self.lib.imgenv_records(self.h, C.byref(rec), C.byref(bpr)), "imgenv_records")
        off = rec.value - base
        n = self.n_robots * _cabi.RECORD_DOUBLES * 8
        # (output_guard "copy": the records stay in the library's private arena -- no tensor for them; such a handle is never a shard)
        self.records = (self.arena[off:off + n].view(torch.float64).view(self.n_robots, _cabi.RECORD_DOUBLES)
                        if 0 <= off and off + n <= int(nbytes) else None)
        self.robot_begin = cfg.robot_begin
        self.robot_end = cfg.robot_end if cfg.robot_end else cfg.n_robots
        self.stack = None  # enable_stack()
        self.stack_arena = None
        self.episodes = None  # enable_episodes()
        self.episode_log = None  # enable_episode_log()
        self.episode_log_capacity = 0
        self.action_outputs = None  # enable_actions()
        self.policy = None  # enable_policy()
        self.policy_loss_out = None  # enable_policy_loss()
        self.obs_post = None  # enable_obs_post()
        self.final_obs = None  # enable_final_obs()
        self.rollout = None  # enable_rollout()
        self.rollout_draws_ped_maps = False  # ... with "ped_maps_drawn"
        self.minibatch = None  # enable_minibatch()
        self.sequences = None  # enable_sequences()
        self.normalise = None  # enable_normalise()
        if self.n_maps > 1:
            rest = self.grids[1:]
            rc = self.lib.imgenv_maps_add(self.h, len(rest), rest.ctypes.data, rest.shape[1], rest.shape[2])
            if rc != 0:
                msg = self.lib.imgenv_last_error().decode()
                self.close()
                raise ValueError("imgenv_maps_add: %s" % msg)
        self._ids_buf = None  # world_maps() / world_tracks() / world_scenarios()
        self.n_track_sets = 0  # tracks_add()
        self.n_scenarios = 0  # scenarios_add()
        self.scenario_obstacles = 0

    def scenarios_add(self, layouts):
        """``imgenv_scenarios_add``: the handle's bank of recorded episodes (the reference's ``cfg_type: bag``), once, before the
        first ``step_autoreset_device``.  ``layouts``: a list of the layout objects ``spawn.native_spawn`` / ``EnvPos.reset`` /
        ``spawn.record_scenarios`` return, all of one cast (this handle's robots and pedestrians per world, the first episode's
        number of obstacles).  ValueError for refused input, RuntimeError for a call out of order."""
        layouts = list(layouts)
        if not layouts:
            raise ValueError("no scenarios")
        first = layouts[0]
        shape = first["obs_shape"] if isinstance(first, dict) else first.obs_shape
        R, P, O = self.n_robots // self.n_worlds, self.n_peds // self.n_worlds, int(len(shape))
        arrays = _cabi.pack_scenarios(layouts, R, P, O)
        rc = self.lib.imgenv_scenarios_add(self.h, len(layouts), O, *[a.ctypes.data for a in arrays.values()])
        self._call(rc, "imgenv_scenarios_add")
        self.n_scenarios, self.scenario_obstacles = len(layouts), O

    def scenarios_policy(self, name, first=0):
        """``imgenv_scenarios_policy``: what fills the device-side reset's pool from now on -- "off" (the sampler), "queue" (placement
        number k replays scenario ``(first + k) % n_scenarios``) or "placement" (``_cabi.scenario_for_placement`` of the placement's
        seed).  Ordered on the current stream, no synchronisation; the first reset behind the call already obeys it."""
        if name not in _cabi.SCENARIO_POLICIES:
            raise ValueError("scenario policy: off | queue | placement")
        self._call(self.lib.imgenv_scenarios_policy(self.h, _cabi.SCENARIO_POLICIES[name], C.c_uint64(int(first) & 0xFFFFFFFFFFFFFFFF),
                                                    self._stream()), "imgenv_scenarios_policy")

    def reset_worlds_scenarios(self, worlds, ids):
        """``imgenv_reset_worlds_scenarios``: world ``worlds[q]`` starts the bank's episode ``ids[q]`` (a host-side reset; the device's
        placement count does not move).  ValueError for an id or a world out of range."""
        self._world_ids_set("imgenv_reset_worlds_scenarios", "scenario", worlds, ids)
        return self.out

    def world_scenarios(self):
        """``imgenv_world_scenarios``: the scenario each world's current episode came from, -1 where its reset did not come from the
        bank (numpy int32 ``[n_worlds]``); synchronises the stream"""
        return self._world_ids("imgenv_world_scenarios")

    def tracks_add(self, sets):
        """``imgenv_tracks_add``: the handle's bank of recorded crowds (dataset scene), once, before the first reset.  ``sets``: a list
        of ``[P, T, 5]`` arrays (x, y, yaw, vx, vy per pedestrian and step; ``P`` = pedestrians per world) or ``(series, lengths)``
        pairs -- ``_cabi.pack_track_sets``.  From then on a reset whose layout carries no ``ped_traj_v`` takes the world's
        pedestrians from the bank.  ValueError for refused arguments, RuntimeError for a call out of order."""
        n, cap, pose, traj, traj_v, length = _cabi.pack_track_sets(sets, self.n_peds // self.n_worlds)
        rc = self.lib.imgenv_tracks_add(self.h, n, cap, pose.ctypes.data, traj.ctypes.data, traj_v.ctypes.data, length.ctypes.data)
        self._call(rc, "imgenv_tracks_add")
        self.n_track_sets = n

    def set_world_tracks(self, worlds, ids):
        """``imgenv_world_tracks_set``: world ``worlds[q]`` takes set ``ids[q]`` at its next bank-fed reset queued after this call
        (policy "keep"); its running episode is untouched.  ValueError (nothing applied) for an id or a world out of range or a
        world listed twice."""
        self._world_ids_set("imgenv_world_tracks_set", "set", worlds, ids)

    def tracks_policy(self, name, repeat=1):
        """``imgenv_tracks_policy``: "keep" (``set_world_tracks`` alone chooses), "placement" (``_cabi.tracks_for_placement(seed,
        n_sets)`` of the placement's seed, inside the device-side reset chain too) or "cycle" (a world's e-th bank-fed reset since
        this call takes set ``(e // repeat) % n_sets``: the reference wrapper's order, wrapping where it exits).  Waits for the device."""
        if name not in _cabi.TRACK_POLICIES:
            raise ValueError("track policy: keep | placement | cycle")
        self._call(self.lib.imgenv_tracks_policy(self.h, _cabi.TRACK_POLICIES[name], int(repeat)), "imgenv_tracks_policy")

    def world_tracks(self):
        """``imgenv_world_tracks``: the set each world's current episode replays, -1 where its last reset brought its own tracks
        (numpy int32 ``[n_worlds]``); synchronises the stream"""
        return self._world_ids("imgenv_world_tracks")

    def set_world_maps(self, worlds, ids):
        """``imgenv_world_maps_set``: world ``worlds[q]`` starts from map ``ids[q]`` of the bank at its next reset of any kind
        queued after this call; its current episode is untouched.  ValueError (nothing applied) for an id, a world out of range
        or a world listed twice."""
        self._world_ids_set("imgenv_world_maps_set", "map", worlds, ids)

    def world_maps(self):
        """``imgenv_world_maps``: the map each world's current episode runs on (numpy int32 ``[n_worlds]``); synchronises the stream"""
        return self._world_ids("imgenv_world_maps")

    def set_maps_policy(self, name):
        """``imgenv_maps_policy``: "keep" (``set_world_maps`` alone chooses) or "placement" (every reset that draws its placement
        from a seed draws the map with it, ``_cabi.map_for_placement(seed, n_maps)`` -- inside the device-side reset chain too)"""
        if name not in _cabi.MAP_POLICIES:
            raise ValueError("map policy: keep | placement")
        self._check(self.lib.imgenv_maps_policy(self.h, _cabi.MAP_POLICIES[name]), "imgenv_maps_policy")

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, self.lib.imgenv_last_error().decode()))

    def _call(self, rc, what, value_codes=(_cabi.EINVAL,)):
        """the return code of an enable or decode entry point: ValueError for a refused argument, RuntimeError otherwise"""
        if rc in value_codes:
            raise ValueError("%s: %s" % (what, self.lib.imgenv_last_error().decode()))
        self._check(rc, what)

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _world_ids_set(self, entry, what, worlds, ids):
        """an entry point that takes a (world, id) list -- the banks' ``*_set`` calls, ``imgenv_reset_worlds_scenarios``: ValueError
        for a refused list, RuntimeError otherwise"""
        worlds, ids = [int(k) for k in worlds], [int(k) for k in ids]
        if len(worlds) != len(ids):
            raise ValueError("one %s id per world" % what)
        n = len(worlds)
        self._call(getattr(self.lib, entry)(self.h, n, (C.c_int32 * max(n, 1))(*worlds), (C.c_int32 * max(n, 1))(*ids), self._stream()), entry)

    def _world_ids(self, entry):
        """a bank's getter: what each world's current episode runs on, numpy int32 ``[n_worlds]``"""
        if self._ids_buf is None:
            self._ids_buf = (C.c_int32 * self.n_worlds)()
        self._check(getattr(self.lib, entry)(self.h, self._ids_buf, self._stream()), entry)
        return np.array(self._ids_buf[:], np.int32)

    def enable_stack(self, image_batch, state_batch, laser_batch):
        """Device-side StateBatchWrapper (``imgenv_stack_enable``; once, before the first reset): from now on every reset / step
        also keeps ``self.stack`` -- zero-copy tensors ``sensor_maps`` float16 ``[R, Ki, H, W]``, ``vector_states`` float32
        ``[R, Ks * state_dim]``, ``lasers`` float64 ``[R, Kl, B]`` holding each robot's last K frames of the current episode,
        oldest first, zero-padded after a reset.  Depths are the YAML keys (``image_batch`` / ``state_batch`` 0 = not stacked,
        ``laser_batch`` < 0 = not stacked, 0 = depth 1); a field that is not stacked has no key.  torch owns the memory, as it
        owns the output arena; a field of depth 1 is a view of ``self.out``'s tensor.  Read-only, like ``out``."""
        import torch
        s = _cabi.make_stack_cfg(image_batch, state_batch, laser_batch)
        nbytes = self.lib.imgenv_stack_bytes(C.byref(self.cfg), C.byref(s))
        if nbytes < 0:
            raise ValueError("imgenv_stack_bytes: %s" % self.lib.imgenv_last_error().decode())
        if nbytes > 0:
            with torch.cuda.device(self.device):
                self.stack_arena = torch.zeros(int(nbytes), dtype=torch.uint8, device=self.device)
            torch.cuda.current_stream(self.device).synchronize()  # (the library's kernels may run on any stream)
            s.arena, s.arena_bytes = self.stack_arena.data_ptr(), int(nbytes)
        so = _cabi.StackOut()
        # (only a call out of order is a RuntimeError here)
        self._call(self.lib.imgenv_stack_enable(self.h, C.byref(s), C.byref(so)), "imgenv_stack_enable",
                   value_codes=(_cabi.EINVAL, _cabi.ENOMEM, _cabi.EDEVICE))
        R, o = self.n_local, self.out
        H, Wd = o["sensor_maps"].shape[1:]
        shapes = {"sensor_maps": (so.image_depth, torch.float16, (R, so.image_depth, H, Wd)),
                  "vector_states": (so.state_depth, torch.float32, (R, so.state_depth * o["vector_states"].shape[1])),
                  "lasers": (so.laser_depth, torch.float64, (R, so.laser_depth, o["lasers"].shape[1]))}
        self.stack = {}
        for name, (depth, dt, shape) in shapes.items():
            ptr = getattr(so, name)
            if depth == 0 or not ptr:
                continue
            if depth == 1:  # the library handed out the imgenv_out array itself
                assert ptr == o[name].data_ptr()
                self.stack[name] = o[name].view(*shape)
                continue
            off = ptr - self.stack_arena.data_ptr()
            n = int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size()
            self.stack[name] = self.stack_arena[off:off + n].view(dt).view(*shape)
        self.stack_depths = (so.image_depth, so.state_depth, so.laser_depth)
        return self.stack

    def enable_episodes(self, min_steps=3, dt=None):
        """Device-side TestEpisodeWrapper (``imgenv_episodes_enable``): from now on every step takes each local robot's command,
        reward and ``is_clean`` into its open episode and every reset folds the episodes of the robots it covers into per-robot
        totals (include/imgenv.h).  ``self.episodes`` maps the names of ``imgenv_episodes_out`` to zero-copy tensors over the
        library's own memory: int32 / float64 ``[R]``, or ``[rows, R]`` for ``ends`` (``_cabi.EP_ENDS``), ``figure_sums``
        (``_cabi.EP_FIGURE_NAMES``) and ``open_f64`` (``_cabi.EP_OPEN_NAMES``).  Read-only; valid until ``close()``.  ``dt`` is the
        YAML's ``control_hz`` (default: the handle's step time); ValueError for a bad cfg or a second call with another one."""
        c = _cabi.make_episodes_cfg(min_steps, self.cfg.step_hz if dt is None else dt)
        eo = _cabi.EpisodesOut()
        self._call(self.lib.imgenv_episodes_enable(self.h, C.byref(c), C.byref(eo)), "imgenv_episodes_enable")
        if self.episodes is None:
            R = eo.n_local
            self.episodes = self._views(eo, {k: (dt_, (rows, R) if rows else (R,)) for k, (dt_, rows) in _cabi.EPISODE_ARRAYS.items()},
                                        "imgenv_episodes_out")
        return self.episodes

    def clear_episodes(self):
        """``imgenv_episodes_clear``: totals, ``last_*`` and the open episodes' sums back to zero, ordered on the current stream"""
        self._check(self.lib.imgenv_episodes_clear(self.h, self._stream()), "imgenv_episodes_clear")

    def enable_episode_log(self, capacity):
        """Device-side episode log (``imgenv_episode_log_enable``; after ``enable_episodes``): from now on every reset chain appends
        one record per episode it closes to a ring of ``capacity`` records, tagged with the map, track set, scenario and placement
        the episode ran on (include/imgenv.h).  ``self.episode_log`` maps ``n_written`` (int64 ``[1]``), ``i32`` (int32
        ``[10, capacity]``, rows ``_cabi.EPLOG_I32_NAMES``), ``f64`` (float64 ``[9, capacity]``, rows ``_cabi.EPLOG_F64_NAMES``) and
        ``placement`` (int64 ``[capacity]``, -1: none) to zero-copy tensors over the library's memory; record ``q`` lives in slot
        ``q % capacity``.  Read-only; valid until ``close()``.  ValueError for a bad capacity or a second call with another one,
        RuntimeError before ``enable_episodes``."""
        c = _cabi.make_episode_log_cfg(capacity)
        lo = _cabi.EpisodeLogOut()
        self._call(self.lib.imgenv_episode_log_enable(self.h, C.byref(c), C.byref(lo)), "imgenv_episode_log_enable")
        if self.episode_log is None:
            n = lo.capacity
            self.episode_log = self._views(lo, {k: (dt_, (1,) if rows < 0 else ((rows, n) if rows else (n,)))
                                                for k, (dt_, rows) in _cabi.EPISODE_LOG_ARRAYS.items()}, "imgenv_episode_log_out")
            self.episode_log_capacity = n
        return self.episode_log

    def read_episode_log(self, first=0, max_records=None):
        """``imgenv_episode_log_read``: ``(records, oldest, n_written)`` -- the records with ``seq`` in ``[max(first, oldest),
        min(first + max_records, n_written))`` (``max_records=None``: up to ``n_written``, so a ``first`` the ring has overwritten starts at
        ``oldest``) as a numpy record array (``_cabi.EPISODE_RECORD_DTYPE``; ``scenario`` resolved as
        ``world_scenarios()`` would have answered while the episode ran).  SYNCHRONISES the current stream."""
        if self.episode_log is None:
            raise RuntimeError("enable_episode_log() was not called")
        # (whatever the window, the library copies records of [oldest, n_written) only: never more than the ring holds)
        n = 0x7FFFFFFF if max_records is None else max(0, min(int(max_records), 0x7FFFFFFF))
        rec = np.zeros(max(min(n, self.episode_log_capacity), 1), _cabi.EPISODE_RECORD_DTYPE)
        oldest, written = C.c_uint64(), C.c_uint64()
        got = self.lib.imgenv_episode_log_read(self.h, C.c_uint64(int(first)), n, rec.ctypes.data, C.byref(oldest), C.byref(written), self._stream())
        if got < 0:
            self._check(int(got), "imgenv_episode_log_read")
        return rec[:int(got)], int(oldest.value), int(written.value)

    def _views(self, out, arrays, what):
        """zero-copy tensors over library-owned arrays: ``arrays`` maps a name of ``out`` to (numpy dtype, shape)"""
        import torch
        views = {}
        for name, (dt_, shape) in arrays.items():
            ptr = getattr(out, name)
            if not ptr:
                continue
            with torch.cuda.device(self.device):
                t = torch.as_tensor(_DeviceArray(ptr, shape, np.dtype(dt_).str), device=self.device)
            if t.data_ptr() != ptr or t.dtype != _torch_dtype(dt_):
                raise RuntimeError("%s.%s: torch made a copy instead of a view" % (what, name))
            views[name] = t
        return views

    def enable_actions(self, discrete_actions=None, continuous_actions=None, act_dim=2):
        """Device-side VelActionWrapper (``imgenv_actions_enable``): ``discrete_actions`` -- the YAML's table, rows of (v, w) or
        (v, w, beep) -- selects TABLE mode, ``continuous_actions`` -- its (lo, hi) per column -- CLIP mode; ``act_dim`` (2 or 3) is
        the width of a float input row.  ``self.action_outputs`` maps ``actions`` float32 ``[R, 3]``, ``speeds`` float32 ``[R, 2]``
        and ``n_bad`` int32 ``[1]`` to zero-copy tensors over the library's memory, filled by ``decode_actions``.  Read-only; valid
        until ``close()``.  ValueError for a bad cfg or a second call with another one."""
        if (discrete_actions is None) == (continuous_actions is None):
            raise ValueError("enable_actions: discrete_actions (a table) or continuous_actions (clip ranges)")
        c, keep = _cabi.make_actions_cfg(table=discrete_actions, clip=continuous_actions, n_cols=act_dim)
        ao = _cabi.ActionsOut()
        self._call(self.lib.imgenv_actions_enable(self.h, C.byref(c), C.byref(ao)), "imgenv_actions_enable")
        if self.action_outputs is None:
            R = ao.n_local
            self.action_outputs = self._views(ao, {k: (dt, (R, n) if n else (1,)) for k, (dt, n) in _cabi.ACTION_ARRAYS.items()},
                                              "imgenv_actions_out")
            self._act_cols, self._act_table = int(act_dim), discrete_actions is not None
        return self.action_outputs

    def decode_actions(self, raw):
        """``imgenv_actions_decode``: what the policy emitted -- a torch tensor or numpy array of int32 / int64 indices ``[R]``
        (TABLE mode) or float32 / float64 rows ``[R, act_dim]``, kept in its dtype; host data is copied to the device first --
        becomes ``action_outputs["actions"]``, which is returned and goes to any step call on the same stream.  One launch,
        ordered on the current stream; also rewrites ``speeds`` and adds the rows it zeroed to ``n_bad``."""
        import torch
        if self.action_outputs is None:
            raise RuntimeError("decode_actions failed (%d): enable_actions was not called" % _cabi.ESTATE)
        if not isinstance(raw, torch.Tensor):
            raw = np.ascontiguousarray(raw)
            if raw.dtype not in _cabi.RAW_DTYPES:
                raw = raw.astype(np.int64 if raw.dtype.kind in "iub" else np.float64 if raw.dtype.itemsize > 4 else np.float32)
            raw = torch.as_tensor(raw, device=self.device)
        if raw.device != self.device or not raw.is_contiguous():
            raw = raw.to(device=self.device).contiguous()
        code = {torch.int32: _cabi.RAW_I32, torch.int64: _cabi.RAW_I64, torch.float32: _cabi.RAW_F32, torch.float64: _cabi.RAW_F64}.get(raw.dtype)
        if code is None:
            raise ValueError("decode_actions: int32 / int64 indices or float32 / float64 rows, not %s" % raw.dtype)
        integer = code in (_cabi.RAW_I32, _cabi.RAW_I64)
        if raw.numel() != self.n_local * (1 if integer else self._act_cols):
            raise ValueError("decode_actions: %s" % ("one index per robot, [%d]" % self.n_local if integer else
                                                     "[%d, %d] floats" % (self.n_local, self._act_cols)))
        # (kept until the next decode: the launch reads it in stream order, a tensor made here from host data must outlive it)
        self._raw_actions = raw
        self._call(self.lib.imgenv_actions_decode(self.h, C.c_void_p(raw.data_ptr()), code, self._stream()), "imgenv_actions_decode")
        return self.action_outputs["actions"]

    def enable_policy(self, kind, seed=0, store=False):
        """The policy head (``imgenv_policy_enable``; needs ``enable_actions`` first -- a table for ``"categorical"``, clip ranges
        for ``"gaussian"`` -- and, with ``store``, ``enable_rollout``).  ``self.policy`` maps ``index`` int32 ``[R]`` (categorical)
        or ``raw`` float32 ``[R, C]`` (Gaussian), ``logp`` and ``entropy`` float32 ``[R]`` and, with ``store``, ``pol_raw`` float32
        ``[C', T, R]``, ``pol_logp`` ``[T, R]`` and ``pol_value`` ``[T + 1, R]`` to zero-copy tensors over the library's memory,
        filled by ``policy_sample``.  Read-only; valid until ``close()``.  ValueError for a refused cfg or a second call with
        another one, RuntimeError before ``enable_actions`` / ``enable_rollout``."""
        c = _cabi.make_policy_cfg(kind, seed, store)
        po = _cabi.PolicyOut()
        self._call(self.lib.imgenv_policy_enable(self.h, C.byref(c), C.byref(po)), "imgenv_policy_enable")
        if self.policy is None:
            R, n, T = po.n_local, po.n_params, po.horizon
            cat = c.kind == _cabi.POLICY_CATEGORICAL
            arrays = dict(index=(np.int32, (R,)), raw=(np.float32, (R, n)), logp=(np.float32, (R,)), entropy=(np.float32, (R,)),
                          pol_raw=(np.float32, (1 if cat else n, T, R)), pol_logp=(np.float32, (T, R)), pol_value=(np.float32, (T + 1, R)))
            self.policy = self._views(po, arrays, "imgenv_policy_out")
            self._pol_cat, self._pol_params, self._pol_store = cat, n, bool(store)
            self._pol_keep = None
        return self.policy

    def _pol_tensor(self, t, shapes, what, who="policy_sample"):
        import torch
        if t is None:
            return None
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.ascontiguousarray(t, np.float32), device=self.device)
        if t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
            t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(t.shape) not in shapes:
            raise ValueError("%s: %s float32 %s" % (who, what, " or ".join(str(list(s)) for s in shapes)))
        return t

    def policy_sample(self, params, log_std=None, values=None, draw=0, deterministic=False, store=True):
        """``imgenv_policy_sample``: ``params`` -- logits float32 ``[R, A]`` or means ``[R, C]`` -- with ``log_std`` float32 ``[C]``
        or ``[R, C]`` (Gaussian) and ``values`` float32 ``[R]`` or None become the sampled action (``deterministic``: the mode) of
        draw number ``draw`` in ``self.policy`` and its decoded rows in ``action_outputs``; ``action_outputs["actions"]`` is
        returned and goes to any step call on the same stream.  One launch, ordered on the current stream.  With a storing head
        the call also writes the rollout window's slot unless ``store`` is False."""
        if self.policy is None:
            raise RuntimeError("policy_sample failed (%d): enable_policy was not called" % _cabi.ESTATE)
        R, n = self.n_local, self._pol_params
        a = _cabi.PolicyArgs()
        a.struct_size = C.sizeof(_cabi.PolicyArgs)
        params = self._pol_tensor(params, [(R, n)], "logits" if self._pol_cat else "mean")
        values = self._pol_tensor(values, [(R,)], "values")
        if params is None:
            raise ValueError("policy_sample: %s is missing" % ("logits" if self._pol_cat else "mean"))
        a.flags = (_cabi.POLICY_DETERMINISTIC if deterministic else 0) | (0 if store or not self._pol_store else _cabi.POLICY_NO_STORE)
        if not self._pol_cat:
            log_std = self._pol_tensor(log_std, [(n,), (R, n)], "log_std")
            if log_std is None:
                raise ValueError("policy_sample: log_std is missing")
            if log_std.dim() == 2:
                a.flags |= _cabi.POLICY_LOG_STD_PER_ROW
            a.log_std = log_std.data_ptr()
        a.draw = int(draw) & 0xFFFFFFFFFFFFFFFF
        a.params = params.data_ptr()
        a.values = values.data_ptr() if values is not None else None
        # (kept until the next sample: the launch reads them in stream order, a tensor made here from host data must outlive it)
        self._pol_keep = (params, log_std, values)
        self._call(self.lib.imgenv_policy_sample(self.h, C.byref(a), self._stream()), "imgenv_policy_sample")
        return self.action_outputs["actions"]

    def policy_value(self, values):
        """the ``IMGENV_POLICY_VALUE_ONLY`` call: ``values`` float32 ``[R]`` into ``policy["pol_value"][n]``, n the rollout
        cursor -- the bootstrap value where n is T"""
        if self.policy is None:
            raise RuntimeError("policy_value failed (%d): enable_policy was not called" % _cabi.ESTATE)
        a = _cabi.PolicyArgs()
        a.struct_size = C.sizeof(_cabi.PolicyArgs)
        values = self._pol_tensor(values, [(self.n_local,)], "values")
        a.flags = _cabi.POLICY_VALUE_ONLY
        a.values = values.data_ptr() if values is not None else None
        self._pol_value_keep = values
        self._call(self.lib.imgenv_policy_sample(self.h, C.byref(a), self._stream()), "imgenv_policy_sample")

    def enable_policy_loss(self, max_rows):
        """PPO's loss on the device (``imgenv_policy_loss_enable``; needs ``enable_policy`` first, not the rollout):
        ``self.policy_loss_out`` maps ``logp``, ``entropy``, ``ratio``, ``pg``, ``vl`` and ``d_values`` float32 ``[max_rows]``,
        ``d_params`` float32 ``[max_rows * n]`` (row i of a call at ``i * n``, n = A or C: ``policy_loss`` returns the call's
        ``[rows, n]`` view), for a Gaussian head ``d_log_std`` likewise and ``d_log_std_shared`` ``[C]``, ``stats`` float32 ``[8]``
        (``_cabi.PLOSS_STATS``), ``n_bad`` int32 ``[1]`` and ``inv_w`` float32 ``[1]`` to zero-copy tensors over the library's memory,
        filled by ``policy_loss``.  Read-only; valid until ``close()``.  ValueError for a refused cfg or a second call with another
        ``max_rows``, RuntimeError before ``enable_policy``."""
        c = _cabi.make_policy_loss_cfg(max_rows)
        lo = _cabi.PolicyLossOut()
        self._call(self.lib.imgenv_policy_loss_enable(self.h, C.byref(c), C.byref(lo)), "imgenv_policy_loss_enable")
        if self.policy_loss_out is None:
            B, n = lo.max_rows, lo.n_params
            arrays = {k: (np.float32, (B,)) for k in ("logp", "entropy", "ratio", "pg", "vl", "d_values")}
            arrays.update(d_params=(np.float32, (B * n,)), d_log_std=(np.float32, (B * n,)), d_log_std_shared=(np.float32, (n,)),
                          stats=(np.float32, (8,)), n_bad=(np.int32, (1,)), inv_w=(np.float32, (1,)))
            self.policy_loss_out = self._views(lo, arrays, "imgenv_policy_loss_out")
            self._ploss_rows = B
            self._ploss_keep = None
            self.policy_loss_serial = 0  # calls queued so far: a holder of the outputs' views can tell whether they are still its call's
        return self.policy_loss_out

    def policy_loss(self, params, values, action, old_logp, adv, ret, weight, log_std=None, old_value=None, clip=0.2, clip_vf=None,
                    vf_coef=0.5, ent_coef=0.0):
        """``imgenv_policy_loss``: the network's new outputs ``params`` -- logits float32 ``[B, A]`` or means ``[B, C]`` with
        ``log_std`` ``[C]`` or ``[B, C]`` -- and ``values`` ``[B]`` against the stored ``action`` (the index as float32 ``[B]``, or
        a sequence of the C raw columns ``[B]`` each), ``old_logp``, ``adv``, ``ret`` and ``weight`` ``[B]``; ``clip_vf`` (with
        ``old_value`` ``[B]``) selects the clipped value loss.  Three launches, ordered on the current stream; nothing
        synchronises.  Returns the call's views of ``policy_loss_out``: the row arrays cut to ``[B]``, ``d_params`` (and
        ``d_log_std``) as ``[B, n]``, rewritten by the next call (``policy_loss_serial`` counts the calls queued)."""
        import torch
        if self.policy_loss_out is None:
            raise RuntimeError("policy_loss failed (%d): enable_policy_loss was not called" % _cabi.ESTATE)
        n, cat = self._pol_params, self._pol_cat
        if not isinstance(params, torch.Tensor):
            params = torch.as_tensor(np.ascontiguousarray(params, np.float32), device=self.device)
        if params.dim() != 2 or params.shape[1] != n or not 1 <= params.shape[0] <= self._ploss_rows:
            raise ValueError("policy_loss: %s float32 [B, %d] with B in 1 .. %d" % ("logits" if cat else "mean", n, self._ploss_rows))
        B = int(params.shape[0])
        cols = [action] if cat else list(action)
        if len(cols) != (1 if cat else n):
            raise ValueError("policy_loss: action is %s" % ("the index, float32 [B]" if cat else "%d raw columns, float32 [B] each" % n))
        a = _cabi.PolicyLossArgs()
        a.struct_size = C.sizeof(_cabi.PolicyLossArgs)
        a.rows = B
        params = self._pol_tensor(params, [(B, n)], "params", "policy_loss")
        keep = [params]
        for name, t in (("values", values), ("old_logp", old_logp), ("adv", adv), ("ret", ret), ("weight", weight)):
            t = self._pol_tensor(t, [(B,)], name, "policy_loss")
            if t is None:
                raise ValueError("policy_loss: %s is missing" % name)
            setattr(a, name, t.data_ptr())
            keep.append(t)
        for q, t in enumerate(cols):
            t = self._pol_tensor(t, [(B,)], "action", "policy_loss")
            if t is None:
                raise ValueError("policy_loss: action is missing")
            a.action[q] = t.data_ptr()
            keep.append(t)
        a.params = params.data_ptr()
        if not cat:
            log_std = self._pol_tensor(log_std, [(n,), (B, n)], "log_std", "policy_loss")
            if log_std is None:
                raise ValueError("policy_loss: log_std is missing")
            if log_std.dim() == 2:
                a.flags |= _cabi.POLICY_LOG_STD_PER_ROW
            a.log_std = log_std.data_ptr()
            keep.append(log_std)
        if clip_vf is not None:
            old_value = self._pol_tensor(old_value, [(B,)], "old_value", "policy_loss")
            if old_value is None:
                raise ValueError("policy_loss: clip_vf needs old_value")
            a.flags |= _cabi.PLOSS_CLIP_VALUE
            a.old_value = old_value.data_ptr()
            a.clip_vf = float(clip_vf)
            keep.append(old_value)
        a.clip, a.vf_coef, a.ent_coef = float(clip), float(vf_coef), float(ent_coef)
        # (kept until the next call: the launches read them in stream order, a tensor made here from host data must outlive them)
        self._ploss_keep = keep
        self._call(self.lib.imgenv_policy_loss(self.h, C.byref(a), self._stream()), "imgenv_policy_loss")
        self.policy_loss_serial += 1  # (behind every refusal: a refused call rewrites nothing)
        out = {}
        for k, t in self.policy_loss_out.items():
            if k in ("d_params", "d_log_std"):
                out[k] = t[:B * n].view(B, n)
            elif k in ("logp", "entropy", "ratio", "pg", "vl", "d_values"):
                out[k] = t[:B]
            else:
                out[k] = t
        return out

    def enable_obs_post(self, ped_norm=True, close=None, avg=_cabi.PED_NORM_AVG, std=_cabi.PED_NORM_STD, close_dist=_cabi.CLOSE_DIST):
        """Device-side StatePedVectorWrapper and ``bool_get_close_to_human`` (``imgenv_obs_post_enable``): from now on every reset /
        step also keeps ``self.obs_post`` -- ``ped_vector_norm`` float32 ``[R, 1 + 7 max_ped]`` (``ped_norm``) and
        ``close_to_human`` uint8 ``[R]`` (``close``; None = where the handle has pedestrians) -- as zero-copy tensors over the
        library's memory.  ``out["ped_vector_states"]`` stays the raw vector.  Defaults are the reference's constants."""
        if close is None:
            close = self.n_peds > 0
        c = _cabi.make_obs_post_cfg(ped_norm, close, avg, std, close_dist)
        po = _cabi.ObsPostOut()
        self._call(self.lib.imgenv_obs_post_enable(self.h, C.byref(c), C.byref(po)), "imgenv_obs_post_enable")
        if self.obs_post is None:
            R = po.n_local
            self.obs_post = self._views(po, {"ped_vector_norm": (np.float32, (R, self.out["ped_vector_states"].shape[1])),
                                             "close_to_human": (np.uint8, (R,))}, "imgenv_obs_post_out")
        return self.obs_post

    def enable_normalise(self, obs=True, reward=True, gamma=0.99, clip_obs=10.0, clip_reward=10.0, eps=1e-8):
        """Running normalisation of ``vector_states`` and of the reward on the device (``imgenv_normalise_enable``; Stable-Baselines3's
        VecNormalize): from now on every chain also keeps ``self.normalise`` -- zero-copy tensors over the library's memory:
        ``norm_vector_states`` float32 ``[R, state_dim]`` and, after ``enable_stack`` with a state stack of depth >= 2,
        ``norm_state_stack`` float32 ``[R, K * state_dim]`` (``obs``); ``norm_rewards`` float64 ``[R]`` (``reward``); and the state
        itself, ``stats`` float64 ``[2, 4 + 2 state_dim]`` and ``returns`` float64 ``[2, R]``, whose current words
        ``normalise_words()`` names.  Frozen robots count for nothing; a reset chain's rows count with their first observation.
        At most two launches per chain; nothing synchronises.  Call it after ``enable_stack`` and before ``enable_final_obs`` /
        ``enable_rollout`` with the normalised fields.  ValueError for a refused cfg or a second call."""
        c = _cabi.make_normalise_cfg(obs, reward, gamma, clip_obs, clip_reward, eps)
        no = _cabi.NormaliseOut()
        self._call(self.lib.imgenv_normalise_enable(self.h, C.byref(c), C.byref(no)), "imgenv_normalise_enable")
        R, D, K = no.n_local, no.state_dim, no.state_depth
        self.normalise = self._views(no, {"norm_vector_states": (np.float32, (R, D)), "norm_state_stack": (np.float32, (R, K * D)),
                                          "norm_rewards": (np.float64, (R,)), "stats": (np.float64, (2, 4 + 2 * D)),
                                          "returns": (np.float64, (2, R))}, "imgenv_normalise_out")
        self._norm_dims = (D, K)
        return self.normalise

    def _need_normalise(self):
        if self.normalise is None:
            raise RuntimeError("enable_normalise() was not called")

    def _normalise_out(self):
        self._need_normalise()
        no = _cabi.NormaliseOut()
        self._check(self.lib.imgenv_normalise_outputs(self.h, C.byref(no)), "imgenv_normalise_outputs")
        return no

    def normalise_words(self):
        """``(stats_word, returns_word, training)``: which word of ``normalise["stats"]`` / ``["returns"]`` is current (host-side
        counts: nothing synchronises)"""
        no = self._normalise_out()
        return no.stats_word, no.returns_word, bool(no.training)

    def normalise_training(self, on):
        """``imgenv_normalise_training``: True -- the chains from now on update the statistics; False -- they only apply them"""
        self._need_normalise()
        self._check(self.lib.imgenv_normalise_training(self.h, 1 if on else 0, self._stream()), "imgenv_normalise_training")

    def normalise_stats(self):
        """``imgenv_normalise_stats_get``: a dict of ``obs_count``, ``obs_mean`` / ``obs_var`` float64 ``[state_dim]``, ``ret_count``,
        ``ret_mean``, ``ret_var`` and ``returns`` float64 ``[R]`` on the host, for a checkpoint.  SYNCHRONISES the device."""
        self._need_normalise()
        s, arrays = _cabi.make_normalise_stats(self._norm_dims[0], self.n_local)
        self._call(self.lib.imgenv_normalise_stats_get(self.h, C.byref(s)), "imgenv_normalise_stats_get")
        return dict(arrays, obs_count=s.obs_count, ret_count=s.ret_count, ret_mean=s.ret_mean, ret_var=s.ret_var)

    def load_normalise_stats(self, stats):
        """``imgenv_normalise_stats_set``: what ``normalise_stats()`` returned (of this handle or of a trainer's) becomes what the
        next chain reads.  SYNCHRONISES the device.  ValueError for a refused value or another ``state_dim`` / ``R``."""
        self._need_normalise()
        s, arrays = _cabi.make_normalise_stats(self._norm_dims[0], self.n_local, stats)
        self._call(self.lib.imgenv_normalise_stats_set(self.h, C.byref(s)), "imgenv_normalise_stats_set")

    def enable_final_obs(self, fields=None):
        """Final observations (``imgenv_final_obs_enable``): from now on every reset -- ``reset``, ``reset_worlds*``,
        ``step_autoreset``, ``step_autoreset_device`` -- first copies the rows it is about to overwrite, for the robots it covers,
        into ``self.final_obs``: zero-copy tensors over the library's memory with the names, shapes and dtypes of ``out``'s, plus
        ``final_count`` int32 ``[R]`` (captures of the row so far).  ``fields``: names of ``_cabi.FINAL_BITS``; None = the
        ``ImageState`` set (without ``lasers`` on a handle without a laser).  ``"stacks"`` (after ``enable_stack``) adds
        ``stack_sensor_maps`` / ``stack_vector_states`` / ``stack_lasers`` for the stacks of depth >= 2, shaped as ``self.stack``'s;
        ``"ped_vector_norm"`` (after ``enable_obs_post``) the normalised pedestrian vector.  One extra launch per reset chain, none
        per step; nothing synchronises.  Read-only; valid until ``close()``.  ValueError for refused fields or a second call with
        other ones, RuntimeError for ``"stacks"`` / ``"ped_vector_norm"`` before their own enable call.  ``"norm_states"`` (after
        ``enable_normalise``, ValueError before it) adds ``norm_vector_states`` / ``norm_state_stack``."""
        if fields is None:
            fields = [n for n in list(_cabi.FINAL_BITS)[:9] if n != "lasers" or self.cfg.use_laser]
        c = _cabi.make_final_obs_cfg(fields)
        fo = _cabi.FinalObsOut()
        self._call(self.lib.imgenv_final_obs_enable(self.h, C.byref(c), C.byref(fo)), "imgenv_final_obs_enable")
        if self.final_obs is None:
            R = fo.n_local
            lay = _cabi.out_layout(self._out_header, self.n_peds, self.cfg.ped_image_size[0], self.cfg.ped_image_size[1])
            arrays = {name: lay[name] for name in list(_cabi.FINAL_BITS)[:11]}
            if self.stack:
                for name, t in self.stack.items():
                    arrays["stack_" + name] = (lay[name][0], tuple(t.shape))
            arrays["ped_vector_norm"] = lay["ped_vector_states"]
            arrays["final_count"] = (np.int32, (R,))  # (uint32 in the library; torch has no arithmetic on it)
            self.final_obs = self._views(fo, arrays, "imgenv_final_obs_out")
            if self.normalise is not None:  # "norm_states": the two fields' pointers are imgenv_normalise_out's
                extra = {"final_" + name: (np.float32, tuple(self.normalise[name].shape)) for name in _cabi.ROLLOUT_NORM_FIELDS
                         if name in self.normalise}
                for name, t in self._views(self._normalise_out(), extra, "imgenv_normalise_out").items():
                    self.final_obs[name[len("final_"):]] = t
        return self.final_obs

    def enable_rollout(self, horizon, final_capacity, fields=None):
        """Rollout storage (``imgenv_rollout_enable``): after ``rollout_begin()`` every step chain also stores its transition and
        the observation it led to, and every reset chain moves the rows it overwrites into a final list, in ``self.rollout``:
        zero-copy tensors over the library's memory -- ``obs_<field>`` ``[T + 1, R, ...]`` and ``final_<field>`` ``[F, ...]`` with
        the row shapes and dtypes of ``out`` / ``stack`` / ``obs_post``, ``actions`` float32 ``[T, R, 3]``, ``rewards`` float32,
        ``dones`` / ``is_clean`` uint8 and ``dones_info`` int32 ``[T, R]``, ``final_idx`` int32 ``[T + 1, R]``, ``final_slot`` /
        ``final_row`` int32 ``[F]`` and ``final_n`` int32 ``[2]`` (include/imgenv.h has the semantics).  ``fields``: names of
        ``_cabi.ROLLOUT_BITS`` (and ``"norm_states"``, ``"norm_rewards"``, ``"ped_maps_drawn"``, below); None = the five single-frame fields (without ``lasers`` on a handle without a laser).  One extra
        launch per chain; nothing synchronises.  Read-only; valid until ``close()``.  ValueError for a refused cfg or a second
        call with another one, RuntimeError for ``"stacks"`` / ``"ped_vector_norm"`` before their own enable call.  After
        ``enable_normalise``: ``"norm_states"`` stores ``norm_vector_states`` (and ``norm_state_stack``) like any field,
        ``"norm_rewards"`` makes ``rewards`` the normalised ones (ValueError before it).  ``"ped_maps_drawn"`` (with
        ``"ped_vector_states"``, without ``"ped_maps"``; ValueError otherwise): the ring keeps no ``obs_ped_maps`` / ``final_ped_maps``,
        the minibatches draw ``mb_ped_maps`` from the stored vectors, ``draw_ped_maps`` draws any slot."""
        if fields is None:
            fields = [n for n in list(_cabi.ROLLOUT_BITS)[:5] if n != "lasers" or self.cfg.use_laser]
        c = _cabi.make_rollout_cfg(horizon, final_capacity, fields)
        ro = _cabi.RolloutOut()
        self._call(self.lib.imgenv_rollout_enable(self.h, C.byref(c), C.byref(ro)), "imgenv_rollout_enable")
        if self.rollout is None:
            R, T, F = ro.n_local, ro.horizon, ro.final_capacity
            lay = _cabi.out_layout(self._out_header, self.n_peds, self.cfg.ped_image_size[0], self.cfg.ped_image_size[1])
            rows = {name: lay[name] for name in _cabi.ROLLOUT_FIELDS[:5]}
            rows["ped_vector_norm"] = lay["ped_vector_states"]
            for name, t in (self.stack or {}).items():
                rows["stack_" + name] = (lay[name][0], tuple(t.shape))
            arrays = {}
            for name, (dt, shape) in rows.items():  # (shape[0] is R)
                arrays["obs_" + name] = (dt, (T + 1,) + tuple(shape))
                arrays["final_" + name] = (dt, (F,) + tuple(shape[1:]))
            arrays.update(actions=(np.float32, (T, R, 3)), rewards=(np.float32, (T, R)), dones=(np.uint8, (T, R)), is_clean=(np.uint8, (T, R)),
                          dones_info=(np.int32, (T, R)), final_idx=(np.int32, (T + 1, R)), final_slot=(np.int32, (F,)),
                          final_row=(np.int32, (F,)), final_n=(np.int32, (2,)))  # (final_n: uint32 in the library)
            self.rollout = self._views(ro, arrays, "imgenv_rollout_out")
            if self.normalise is not None:  # "norm_states": the two fields' pointers are imgenv_normalise_out's
                no, extra = self._normalise_out(), {}
                for name in _cabi.ROLLOUT_NORM_FIELDS:
                    if name in self.normalise and getattr(no, "rollout_obs_" + name):
                        shape = tuple(self.normalise[name].shape)
                        rows[name] = (np.float32, shape)
                        extra["rollout_obs_" + name] = (np.float32, (T + 1,) + shape)
                        extra["rollout_final_" + name] = (np.float32, (F,) + shape[1:])
                for name, t in self._views(no, extra, "imgenv_normalise_out").items():
                    self.rollout[name[len("rollout_"):]] = t
            self.rollout_horizon, self.rollout_final_capacity = T, F
            self._rollout_rows = rows
            self.rollout_draws_ped_maps = bool(c.fields & _cabi.ROLLOUT_PED_MAPS_DRAWN)
        return self.rollout

    def rollout_cursor(self):
        """``(n, resets)``: the transitions and the reset chains stored since ``rollout_begin()`` (``n`` -1 before the first one);
        ``rollout["final_n"][resets & 1]`` is the number of final entries so far.  A host-side count: nothing synchronises."""
        if self.rollout is None:
            raise RuntimeError("enable_rollout() was not called")
        ro = _cabi.RolloutOut()
        self._check(self.lib.imgenv_rollout_outputs(self.h, C.byref(ro)), "imgenv_rollout_outputs")
        return ro.n, ro.resets

    def rollout_begin(self):
        """``imgenv_rollout_begin``: slot n becomes slot 0 (the first time: the live observation), ``final_idx`` -1, ``final_n``
        0 and the cursor 0, ordered on the current stream"""
        self._check(self.lib.imgenv_rollout_begin(self.h, self._stream()), "imgenv_rollout_begin")

    def rollout_gae(self, values, final_values=None, gamma=0.99, lam=0.95, adv=None, ret=None):
        """``imgenv_rollout_gae``: advantages and returns of the stored transitions, one launch on the current stream.  ``values``
        float32 ``[T + 1, R]`` and ``final_values`` float32 ``[F]`` or None are contiguous tensors on the handle's device.  Returns
        ``(adv, ret)`` float32 ``[T, R]`` (made with zeros unless given); rows ``t >= n`` are left as they are."""
        import torch
        if self.rollout is None:
            raise RuntimeError("enable_rollout() was not called")
        T, F, R = self.rollout_horizon, self.rollout_final_capacity, self.n_local

        def ok(t, shape):
            return isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == self.device and t.is_contiguous() and tuple(t.shape) == shape
        if not ok(values, (T + 1, R)) or (final_values is not None and not ok(final_values, (F,))):
            raise ValueError("rollout_gae: values float32 [%d, %d] and final_values float32 [%d] or None, contiguous on %s" % (T + 1, R, F, self.device))
        if adv is None:
            adv = torch.zeros((T, R), dtype=torch.float32, device=self.device)
        if ret is None:
            ret = torch.zeros((T, R), dtype=torch.float32, device=self.device)
        if not ok(adv, (T, R)) or not ok(ret, (T, R)):
            raise ValueError("rollout_gae: adv and ret float32 [%d, %d], contiguous on %s" % (T, R, self.device))
        fv = C.c_void_p(final_values.data_ptr()) if final_values is not None else None
        self._check(self.lib.imgenv_rollout_gae(self.h, C.c_void_p(values.data_ptr()), fv, float(gamma), float(lam),
                                                C.c_void_p(adv.data_ptr()), C.c_void_p(ret.data_ptr()), self._stream()), "imgenv_rollout_gae")
        return adv, ret

    def draw_ped_maps(self, ped_vectors, rows=None, out=None):
        """``imgenv_ped_maps_draw``: the pedestrian maps of pedestrian vectors, bit for bit what ``out["ped_maps"]`` showed beside
        them; one launch on the current stream, nothing synchronises.  ``ped_vectors`` float32 ``[m, ped_vec_len]``; ``rows`` int32
        ``[n]`` or None: map ``i`` is drawn from row ``rows[i]`` (below 0: all zeros), or from row ``i``; ``out`` float32
        ``[n, 3, Hp, Wp]`` (made unless given).  All contiguous tensors on the handle's device.  Returns ``out``."""
        import torch
        PV, (Hp, Wp) = self._out_header.ped_vec_len, self.cfg.ped_image_size

        def ok(t, dtype, shape):
            return (isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == self.device and t.is_contiguous() and t.dim() == len(shape)
                    and all(want is None or got == want for got, want in zip(t.shape, shape)))
        if not ok(ped_vectors, torch.float32, (None, PV)):
            raise ValueError("draw_ped_maps: ped_vectors float32 [m, %d], contiguous on %s" % (PV, self.device))
        if rows is not None and not ok(rows, torch.int32, (None,)):
            raise ValueError("draw_ped_maps: rows int32 [n] or None, contiguous on %s" % (self.device,))
        n = int(rows.shape[0] if rows is not None else ped_vectors.shape[0])
        if out is None:
            out = torch.empty((n, 3, Hp, Wp), dtype=torch.float32, device=self.device)
        if not ok(out, torch.float32, (n, 3, Hp, Wp)):
            raise ValueError("draw_ped_maps: out float32 [%d, 3, %d, %d], contiguous on %s" % (n, Hp, Wp, self.device))
        if n == 0:  # (an empty tensor has no address to hand over)
            return out
        rp = C.c_void_p(rows.data_ptr()) if rows is not None else None
        self._call(self.lib.imgenv_ped_maps_draw(self.h, C.c_void_p(ped_vectors.data_ptr()), rp, n, C.c_void_p(out.data_ptr()), self._stream()),
                   "imgenv_ped_maps_draw")
        return out

    def enable_minibatch(self, batch, buffers=1, fields=None):
        """Minibatches out of the rollout storage (``imgenv_rollout_minibatch_enable``; needs ``enable_rollout`` first):
        ``self.minibatch`` -- zero-copy tensors over the library's memory: ``mb_<field>`` ``[buffers, B, ...]`` with the row shapes
        and dtypes of ``rollout["obs_<field>"]``, ``mb_actions`` float32 ``[buffers, B, 3]``, ``mb_rewards`` / ``mb_weight`` float32,
        ``mb_dones`` uint8, ``mb_dones_info`` / ``mb_index`` int32 ``[buffers, B]``, ``mb_scalars`` float32 ``[buffers, 6, B]``
        (``t[b]`` is contiguous; the buffers of an array lie 256-byte aligned side by side), and ``valid`` / ``order`` int32
        ``[T * R]``, ``valid_n`` int32 ``[1]``, ``norm`` float32 ``[2]``.  ``fields``: the names ``enable_rollout``
        takes (``_cabi.ROLLOUT_BITS``' and ``"norm_states"``, ``"ped_maps_drawn"``), a subset of the rollout's; None = all of them
        (``"ped_maps_drawn"``: ``mb_ped_maps``, drawn by one more launch per minibatch).  Nothing is launched; read-only; valid until ``close()``.  ValueError for a refused
        cfg or a second call with another one, RuntimeError before ``enable_rollout``."""
        import torch
        c = _cabi.make_minibatch_cfg(batch, buffers, fields)
        mo = _cabi.MinibatchOut()
        self._call(self.lib.imgenv_rollout_minibatch_enable(self.h, C.byref(c), C.byref(mo)), "imgenv_rollout_minibatch_enable")
        if self.minibatch is None:
            B, NB, TR = mo.batch, mo.buffers, mo.horizon * mo.n_local
            views = self._views(mo, {"valid": (np.int32, (TR,)), "order": (np.int32, (TR,)), "valid_n": (np.int32, (1,)),  # (valid_n: uint32 in the library)
                                     "norm": (np.float32, (2,))}, "imgenv_minibatch_out")
            rows = {"mb_" + name: (self._rollout_rows[name][0], tuple(self._rollout_rows[name][1][1:]))
                    for name in _cabi.ROLLOUT_FIELDS if getattr(mo.buf[0], "mb_" + name)
                    and ("obs_" + name in (self.rollout or {}) or (name == "ped_maps" and self.rollout_draws_ped_maps))}
            norm_ptrs = {}  # the normalised fields' buffers: imgenv_normalise_out.mb_norm_*
            if self.normalise is not None:
                no = self._normalise_out()
                for name in _cabi.ROLLOUT_NORM_FIELDS:
                    if getattr(no, "mb_" + name)[0]:
                        rows["mb_" + name] = (np.float32, tuple(self._rollout_rows[name][1][1:]))
                        norm_ptrs["mb_" + name] = [getattr(no, "mb_" + name)[b] for b in range(NB)]
            rows.update(mb_actions=(np.float32, (3,)), mb_rewards=(np.float32, ()), mb_dones=(np.uint8, ()), mb_dones_info=(np.int32, ()),
                        mb_index=(np.int32, ()), mb_weight=(np.float32, ()))
            arrays = {name: (dt, (B,) + shape) for name, (dt, shape) in rows.items()}
            arrays["mb_scalars"] = (np.float32, (_cabi.MB_MAX_SCALARS, B))
            for name, (dt, shape) in arrays.items():
                # one view over the array's buffers: buffer b starts (size rounded up to 256 bytes) behind buffer b - 1
                item = np.dtype(dt).itemsize
                nbytes = int(np.prod(shape)) * item
                pitch = (nbytes + 255) // 256 * 256
                ptrs = norm_ptrs.get(name) or [getattr(mo.buf[b], name) for b in range(NB)]
                if any(ptrs[b] != ptrs[0] + b * pitch for b in range(NB)):
                    raise RuntimeError("imgenv_minibatch_out.%s: the buffers do not lie side by side" % name)
                first = types.SimpleNamespace(**{name: ptrs[0]}) if name in norm_ptrs else mo.buf[0]
                span = self._views(first, {name: (dt, ((NB - 1) * pitch // item + nbytes // item,))}, "imgenv_minibatch_buffer")[name]
                strides, acc = [], 1
                for d in reversed(shape):
                    strides.insert(0, acc)
                    acc *= d
                views[name] = torch.as_strided(span, (NB,) + tuple(shape), (pitch // item,) + tuple(strides))
            self.minibatch = views
            self.minibatch_batch, self.minibatch_buffers = B, NB
        return self.minibatch

    def _need_minibatch(self):
        if self.minibatch is None:
            raise RuntimeError("enable_minibatch() was not called")

    def rollout_index(self):
        """``imgenv_rollout_index``: ``minibatch["valid"]`` = the ascending list of the stored transitions ``k = t * R + row`` with
        ``is_clean != 0``, ``valid_n`` their count; three launches on the current stream, nothing synchronises.  A later step, reset
        or ``rollout_begin()`` makes the index stale: ``rollout_stats`` / ``_shuffle`` / ``_minibatch`` then raise RuntimeError."""
        self._need_minibatch()
        self._check(self.lib.imgenv_rollout_index(self.h, self._stream()), "imgenv_rollout_index")

    def rollout_valid_count(self):
        """``valid_n`` as a Python int.  SYNCHRONISES: it waits for the stream and reads one word from the device."""
        self._need_minibatch()
        return int(self.minibatch["valid_n"].item())

    def _mb_tensor(self, t, what, shapes):
        import torch
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == self.device and t.is_contiguous() and tuple(t.shape) in shapes):
            raise ValueError("%s: float32 %s, contiguous on %s" % (what, " or ".join(str(list(s)) for s in shapes), self.device))
        return C.c_void_p(t.data_ptr())

    def rollout_stats(self, x, eps=1e-8, out=None):
        """``imgenv_rollout_stats``: ``(mean, 1 / sqrt(var + eps))`` of ``x`` float32 ``[T, R]`` over the valid list, accumulated in
        float64 in a fixed order (two calls give identical bits); ``var`` is the POPULATION variance (divisor V, not torch.std's
        V - 1).  Into ``out`` float32 ``[2]`` or, None, ``minibatch["norm"]``; returns that tensor.  Four launches."""
        self._need_minibatch()
        T, R = self.rollout_horizon, self.n_local
        xp = self._mb_tensor(x, "rollout_stats: x", [(T, R)])
        op = self._mb_tensor(out, "rollout_stats: out", [(2,)]) if out is not None else None
        self._call(self.lib.imgenv_rollout_stats(self.h, xp, float(eps), op, self._stream()), "imgenv_rollout_stats")
        return out if out is not None else self.minibatch["norm"]

    def rollout_shuffle(self, seed):
        """``imgenv_rollout_shuffle``: ``minibatch["order"]`` = the valid list in a fresh order drawn from the 64-bit ``seed`` (a
        keyed bijection evaluated per position: include/imgenv.h), -1 behind ``valid_n``; one launch"""
        self._need_minibatch()
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._check(self.lib.imgenv_rollout_shuffle(self.h, seed & 0xFFFFFFFF, seed >> 32, self._stream()), "imgenv_rollout_shuffle")

    def rollout_minibatch(self, j, buffer=0, scalars=(), normalise=None, norm=None):
        """``imgenv_rollout_minibatch``: minibatch ``j`` of the current order into buffer ``buffer``, one launch.  ``scalars``: up
        to 6 float32 tensors ``[T, R]`` or ``[T + 1, R]``, contiguous on the handle's device, gathered into
        ``minibatch["mb_scalars"][buffer, s]``; ``normalise``: an index into them whose values become ``(x - norm[0]) * norm[1]``,
        ``norm`` float32 ``[2]`` or None for ``minibatch["norm"]``.  Slots behind the valid list are zeros with ``mb_index`` -1
        and ``mb_weight`` 0.  Returns the dict of buffer ``buffer``'s views."""
        self._need_minibatch()
        T, R = self.rollout_horizon, self.n_local
        scalars = list(scalars)
        if len(scalars) > _cabi.MB_MAX_SCALARS:
            raise ValueError("rollout_minibatch: at most %d scalars" % _cabi.MB_MAX_SCALARS)
        ptrs = [self._mb_tensor(t, "rollout_minibatch: scalars[%d]" % s, [(T, R), (T + 1, R)]).value for s, t in enumerate(scalars)]
        np_ = self._mb_tensor(norm, "rollout_minibatch: norm", [(2,)]).value if norm is not None else None
        a = _cabi.make_minibatch_args(j, buffer, ptrs, -1 if normalise is None else normalise, np_)
        self._call(self.lib.imgenv_rollout_minibatch(self.h, C.byref(a), self._stream()), "imgenv_rollout_minibatch")
        return {name: t[buffer] for name, t in self.minibatch.items() if name.startswith("mb_")}

    def _side_by_side(self, name, ptrs, dt, shape, what):
        """one ``[len(ptrs)] + shape`` view over an array's buffers: buffer b starts (size rounded up to 256 bytes) behind buffer b - 1"""
        import torch
        NB, item = len(ptrs), np.dtype(dt).itemsize
        nbytes = int(np.prod(shape)) * item
        pitch = (nbytes + 255) // 256 * 256
        if any(ptrs[b] != ptrs[0] + b * pitch for b in range(NB)):
            raise RuntimeError("%s.%s: the buffers do not lie side by side" % (what, name))
        first = types.SimpleNamespace(**{name: ptrs[0]})
        span = self._views(first, {name: (dt, ((NB - 1) * pitch // item + nbytes // item,))}, what)[name]
        strides, acc = [], 1
        for d in reversed(shape):
            strides.insert(0, acc)
            acc *= d
        return torch.as_strided(span, (NB,) + tuple(shape), (pitch // item,) + tuple(strides))

    def enable_sequences(self, length, batch, buffers=1, fields=None, state_bytes=()):
        """Sequence minibatches for recurrent policies out of the rollout storage (``imgenv_rollout_seq_enable``; needs
        ``enable_rollout`` first, not ``enable_minibatch``): the window cut into chunks of ``length`` steps per row, sequence ``q = c *
        R + row``.  ``self.sequences`` -- zero-copy tensors over the library's memory, TIME-MAJOR: ``mb_<field>`` ``[buffers, L, Bs,
        ...]`` with the row shapes and dtypes of ``rollout["obs_<field>"]``, ``mb_actions`` float32 ``[buffers, L, Bs, 3]``,
        ``mb_rewards`` / ``mb_weight`` float32, ``mb_dones`` / ``mb_first`` uint8, ``mb_dones_info`` / ``mb_index`` int32 ``[buffers, L,
        Bs]``, ``mb_scalars`` float32 ``[buffers, 6, L, Bs]``, ``mb_seq`` / ``mb_seq_len`` int32 ``[buffers, Bs]``, ``mb_seq_state0`` /
        ``mb_seq_state1`` uint8 ``[buffers, Bs, state_bytes[a]]`` (``.view(dtype)`` them), and ``seq_flag`` uint8, ``seq_valid`` /
        ``seq_order`` int32 ``[C_max * R]``, ``seq_valid_n`` int32 ``[1]``.  ``mb_first``: a reset rewrote that step's observation, the
        row's episode starts there (it does not say whether slot 0 continues the previous window).  ``fields`` as ``enable_minibatch``
        takes them; ``state_bytes``: the row sizes of up to 2 state arrays (LSTM h and c), multiples of 4.  Nothing is launched;
        read-only; valid until ``close()``.  ValueError for a refused cfg or a second call with another one, RuntimeError before
        ``enable_rollout``."""
        c = _cabi.make_seq_cfg(length, batch, buffers, fields, state_bytes)
        so = _cabi.SeqOut()
        self._call(self.lib.imgenv_rollout_seq_enable(self.h, C.byref(c), C.byref(so)), "imgenv_rollout_seq_enable")
        if self.sequences is None:
            L, Bs, NB, S = so.length, so.batch, so.buffers, so.max_sequences
            views = self._views(so, {"seq_flag": (np.uint8, (S,)), "seq_valid": (np.int32, (S,)), "seq_order": (np.int32, (S,)),
                                     "seq_valid_n": (np.int32, (1,))}, "imgenv_seq_out")  # (seq_valid_n: uint32 in the library)
            rows = {"mb_" + name: (self._rollout_rows[name][0], (L, Bs) + tuple(self._rollout_rows[name][1][1:]))
                    for name in _cabi.ROLLOUT_FIELDS + _cabi.ROLLOUT_NORM_FIELDS if getattr(so.buf[0], "mb_" + name)}
            rows.update(mb_actions=(np.float32, (L, Bs, 3)), mb_rewards=(np.float32, (L, Bs)), mb_dones=(np.uint8, (L, Bs)),
                        mb_dones_info=(np.int32, (L, Bs)), mb_index=(np.int32, (L, Bs)), mb_weight=(np.float32, (L, Bs)),
                        mb_first=(np.uint8, (L, Bs)), mb_scalars=(np.float32, (_cabi.MB_MAX_SCALARS, L, Bs)), mb_seq=(np.int32, (Bs,)),
                        mb_seq_len=(np.int32, (Bs,)))
            for name, (dt, shape) in rows.items():
                views[name] = self._side_by_side(name, [getattr(so.buf[b], name) for b in range(NB)], dt, shape, "imgenv_seq_buffer")
            for a in range(_cabi.SEQ_MAX_STATES):
                if so.state_bytes[a] > 0:
                    views["mb_seq_state%d" % a] = self._side_by_side("mb_seq_state%d" % a, [so.buf[b].mb_seq_state[a] for b in range(NB)], np.uint8,
                                                                     (Bs, so.state_bytes[a]), "imgenv_seq_buffer")
            self.sequences = views
            self.seq_length, self.seq_batch, self.seq_buffers, self.seq_state_bytes = L, Bs, NB, tuple(so.state_bytes)
        return self.sequences

    def _need_sequences(self):
        if self.sequences is None:
            raise RuntimeError("enable_sequences() was not called")

    def rollout_seq_index(self):
        """``imgenv_rollout_seq_index``: ``sequences["seq_flag"][q]`` = 1 where any transition sequence ``q`` covers has ``is_clean !=
        0``, ``seq_valid`` the ascending list of those, ``seq_valid_n`` their count; four launches on the current stream, nothing
        synchronises.  A later step, reset or ``rollout_begin()`` makes the index stale: ``rollout_seq_shuffle`` / ``_seq_minibatch``
        then raise RuntimeError."""
        self._need_sequences()
        self._check(self.lib.imgenv_rollout_seq_index(self.h, self._stream()), "imgenv_rollout_seq_index")

    def rollout_seq_count(self):
        """``seq_valid_n`` as a Python int.  SYNCHRONISES: it waits for the stream and reads one word from the device."""
        self._need_sequences()
        return int(self.sequences["seq_valid_n"].item())

    def rollout_seq_shuffle(self, seed):
        """``imgenv_rollout_seq_shuffle``: ``sequences["seq_order"]`` = the valid sequences in a fresh order drawn from the 64-bit
        ``seed`` (``rollout_shuffle``'s bijection over ``seq_valid_n``), -1 behind; one launch"""
        self._need_sequences()
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._check(self.lib.imgenv_rollout_seq_shuffle(self.h, seed & 0xFFFFFFFF, seed >> 32, self._stream()), "imgenv_rollout_seq_shuffle")

    def rollout_seq_minibatch(self, j, buffer=0, scalars=(), normalise=None, norm=None, states=()):
        """``imgenv_rollout_seq_minibatch``: sequence minibatch ``j`` of the current order into buffer ``buffer``, one launch (two
        where the rollout draws its ``ped_maps``).  ``scalars``: up to 6 float32 tensors ``[T, R]`` or ``[T + 1, R]``, gathered into
        ``sequences["mb_scalars"][buffer, s]`` ``[L, Bs]``; ``normalise``: an index into them whose values become ``(x - norm[0]) *
        norm[1]`` with ``norm`` float32 ``[2]`` (required then).  ``states``: one contiguous tensor ``[T or T + 1, R, ...]`` per
        ``state_bytes`` entry of ``enable_sequences``, rows of exactly that many bytes, 16-byte aligned: ``mb_seq_state<a>[buffer,
        i]`` is its row at the first step of slot ``i``'s sequence.  Steps that do not exist and slots behind the valid list are
        zeros with ``mb_index`` -1 and ``mb_weight`` 0.  Returns the dict of buffer ``buffer``'s views."""
        import torch
        self._need_sequences()
        T, R = self.rollout_horizon, self.n_local
        scalars, states = list(scalars), list(states)
        if len(scalars) > _cabi.MB_MAX_SCALARS:
            raise ValueError("rollout_seq_minibatch: at most %d scalars" % _cabi.MB_MAX_SCALARS)
        ptrs = [self._mb_tensor(t, "rollout_seq_minibatch: scalars[%d]" % s, [(T, R), (T + 1, R)]).value for s, t in enumerate(scalars)]
        np_ = self._mb_tensor(norm, "rollout_seq_minibatch: norm", [(2,)]).value if norm is not None else None
        if normalise is not None and norm is None:
            raise ValueError("rollout_seq_minibatch: normalise needs norm, float32 [2]")
        want = [nb for nb in self.seq_state_bytes if nb > 0]
        if len(states) != len(want):
            raise ValueError("rollout_seq_minibatch: %d state arrays (enable_sequences was given %d)" % (len(states), len(want)))
        sp = [None] * _cabi.SEQ_MAX_STATES
        slots = [a for a, nb in enumerate(self.seq_state_bytes) if nb > 0]
        for a, t in zip(slots, states):
            nb = self.seq_state_bytes[a]
            if not (isinstance(t, torch.Tensor) and t.device == self.device and t.is_contiguous() and t.dim() >= 2 and t.shape[0] in (T, T + 1)
                    and t.shape[1] == R and t[0, 0].numel() * t.element_size() == nb):
                raise ValueError("rollout_seq_minibatch: states[%d]: [%d or %d, %d, ...] with rows of %d bytes, contiguous on %s" % (a, T, T + 1, R, nb, self.device))
            sp[a] = t.data_ptr()
        a = _cabi.make_seq_args(j, buffer, ptrs, -1 if normalise is None else normalise, np_, sp)
        self._call(self.lib.imgenv_rollout_seq_minibatch(self.h, C.byref(a), self._stream()), "imgenv_rollout_seq_minibatch")
        return {name: t[buffer] for name, t in self.sequences.items() if name.startswith("mb_")}

    def reset(self, layout):
        """Reset everything. A handle of several worlds (``n_worlds`` > 1) takes either one batch of all robots and
        pedestrians (world-major) with an obstacle list shared by every world, or a list of one layout per world."""
        if isinstance(layout, (list, tuple)):
            if len(layout) != self.n_worlds:
                raise ValueError("expected %d layouts, one per world" % self.n_worlds)
            return self.reset_worlds(list(range(self.n_worlds)), layout)
        b, keep = _cabi.make_reset_batch(layout if isinstance(layout, dict) else layout.as_batch(), self.n_robots,
                                         self.n_peds)
        self._check(self.lib.imgenv_reset(self.h, C.byref(b), self._stream()), "imgenv_reset")
        return self.out

    def prepare_reset(self, layout):
        """The C-ABI reset batch of one world's layout, built once and reusable: ``(batch, keepalive)`` for ``reset_worlds``."""
        return _cabi.make_reset_batch(layout if isinstance(layout, dict) else layout.as_batch(),
                                      self.n_robots // self.n_worlds, self.n_peds // self.n_worlds)

    def reset_worlds(self, worlds, layouts):
        """Reset several worlds of a multi-world handle in one call (one set of launches): ``layouts[q]`` -- a layout or
        what ``prepare_reset`` returned for it -- goes to world ``worlds[q]``."""
        n = len(worlds)
        if n == 0:
            return self.out
        prepared = [lay if isinstance(lay, tuple) else self.prepare_reset(lay) for lay in layouts]
        arr = (_cabi.ResetBatch * n)(*[b for b, _ in prepared])
        ids = (C.c_int32 * n)(*[int(k) for k in worlds])
        if self._trace is not None:
            import time
            t0 = time.perf_counter()
            rc = self.lib.imgenv_reset_worlds(self.h, n, ids, arr, self._stream())
            self._trace[0] += time.perf_counter() - t0
            self._trace[1] += 1
            self._check(rc, "imgenv_reset_worlds")
            return self.out
        self._check(self.lib.imgenv_reset_worlds(self.h, n, ids, arr, self._stream()), "imgenv_reset_worlds")
        return self.out

    def reset_worlds_spawn(self, worlds, spawn_cfg, seeds):
        """Reset the listed worlds from fresh random placements made inside the library (``imgenv_reset_worlds_spawn``):
        ``spawn_cfg`` = what ``spawn.make_spawn_cfg`` returned, ``seeds[q]`` seeds world ``worlds[q]``."""
        n = len(worlds)
        if n == 0:
            return self.out
        ids = (C.c_int32 * n)(*[int(k) for k in worlds])
        sd = (C.c_uint64 * n)(*[int(v) & 0xFFFFFFFFFFFFFFFF for v in seeds])
        self._check(self.lib.imgenv_reset_worlds_spawn(self.h, n, ids, C.byref(spawn_cfg[0]), sd, self._stream()),
                    "imgenv_reset_worlds_spawn")
        return self.out

    def reset_world(self, world, layout):
        """Reset ONE world of a multi-world handle (ImageEnv.reset of one env process, yaml_env.py:296-317); the others
        keep their state and their time limits.  ``layout`` holds that world's robots, pedestrians and obstacles."""
        b, keep = _cabi.make_reset_batch(layout if isinstance(layout, dict) else layout.as_batch(),
                                         self.n_robots // self.n_worlds, self.n_peds // self.n_worlds)
        self._check(self.lib.imgenv_reset_world(self.h, int(world), C.byref(b), self._stream()), "imgenv_reset_world")
        return self.out

    def _actions(self, actions):
        import torch
        if not isinstance(actions, torch.Tensor):
            actions = torch.as_tensor(np.ascontiguousarray(actions, np.float32), device=self.device)
        if actions.dtype != torch.float32 or actions.device != self.device or not actions.is_contiguous():
            actions = actions.to(device=self.device, dtype=torch.float32).contiguous()
        if actions.numel() != self.n_local * 3:
            raise ValueError("actions must be [%d, 3] (v, w, beep)" % self.n_local)
        return actions

    def step(self, actions, actions_ready=None):
        """One step, ordered on the current stream: behind whatever writes ``actions`` there, and behind whatever still reads the
        last step's outputs there.  ``actions_ready`` (``IMGENV_STEP_ACTIONS_READY``) is accepted for compatibility and has had no
        effect since round 6 (include/imgenv.h)."""
        import torch
        if actions_ready is None:
            actions_ready = not isinstance(actions, torch.Tensor)
        a = self._actions(actions)  # (host data: torch's copy from pageable memory returns when the data is on the device)
        self._check(self.lib.imgenv_step_flags(self.h, C.c_void_p(a.data_ptr()), _cabi.STEP_ACTIONS_READY if actions_ready else 0,
                                               self._stream()), "imgenv_step")
        return self.out

    def step_autoreset(self, actions, spawn_cfg, seed0):
        """``imgenv_step_autoreset``: one step, then every world whose robots are all done starts a new episode from a fresh
        placement drawn inside the library (the k-th such world, ascending, from ``seed0 + k``).  Returns the outputs and the
        list of worlds that were reset; ``out['step_*']`` keep what the step itself returned for them."""
        a = self._actions(actions)
        if self._finished_buf is None:
            self._finished_buf = (C.c_int32 * self.n_worlds)()
        n = C.c_int32(0)
        self._check(self.lib.imgenv_step_autoreset(self.h, C.c_void_p(a.data_ptr()), C.byref(spawn_cfg[0]),
                                                   C.c_uint64(int(seed0) & 0xFFFFFFFFFFFFFFFF), self._finished_buf,
                                                   self.n_worlds, C.byref(n), self._stream()), "imgenv_step_autoreset")
        return self.out, list(self._finished_buf[:n.value])

    def step_autoreset_device(self, actions, spawn_cfg, seed0):
        """``imgenv_step_autoreset_device``: the same without the host in the loop -- finished worlds are found, placed and
        reset by kernels alone, the call returns once everything is queued (no synchronisation, nothing read back).  The first
        call fixes ``seed0``: the k-th world reset from then on takes placement ``seed0 + k``."""
        a = self._actions(actions)
        self._check(self.lib.imgenv_step_autoreset_device(self.h, C.c_void_p(a.data_ptr()), C.byref(spawn_cfg[0]),
                                                          C.c_uint64(int(seed0) & 0xFFFFFFFFFFFFFFFF), self._stream()),
                    "imgenv_step_autoreset_device")
        return self.out

    def autoreset_last(self):
        """(worlds the last ``step_autoreset_device`` reset, placement number of the first of them); synchronises the stream"""
        if self._finished_buf is None:
            self._finished_buf = (C.c_int32 * self.n_worlds)()
        n, first = C.c_int32(0), C.c_uint64(0)
        self._check(self.lib.imgenv_autoreset_last(self.h, self._finished_buf, self.n_worlds, C.byref(n), C.byref(first), self._stream()),
                    "imgenv_autoreset_last")
        return list(self._finished_buf[:n.value]), int(first.value)

    def world_placement(self, world, n_obstacles):
        """the placement ``world`` currently runs, as its device-side reset received it: ``(ResetLayout, placement number)``"""
        from .worldgen import ResetLayout
        R, P, O = self.n_robots // self.n_worlds, self.n_peds // self.n_worlds, int(n_obstacles)
        out = dict(robot_pose=np.zeros((R, 4)), robot_goal=np.zeros((R, 2)), ped_pose=np.zeros((P, 4)), ped_goal=np.zeros((P, 2)),
                   ped_traj=np.zeros((P, 2, 3)), ped_traj_len=np.zeros(P, np.int32), obs_shape=np.zeros(O, np.int32),
                   obs_size=np.zeros((O, 4), np.float32), obs_pose=np.zeros((O, 4)))
        serial = C.c_uint64(0)
        self._check(self.lib.imgenv_world_placement(self.h, int(world), C.byref(serial), *[a.ctypes.data for a in out.values()]),
                    "imgenv_world_placement")
        return ResetLayout(**out), int(serial.value)

    def step_begin(self, actions):
        a = self._actions(actions)
        # (kept until step_end: the step's kernels read the actions up to the chain's end, include/imgenv.h -- a tensor made here
        # from host data would otherwise go back to torch's allocator, and to whoever allocates next, between the two calls)
        self._step_actions = a
        self._check(self.lib.imgenv_step_begin(self.h, C.c_void_p(a.data_ptr()), self._stream()), "imgenv_step_begin")

    def step_end(self):
        self._check(self.lib.imgenv_step_end(self.h, self._stream()), "imgenv_step_end")
        self._step_actions = None
        return self.out

    def init_comm(self, rank=None, n_ranks=None):
        """Give the library its own RCCL communicator so that ``step()`` runs the all-gather of a
        robot-sharded world itself.  The 128-byte id is created on rank 0 and broadcast through the
        already-initialised ``torch.distributed`` group (plumbing only)."""
        import torch
        import torch.distributed as dist
        rank = dist.get_rank() if rank is None else rank
        n_ranks = dist.get_world_size() if n_ranks is None else n_ranks
        buf = (C.c_ubyte * 128)()
        if rank == 0:
            self._check(self.lib.imgenv_comm_unique_id(buf), "imgenv_comm_unique_id")
        t = torch.tensor(list(buf), dtype=torch.uint8, device=self.device)
        if n_ranks > 1:
            dist.broadcast(t, src=0)
        raw = bytes(t.cpu().tolist())
        buf2 = (C.c_ubyte * 128).from_buffer_copy(raw)
        self._check(self.lib.imgenv_comm_init(self.h, buf2, rank, n_ranks), "imgenv_comm_init")
        self.native_comm = True

    def comm_info(self):
        """(ranks, rank) as RCCL reports them for the library's own communicator"""
        n, r = C.c_int32(), C.c_int32()
        self._check(self.lib.imgenv_comm_info(self.h, C.byref(n), C.byref(r)), "imgenv_comm_info")
        return n.value, r.value

    def launches(self):
        return self.lib.imgenv_step_launches(self.h)

    def layer_mode(self):
        """what ``imgenv_create`` decided: {"layer": composed | stamped | counting, "shard_bitmaps", "early_observation", "crowd_ahead"}"""
        m = self.lib.imgenv_layer_mode(self.h)
        return dict(layer=("composed", "stamped", "counting")[m & 3], shard_bitmaps=bool(m & 4), early_observation=bool(m & 8),
                    crowd_ahead=bool(m & 16))

    def timing(self, mode, which=-1):
        """0 off, 1 every kernel, 2 only kernel id ``which`` (HIP events on the launch stream)"""
        self._check(self.lib.imgenv_timing(self.h, mode, which), "imgenv_timing")

    def timing_read(self):
        """{kernel name: (total ms, launches)} since the last timing() call"""
        ms = (C.c_double * _cabi.K_COUNT)()
        n = (C.c_int64 * _cabi.K_COUNT)()
        self._check(self.lib.imgenv_timing_read(self.h, ms, n), "imgenv_timing_read")
        return {self.lib.imgenv_kernel_name(q).decode(): (ms[q], n[q]) for q in range(_cabi.K_COUNT)}

    def snapshot(self):
        """host copies (numpy) of every output, after synchronising the stream"""
        import torch
        torch.cuda.synchronize(self.device)
        return {k: v.cpu().numpy().copy() for k, v in self.out.items()}

    def close(self):
        if getattr(self, "h", None):
            self.episodes = self.episode_log = self.action_outputs = self.obs_post = self.final_obs = self.rollout = self.minibatch = None  # (views of memory the handle owns)
            self.normalise = self.policy = self.policy_loss_out = self.sequences = None
            self.lib.imgenv_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
