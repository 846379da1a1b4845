"""ctypes mirror of ``include/imgenv.h`` -- the C ABI of the HIP step() library.

The product path loads ``img_env_amd/csrc/libimgenv_hip.so`` and nothing else: there is no CPU
fallback.  :func:`load_library` raises if the extension is missing or was built for another ABI.
"""
import ctypes as C
import os

import numpy as np

ABI_VERSION = 2
RECORD_DOUBLES = 8

SHAPE_CIRCLE, SHAPE_RECTANGLE, SHAPE_LEG = 0, 1, 2
SCENE_EMPTY, SCENE_RVO, SCENE_ERVO, SCENE_PEDSIM, SCENE_DATASET = 0, 1, 2, 3, 4
KTYPE_DIFF, KTYPE_OMNI = 0, 1
FLAG_PRIVATE_GRIDS = 1
FLAG_COMPOSE_DENSE = 2
FLAG_COMPOSE_SPARSE = 4
STEP_ACTIONS_READY = 1  # imgenv_step_flags: the actions are complete when the call is made (include/imgenv.h)
FLAG_LAYER_SUM = 512  # the counting class layer wherever it can run (include/imgenv.h)
FLAG_NO_VIEW_MAPS = 8  # imgenv_out.view_maps not wanted (include/imgenv.h)
FLAG_VIEW_TILED = 32  # views through the tiled kernels (csrc/view_big.h) / through k_view, where both can run
FLAG_VIEW_WAVE = 64
FLAG_AGENT_STATE_EXTRAS = 16  # AgentState.hits_x / hits_y / angular_map as well
FLAG_CHECK_OUTPUTS = 128  # debug: checksum every output array between calls, EINVAL "the caller wrote into imgenv_out.<field>"
FLAG_FULL_REWRITE = 256   # the outputs are copies rewritten in full by every call (the reference's value-copy ownership)
FLAG_CHECK_OUTPUTS_FIRST = 1024  # FLAG_CHECK_OUTPUTS for the handle's first 64 calls only (World's default)
ANGULAR_BINS = 72
STACK_MAX_DEPTH = 16  # IMGENV_STACK_MAX_DEPTH
MAPS_KEEP, MAPS_BY_PLACEMENT = 0, 1  # imgenv_maps_policy
MAP_POLICIES = {"keep": MAPS_KEEP, "placement": MAPS_BY_PLACEMENT}
TRACKS_KEEP, TRACKS_BY_PLACEMENT, TRACKS_CYCLE = 0, 1, 2  # imgenv_tracks_policy
TRACK_POLICIES = {"keep": TRACKS_KEEP, "placement": TRACKS_BY_PLACEMENT, "cycle": TRACKS_CYCLE}
TRACKS_PLACEMENT_SALT = 0xBB67AE8584CAA73B  # imgenv_tracks_for_placement (csrc/track_bank.h)
SCENARIOS_OFF, SCENARIOS_QUEUE, SCENARIOS_BY_PLACEMENT = 0, 1, 2  # imgenv_scenarios_policy
SCENARIO_POLICIES = {"off": SCENARIOS_OFF, "queue": SCENARIOS_QUEUE, "placement": SCENARIOS_BY_PLACEMENT}
SCENARIO_PLACEMENT_SALT = 0x3C6EF372FE94F82B  # imgenv_scenario_for_placement (csrc/scenario_bank.h)
SPAWN_MAX_AGENTS, SPAWN_MAX_OBST = 256, 24  # one world's cast in the device-side reset (csrc/spawn_slot.h)
EINVAL, ENOMEM, EDEVICE, ESTATE = -1, -2, -3, -4

SHAPES = {"circle": SHAPE_CIRCLE, "rectangle": SHAPE_RECTANGLE, "leg": SHAPE_LEG}
# Env.msg ped_scene_type strings (scenefactory.h:8-24): anything else is the EmptyScene
SCENES = {"rvoscene": SCENE_RVO, "ervoscene": SCENE_ERVO, "pedscene": SCENE_PEDSIM, "dataset": SCENE_DATASET}
KTYPES = {"diff": KTYPE_DIFF, "omni": KTYPE_OMNI}

_i32, _f32, _f64, _i64 = C.c_int32, C.c_float, C.c_double, C.c_int64
_pi32, _pf32, _pf64 = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)


class Limiter(C.Structure):
    _fields_ = [("has_velocity_limits", _i32), ("has_acceleration_limits", _i32), ("has_jerk_limits", _i32),
                ("min_velocity", _f32), ("max_velocity", _f32), ("min_acceleration", _f32),
                ("max_acceleration", _f32), ("min_jerk", _f32), ("max_jerk", _f32)]


class Cfg(C.Structure):
    _fields_ = [
        ("abi_version", _i32), ("struct_size", _i32),
        ("view_resolution", _f32), ("view_width", _f32), ("view_height", _f32), ("step_hz", _f32),
        ("state_dim", _i32), ("use_laser", _i32), ("range_total", _i32),
        ("view_angle_begin", _f32), ("view_angle_end", _f32), ("view_min_dist", _f32), ("view_max_dist", _f32),
        ("beep_r", _f32), ("ped_ca_p", _f32), ("relation_ped_robo", _i32),
        ("global_resolution", _f32), ("ped_scene_type", _i32), ("n_robots", _i32), ("n_peds", _i32),
        ("robot_ktype", _i32),
        ("robot_shape", _pi32), ("robot_size", _pf32), ("robot_sensor_cfg", _pf32),
        ("limiter_v", Limiter), ("limiter_w", Limiter),
        ("ped_shape", _pi32), ("ped_size", _pf32), ("ped_max_speed", _pf32),
        ("image_size", _i32 * 2), ("ped_image_size", _i32 * 2), ("max_ped", _i32), ("ped_vec_dim", _i32),
        ("ped_image_r", _f64), ("laser_max", _f64), ("laser_norm", _i32),
        ("robot_size_last", _pf64),
        ("ped_safety_space", _f64), ("time_max", _i32),
        ("robot_begin", _i32), ("robot_end", _i32),
        ("device", _i32), ("flags", _i32),
        ("out_arena", C.c_void_p), ("out_arena_bytes", _i64),
        ("n_worlds", _i32), ("reserved_", _i32),
    ]


class ResetBatch(C.Structure):
    _fields_ = [
        ("struct_size", _i32), ("n_obstacles", _i32),
        ("obs_shape", _pi32), ("obs_size", _pf32), ("obs_pose", _pf64),
        ("robot_pose", _pf64), ("robot_goal", _pf64),
        ("ped_pose", _pf64), ("ped_goal", _pf64), ("ped_traj_len", _pi32), ("ped_traj", _pf64),
        ("ped_traj_cap", _i32), ("ignore_obstacle", _i32),
        ("ped_traj_v", _pf64),
    ]


POSE_FIX, POSE_RAND_ANGLE, POSE_RANGE, POSE_RANGE_YAW, POSE_RANGE_VIEW = 0, 1, 2, 3, 4
POSE_RANGE_CIRCLE, POSE_RANGE_CIRCLE_FIX, POSE_CIRCLE_FIX, POSE_RANGE_MULTI = 5, 6, 7, 8


class SpawnAgent(C.Structure):
    _fields_ = [("begin_type", _i32), ("target_type", _i32), ("begin", C.c_double * 6), ("target", C.c_double * 6),
                ("module_size", C.c_double), ("begin_multi", C.POINTER(C.c_double)), ("target_multi", C.POINTER(C.c_double)),
                ("n_begin_multi", _i32), ("n_target_multi", _i32)]


class SpawnObstacle(C.Structure):
    _fields_ = [("shape", _i32), ("pose_type", _i32), ("size_range", C.c_double * 4), ("pose", C.c_double * 6)]


class SpawnCfg(C.Structure):
    _fields_ = [("struct_size", _i32), ("n_robots", _i32), ("n_peds", _i32), ("n_obstacles", _i32),
                ("agents", C.POINTER(SpawnAgent)), ("obstacles", C.POINTER(SpawnObstacle)),
                ("clearance", C.c_double), ("target_min_dist", C.c_double), ("circle_ranges", C.c_double * 2),
                ("go_back", _i32), ("ignore_obstacle", _i32)]


class Out(C.Structure):
    _fields_ = [
        ("struct_size", _i32), ("n_local", _i32), ("view_h", _i32), ("view_w", _i32), ("n_beams", _i32),
        ("state_dim", _i32), ("ped_vec_len", _i32), ("image_h", _i32), ("image_w", _i32), ("grid_h", _i32), ("grid_w", _i32),
        ("vector_states", C.c_void_p), ("view_maps", C.c_void_p), ("sensor_maps", C.c_void_p),
        ("lasers_raw", C.c_void_p), ("lasers", C.c_void_p), ("ped_vector_states", C.c_void_p),
        ("ped_maps", C.c_void_p), ("is_collisions", C.c_void_p), ("is_arrives", C.c_void_p),
        ("step_ds", C.c_void_p), ("ped_min_dists", C.c_void_p),
        ("base_rewards", C.c_void_p), ("base_dones", C.c_void_p),
        ("rewards", C.c_void_p), ("paper_rewards", C.c_void_p), ("dones", C.c_void_p), ("dones_info", C.c_void_p), ("is_clean", C.c_void_p),
        ("robot_pose", C.c_void_p), ("ped_state", C.c_void_p), ("counters", C.c_void_p),
        ("step_rewards", C.c_void_p), ("step_dones", C.c_void_p), ("step_dones_info", C.c_void_p), ("step_is_clean", C.c_void_p),
        ("step_is_arrives", C.c_void_p), ("step_is_collisions", C.c_void_p), ("step_all_down", C.c_void_p),
        ("hits_x", C.c_void_p), ("hits_y", C.c_void_p), ("angular_map", C.c_void_p),
    ]


class StackCfg(C.Structure):
    _fields_ = [("struct_size", _i32), ("image_batch", _i32), ("state_batch", _i32), ("laser_batch", _i32),
                ("arena", C.c_void_p), ("arena_bytes", _i64)]


class StackOut(C.Structure):
    _fields_ = [("struct_size", _i32), ("n_local", _i32), ("image_depth", _i32), ("state_depth", _i32), ("laser_depth", _i32),
                ("reserved_", _i32), ("sensor_maps", C.c_void_p), ("vector_states", C.c_void_p), ("lasers", C.c_void_p)]


def make_stack_cfg(image_batch, state_batch, laser_batch, arena=None, arena_bytes=0):
    """the YAML keys of StateBatchWrapper (base.py:103-105) as an ``imgenv_stack_cfg``"""
    s = StackCfg()
    s.struct_size = C.sizeof(StackCfg)
    s.image_batch, s.state_batch, s.laser_batch = int(image_batch), int(state_batch), int(laser_batch)
    s.arena, s.arena_bytes = arena, int(arena_bytes)
    return s


class EpisodesCfg(C.Structure):
    _fields_ = [("struct_size", _i32), ("min_steps", _i32), ("dt", _f64)]


#: imgenv_episodes_out's arrays: name -> (numpy dtype, rows: 0 = [R], k = [k][R])
EP_END_BINS, EP_FIGURES, EP_OPEN_F64 = 6, 8, 15
EP_ENDS = ("arrive", "timeout", "static_collision", "ped_collision", "other_collision", "aborted")  # rows of ``ends``
EP_FIGURE_NAMES = ("w_variance", "w_zero", "v_acc", "w_acc", "v_jerk", "w_jerk", "v_avg", "w_avg")  # rows of ``figure_sums``
EP_OPEN_NAMES = ("n", "sum_v", "sum_w", "sum_ww", "sum_absw", "acc_v", "acc_w", "jerk_v", "jerk_w", "prev_v", "prev_w", "prev2_v",
                 "prev2_w", "w_zero", "ep_return")  # rows of ``open_f64``
EPISODE_ARRAYS = {
    "ends": (np.int32, EP_END_BINS), "episodes": (np.int32, 0), "short_episodes": (np.int32, 0), "speed_steps": (np.int32, 0),
    "arrive_steps": (np.int32, 0), "len_sum": (np.int32, 0), "v_sum": (np.float64, 0), "w_sum": (np.float64, 0),
    "figure_sums": (np.float64, EP_FIGURES), "return_sum": (np.float64, 0), "last_code": (np.int32, 0), "last_steps": (np.int32, 0),
    "last_len": (np.int32, 0), "last_episode": (np.int32, 0), "last_return": (np.float64, 0), "open_f64": (np.float64, EP_OPEN_F64),
    "open_steps": (np.int32, 0), "open_len": (np.int32, 0), "open": (np.int32, 0),
}


class EpisodesOut(C.Structure):
    _fields_ = [("struct_size", _i32), ("n_local", _i32)] + [(name, C.c_void_p) for name in EPISODE_ARRAYS]


def make_episodes_cfg(min_steps, dt):
    """``imgenv_episodes_cfg``: TestEpisodeWrapper's ``tmp_steps > 3`` (TestEpisodeWrapper.py:48) and ``control_hz`` (:17)"""
    c = EpisodesCfg()
    c.struct_size = C.sizeof(EpisodesCfg)
    c.min_steps, c.dt = int(min_steps), float(dt)
    return c


EPLOG_MAX_CAPACITY, EPLOG_I32, EPLOG_F64, EPLOG_SCN_DEVICE = 1 << 22, 10, 9, -2
#: rows of imgenv_episode_log_out.i32 and .f64
EPLOG_I32_NAMES = ("robot", "world", "code", "steps", "len", "counted", "episode", "map", "tracks", "scenario_raw")
EPLOG_F64_NAMES = ("ep_return",) + EP_FIGURE_NAMES
#: imgenv_episode_log_out's arrays: name -> (numpy dtype, rows: 0 = [capacity], k = [k][capacity], -1 = [1]).  The two uint64 arrays
#: are viewed as int64 (torch has no arithmetic on uint64): a placement of ~0, "none", reads -1.
EPISODE_LOG_ARRAYS = {"n_written": (np.int64, -1), "i32": (np.int32, EPLOG_I32), "f64": (np.float64, EPLOG_F64), "placement": (np.int64, 0)}


class EpisodeLogCfg(C.Structure):
    _fields_ = [("struct_size", _i32), ("capacity", _i32)]


class EpisodeLogOut(C.Structure):
    _fields_ = [("struct_size", _i32), ("capacity", _i32)] + [(name, C.c_void_p) for name in EPISODE_LOG_ARRAYS]


class EpisodeRecord(C.Structure):
    """``imgenv_episode_record``: 128 bytes"""
    _fields_ = ([("seq", C.c_uint64), ("placement", C.c_uint64)] +
                [(k, _i32) for k in ("robot", "world", "code", "steps", "len", "counted", "episode", "map", "tracks", "scenario")] +
                [("ep_return", _f64), ("figures", _f64 * EP_FIGURES)])


#: ``EpisodeRecord`` as a numpy record dtype (the same 128 bytes)
EPISODE_RECORD_DTYPE = np.dtype([("seq", np.uint64), ("placement", np.uint64)] +
                                [(k, np.int32) for k in ("robot", "world", "code", "steps", "len", "counted", "episode", "map", "tracks", "scenario")] +
                                [("ep_return", np.float64), ("figures", np.float64, (EP_FIGURES,))])


def make_episode_log_cfg(capacity):
    c = EpisodeLogCfg()
    c.struct_size = C.sizeof(EpisodeLogCfg)
    c.capacity = int(capacity)
    return c


ACTIONS_TABLE, ACTIONS_CLIP, ACTIONS_MAX_TABLE = 0, 1, 4096
RAW_I32, RAW_I64, RAW_F32, RAW_F64 = 0, 1, 2, 3  # ``dtype`` of imgenv_actions_decode
RAW_DTYPES = {np.dtype(np.int32): RAW_I32, np.dtype(np.int64): RAW_I64, np.dtype(np.float32): RAW_F32, np.dtype(np.float64): RAW_F64}
OBS_PED_NORM, OBS_CLOSE = 1, 2
#: StatePedVectorWrapper.avg / .std (base.py:20-21) and InfoLogWrapper's ``ped_min_dist < 1`` (base.py:250)
PED_NORM_AVG = (0.0, 0.0, 0.0, 0.0, 0.25, 0.25, 0.0)
PED_NORM_STD = (6.0, 6.0, 0.6, 0.9, 0.50, 0.5, 6.0)
CLOSE_DIST = 1.0


class ActionsCfg(C.Structure):
    _fields_ = [("struct_size", _i32), ("mode", _i32), ("n_cols", _i32), ("n_table", _i32), ("table", C.c_void_p), ("clip", (_f32 * 2) * 3)]


#: imgenv_actions_out's arrays: name -> (numpy dtype, columns: the array is [R][columns]; 0 = one element for the handle)
ACTION_ARRAYS = {"actions": (np.float32, 3), "speeds": (np.float32, 2), "n_bad": (np.int32, 0)}


class ActionsOut(C.Structure):
    _fields_ = [("struct_size", _i32), ("n_local", _i32)] + [(name, C.c_void_p) for name in ACTION_ARRAYS]


def make_actions_cfg(table=None, clip=None, n_cols=2):
    """``imgenv_actions_cfg``: TABLE mode from the YAML's ``discrete_actions`` (rows of 2 or 3 values; a two-column row gets beep
    0, action.py:29-30), or CLIP mode from its ``continuous_actions`` (at least ``n_cols`` rows of (lo, hi)).  Returns the struct
    and what it points to."""
    c = ActionsCfg()
    c.struct_size = C.sizeof(ActionsCfg)
    c.n_cols = int(n_cols)
    keep = None
    if table is not None:
        rows = [list(r) for r in table]
        if any(len(r) not in (2, 3) for r in rows):
            raise ValueError("discrete_actions: rows of (v, w) or (v, w, beep)")
        keep = np.ascontiguousarray([[r[0], r[1], r[2] if len(r) == 3 else 0] for r in rows], np.float32).reshape(-1, 3)
        c.mode, c.n_table, c.table = ACTIONS_TABLE, len(keep), keep.ctypes.data if len(keep) else None
    else:
        rng = np.asarray(clip, np.float64).reshape(-1, 2)
        if c.n_cols in (2, 3) and len(rng) < c.n_cols:
            raise ValueError("continuous_actions: %d ranges for %d columns (IndexError in base.py:50)" % (len(rng), c.n_cols))
        c.mode = ACTIONS_CLIP
        for i, (lo, hi) in enumerate(rng[:3]):
            c.clip[i][0], c.clip[i][1] = float(lo), float(hi)
    return c, keep


#: the policy head (imgenv_policy_enable; csrc/policy.h)
POLICY_CATEGORICAL, POLICY_GAUSSIAN = 0, 1
POLICY_STORE = 1  # imgenv_policy_cfg.flags
POLICY_DETERMINISTIC, POLICY_LOG_STD_PER_ROW, POLICY_NO_STORE, POLICY_VALUE_ONLY = 1, 2, 4, 8  # imgenv_policy_args.flags
#: imgenv_policy_out's arrays, in the struct's order
POLICY_ARRAYS = ("index", "raw", "logp", "entropy", "pol_raw", "pol_logp", "pol_value")


class PolicyCfg(C.Structure):
    _fields_ = [("struct_size", _i32), ("kind", _i32), ("flags", _i32), ("reserved", _i32), ("seed", C.c_uint64)]


class PolicyOut(C.Structure):
    _fields_ = [("struct_size", _i32), ("n_local", _i32), ("n_params", _i32), ("horizon", _i32)] + [(name, C.c_void_p) for name in POLICY_ARRAYS]


class PolicyArgs(C.Structure):
    _fields_ = [("struct_size", _i32), ("flags", _i32), ("draw", C.c_uint64), ("params", C.c_void_p), ("log_std", C.c_void_p),
                ("values", C.c_void_p)]


def make_policy_cfg(kind, seed=0, store=False):
    """``imgenv_policy_cfg``: ``kind`` is POLICY_CATEGORICAL / POLICY_GAUSSIAN or "categorical" / "gaussian" """
    c = PolicyCfg()
    c.struct_size = C.sizeof(PolicyCfg)
    c.kind = {"categorical": POLICY_CATEGORICAL, "gaussian": POLICY_GAUSSIAN}.get(kind, kind)
    c.flags = POLICY_STORE if store else 0
    c.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return c


#: PPO's loss (imgenv_policy_loss_enable; csrc/policy_loss.h)
PLOSS_CLIP_VALUE = 1  # imgenv_policy_loss_args.flags, beside POLICY_LOG_STD_PER_ROW
#: imgenv_policy_loss_out's arrays, in the struct's order
PLOSS_ARRAYS = ("logp", "entropy", "ratio", "pg", "vl", "d_params", "d_log_std", "d_log_std_shared", "d_values", "stats", "n_bad", "inv_w")
#: the entries of stats
PLOSS_STATS = ("loss", "pg_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "weight_sum")


class PolicyLossCfg(C.Structure):
    _fields_ = [("struct_size", _i32), ("max_rows", _i32), ("reserved", _i32 * 2)]


class PolicyLossOut(C.Structure):
    _fields_ = [("struct_size", _i32), ("n_params", _i32), ("max_rows", _i32), ("reserved", _i32)] + [(name, C.c_void_p) for name in PLOSS_ARRAYS]


class PolicyLossArgs(C.Structure):
    _fields_ = [("struct_size", _i32), ("flags", _i32), ("rows", _i32), ("reserved", _i32), ("params", C.c_void_p), ("log_std", C.c_void_p),
                ("values", C.c_void_p), ("action", C.c_void_p * 3), ("old_logp", C.c_void_p), ("old_value", C.c_void_p), ("adv", C.c_void_p),
                ("ret", C.c_void_p), ("weight", C.c_void_p), ("clip", _f32), ("clip_vf", _f32), ("vf_coef", _f32), ("ent_coef", _f32)]


def make_policy_loss_cfg(max_rows):
    """``imgenv_policy_loss_cfg``"""
    c = PolicyLossCfg()
    c.struct_size = C.sizeof(PolicyLossCfg)
    c.max_rows = int(max_rows)
    return c


class ObsPostCfg(C.Structure):
    _fields_ = [("struct_size", _i32), ("flags", _i32), ("avg", _f64 * 7), ("std", _f64 * 7), ("close_dist", _f64)]


class ObsPostOut(C.Structure):
    _fields_ = [("struct_size", _i32), ("n_local", _i32), ("ped_vector_norm", C.c_void_p), ("close_to_human", C.c_void_p)]


def make_obs_post_cfg(ped_norm=True, close=True, avg=PED_NORM_AVG, std=PED_NORM_STD, close_dist=CLOSE_DIST):
    """``imgenv_obs_post_cfg`` with the reference's constants as defaults"""
    c = ObsPostCfg()
    c.struct_size = C.sizeof(ObsPostCfg)
    c.flags = (OBS_PED_NORM if ped_norm else 0) | (OBS_CLOSE if close else 0)
    c.avg[:], c.std[:] = [float(x) for x in avg], [float(x) for x in std]
    c.close_dist = float(close_dist)
    return c


#: imgenv_final_obs_cfg.fields: name -> IMGENV_FINAL_* bit, in bit order.  The first eleven are fields of imgenv_out.
FINAL_BITS = {"vector_states": 1, "sensor_maps": 2, "lasers": 4, "ped_vector_states": 8, "ped_maps": 16, "is_collisions": 32,
              "is_arrives": 64, "step_ds": 128, "ped_min_dists": 256, "view_maps": 512, "lasers_raw": 1024, "stacks": 2048,
              "ped_vector_norm": 4096}
FINAL_IMAGE_STATE, FINAL_ALL = 511, 8191
FINAL_NORM_STATES = 8192  # IMGENV_FINAL_NORM_STATES: after imgenv_normalise_enable only, not part of FINAL_ALL
#: the pointers of imgenv_final_obs_out, in the struct's order
FINAL_ARRAYS = tuple(list(FINAL_BITS)[:11]) + ("stack_sensor_maps", "stack_vector_states", "stack_lasers", "ped_vector_norm", "final_count")
FINAL_BLOCK, FINAL_MAX_BLOCKS = 256, 1024  # k_final_obs' launch shape (csrc/launch_plan.h)


class FinalObsCfg(C.Structure):
    _fields_ = [("struct_size", _i32), ("fields", _i32)]


class FinalObsOut(C.Structure):
    _fields_ = [("struct_size", _i32), ("n_local", _i32)] + [(name, C.c_void_p) for name in FINAL_ARRAYS]


_FINAL_NAMES = dict(FINAL_BITS, norm_states=FINAL_NORM_STATES)


def make_final_obs_cfg(fields):
    """``imgenv_final_obs_cfg``: ``fields`` is an int of IMGENV_FINAL_* bits or an iterable of ``FINAL_BITS`` names (and
    ``"norm_states"``, IMGENV_FINAL_NORM_STATES)"""
    c = FinalObsCfg()
    c.struct_size = C.sizeof(FinalObsCfg)
    if isinstance(fields, (int, np.integer)):
        c.fields = int(fields)
    else:
        names = list(fields)
        unknown = [n for n in names if n not in _FINAL_NAMES]
        if unknown:
            raise ValueError("final observation fields: unknown %s (known: %s)" % (unknown, ", ".join(FINAL_BITS)))
        c.fields = sum({_FINAL_NAMES[n] for n in names})
    return c


#: imgenv_rollout_cfg.fields: name -> IMGENV_ROLLOUT_* bit, in bit order
ROLLOUT_BITS = {"sensor_maps": 1, "vector_states": 2, "lasers": 4, "ped_vector_states": 8, "ped_maps": 16, "ped_vector_norm": 32, "stacks": 64}
ROLLOUT_ALL = 127
#: after imgenv_normalise_enable only, not part of ROLLOUT_ALL: the normalised state (and its stack) as fields; the normalised reward as ``rewards``
ROLLOUT_NORM_STATES, ROLLOUT_NORM_REWARDS = 128, 256
#: not part of ROLLOUT_ALL either (and no name of ROLLOUT_BITS: it excludes ``ped_maps``): the ring keeps no ped_maps, the minibatches
#: draw ``mb_ped_maps`` from the stored ``ped_vector_states`` (imgenv_ped_maps_draw; csrc/ped_draw.h)
ROLLOUT_PED_MAPS_DRAWN = 512
_ROLLOUT_NAMES = dict(ROLLOUT_BITS, norm_states=ROLLOUT_NORM_STATES, norm_rewards=ROLLOUT_NORM_REWARDS, ped_maps_drawn=ROLLOUT_PED_MAPS_DRAWN)
#: the stored observation fields, in the order of imgenv_rollout_out's obs_* and final_* pointers
ROLLOUT_FIELDS = ("sensor_maps", "vector_states", "lasers", "ped_vector_states", "ped_maps", "ped_vector_norm",
                  "stack_sensor_maps", "stack_vector_states", "stack_lasers")
#: ROLLOUT_NORM_STATES' two fields: their ring / final / minibatch pointers are imgenv_normalise_out's (rollout_* / mb_norm_*)
ROLLOUT_NORM_FIELDS = ("norm_vector_states", "norm_state_stack")
#: the other pointers of imgenv_rollout_out, in the struct's order
ROLLOUT_SCALARS = ("actions", "rewards", "dones", "is_clean", "dones_info", "final_idx", "final_slot", "final_row", "final_n")
ROLLOUT_HEADER = ("struct_size", "n_local", "horizon", "final_capacity", "n", "resets")
ROLLOUT_BLOCK, ROLLOUT_MAX_BLOCKS, GAE_BLOCK, GAE_MAX_BLOCKS = 256, 1024, 64, 1024  # the launch shapes (csrc/launch_plan.h)
PED_DRAW_BLOCK, PED_DRAW_MAX_BLOCKS, PED_DRAW_LDS_BYTES = 256, 2048, 65536            # k_ped_draw's (csrc/ped_draw.h)


class RolloutCfg(C.Structure):
    _fields_ = [("struct_size", _i32), ("horizon", _i32), ("final_capacity", _i32), ("fields", _i32)]


class RolloutOut(C.Structure):
    _fields_ = ([(name, _i32) for name in ROLLOUT_HEADER] + [("obs_" + name, C.c_void_p) for name in ROLLOUT_FIELDS] +
                [("final_" + name, C.c_void_p) for name in ROLLOUT_FIELDS] + [(name, C.c_void_p) for name in ROLLOUT_SCALARS])


def make_rollout_cfg(horizon, final_capacity, fields):
    """``imgenv_rollout_cfg``: ``fields`` is an int of IMGENV_ROLLOUT_* bits or an iterable of names: ``ROLLOUT_BITS``', ``"norm_states"``,
    ``"norm_rewards"``, ``"ped_maps_drawn"``"""
    c = RolloutCfg()
    c.struct_size = C.sizeof(RolloutCfg)
    c.horizon, c.final_capacity = int(horizon), int(final_capacity)
    if isinstance(fields, (int, np.integer)):
        c.fields = int(fields)
    else:
        names = list(fields)
        unknown = [n for n in names if n not in _ROLLOUT_NAMES]
        if unknown:
            raise ValueError("rollout fields: unknown %s (known: %s)" % (unknown, ", ".join(_ROLLOUT_NAMES)))
        c.fields = sum({_ROLLOUT_NAMES[n] for n in names})
    return c


#: rollout minibatches (imgenv_rollout_minibatch_enable; csrc/minibatch.h)
MB_MAX_SCALARS, MB_MAX_BUFFERS = 6, 4
#: the launch shapes and the shuffle's rounds (csrc/launch_plan.h)
MB_INDEX_BLOCK, MB_LANE_FLAGS, MB_TILE, MB_SCAN_BLOCK, MB_STATS_BLOCK, MB_STATS_PER_LANE, MB_SHUFFLE_BLOCK, MB_ROUNDS = 256, 16, 4096, 256, 256, 16, 256, 6
#: the per-transition arrays of imgenv_minibatch_buffer behind its mb_<field> pointers, in the struct's order
MB_SCALARS = ("mb_actions", "mb_rewards", "mb_dones", "mb_dones_info", "mb_index", "mb_weight", "mb_scalars")
MB_HEADER = ("struct_size", "n_local", "horizon", "batch", "buffers", "fields")
#: the handle-wide pointers of imgenv_minibatch_out, in the struct's order
MB_ARRAYS = ("valid", "order", "valid_n", "norm", "tile_count", "tile_base", "stat_part", "stat_mean")


class MinibatchCfg(C.Structure):
    _fields_ = [("struct_size", _i32), ("batch", _i32), ("buffers", _i32), ("fields", _i32)]


class MinibatchBuffer(C.Structure):
    _fields_ = [("mb_" + name, C.c_void_p) for name in ROLLOUT_FIELDS] + [(name, C.c_void_p) for name in MB_SCALARS]


class MinibatchOut(C.Structure):
    _fields_ = [(name, _i32) for name in MB_HEADER] + [(name, C.c_void_p) for name in MB_ARRAYS] + [("buf", MinibatchBuffer * MB_MAX_BUFFERS)]


class MinibatchArgs(C.Structure):
    _fields_ = [("struct_size", _i32), ("j", _i32), ("buffer", _i32), ("n_scalars", _i32), ("normalise", _i32), ("reserved", _i32),
                ("scalars", C.c_void_p * MB_MAX_SCALARS), ("norm", C.c_void_p)]


def make_minibatch_cfg(batch, buffers=1, fields=0):
    """``imgenv_minibatch_cfg``: ``fields`` is an int of IMGENV_ROLLOUT_* bits (0: every field the rollout stores) or an iterable
    of the names ``make_rollout_cfg`` takes"""
    c = MinibatchCfg()
    c.struct_size = C.sizeof(MinibatchCfg)
    c.batch, c.buffers = int(batch), int(buffers)
    if fields is None:
        fields = 0
    if isinstance(fields, (int, np.integer)):
        c.fields = int(fields)
    else:
        names = list(fields)
        unknown = [n for n in names if n not in _ROLLOUT_NAMES]
        if unknown:
            raise ValueError("minibatch fields: unknown %s (known: %s)" % (unknown, ", ".join(_ROLLOUT_NAMES)))
        c.fields = sum({_ROLLOUT_NAMES[n] for n in names})
    return c


#: sequence minibatches (imgenv_rollout_seq_enable; csrc/sequences.h)
SEQ_MAX_STATES, SEQ_MAX_STATE_BYTES, SEQ_FLAG_BLOCK = 2, 65536, 256
#: the arrays of imgenv_seq_buffer behind its mb_<field> pointers (the normalised fields' included), in the struct's order
SEQ_SCALARS = ("mb_actions", "mb_rewards", "mb_dones", "mb_dones_info", "mb_index", "mb_weight", "mb_first", "mb_scalars", "mb_seq", "mb_seq_len",
               "mb_seq_state")
SEQ_HEADER = ("struct_size", "n_local", "horizon", "length", "batch", "buffers", "fields", "max_sequences", "state_bytes")
#: the handle-wide pointers of imgenv_seq_out, in the struct's order
SEQ_ARRAYS = ("seq_flag", "seq_valid", "seq_order", "seq_valid_n", "tile_count", "tile_base")


class SeqCfg(C.Structure):
    _fields_ = [("struct_size", _i32), ("length", _i32), ("batch", _i32), ("buffers", _i32), ("fields", _i32), ("state_bytes", _i32 * SEQ_MAX_STATES),
                ("reserved", _i32)]


class SeqBuffer(C.Structure):
    _fields_ = ([("mb_" + name, C.c_void_p) for name in ROLLOUT_FIELDS + ROLLOUT_NORM_FIELDS] + [(name, C.c_void_p) for name in SEQ_SCALARS[:-1]] +
                [("mb_seq_state", C.c_void_p * SEQ_MAX_STATES)])


class SeqOut(C.Structure):
    _fields_ = ([(name, _i32) for name in SEQ_HEADER[:-1]] + [("state_bytes", _i32 * SEQ_MAX_STATES)] + [(name, C.c_void_p) for name in SEQ_ARRAYS] +
                [("buf", SeqBuffer * MB_MAX_BUFFERS)])


class SeqArgs(C.Structure):
    _fields_ = [("struct_size", _i32), ("j", _i32), ("buffer", _i32), ("n_scalars", _i32), ("normalise", _i32), ("reserved", _i32),
                ("scalars", C.c_void_p * MB_MAX_SCALARS), ("norm", C.c_void_p), ("states", C.c_void_p * SEQ_MAX_STATES)]


def make_seq_cfg(length, batch, buffers=1, fields=0, state_bytes=()):
    """``imgenv_seq_cfg``: ``fields`` as ``make_minibatch_cfg`` takes them; ``state_bytes``: up to 2 row sizes of the caller's state arrays"""
    c = SeqCfg()
    c.struct_size = C.sizeof(SeqCfg)
    c.length, c.batch, c.buffers = int(length), int(batch), int(buffers)
    c.fields = make_minibatch_cfg(1, 1, fields).fields
    state_bytes = list(state_bytes)
    if len(state_bytes) > SEQ_MAX_STATES:
        raise ValueError("sequences: at most %d state arrays" % SEQ_MAX_STATES)
    for a, nb in enumerate(state_bytes):
        c.state_bytes[a] = int(nb)
    return c


def make_seq_args(j, buffer=0, scalars=(), normalise=-1, norm=None, states=()):
    """``imgenv_seq_args``: ``scalars`` and ``states`` device addresses (ints), ``norm`` one or None"""
    a = SeqArgs()
    a.struct_size = C.sizeof(SeqArgs)
    a.j, a.buffer, a.n_scalars, a.normalise = int(j), int(buffer), len(scalars), int(normalise)
    for s, ptr in enumerate(scalars[:MB_MAX_SCALARS]):
        a.scalars[s] = ptr
    a.norm = norm
    for q, ptr in enumerate(states[:SEQ_MAX_STATES]):
        a.states[q] = ptr
    return a


#: running normalisation (imgenv_normalise_enable; csrc/normalise.h)
NORM_OBS, NORM_REWARD = 1, 2
NORM_BLOCK, NORM_PER_LANE, NORM_MAX_COLS, NORM_MAX_BLOCKS = 256, 8, 64, 1024  # the launch shapes (csrc/launch_plan.h)


class NormaliseCfg(C.Structure):
    _fields_ = [("struct_size", _i32), ("flags", _i32), ("gamma", C.c_double), ("clip_obs", C.c_double), ("clip_reward", C.c_double),
                ("eps", C.c_double)]


class NormaliseOut(C.Structure):
    _fields_ = [("struct_size", _i32), ("n_local", _i32), ("state_dim", _i32), ("state_depth", _i32), ("norm_vector_states", C.c_void_p),
                ("norm_state_stack", C.c_void_p), ("norm_rewards", C.c_void_p), ("stats", C.c_void_p), ("returns", C.c_void_p),
                ("stats_word", _i32), ("returns_word", _i32), ("training", _i32), ("reserved", _i32),
                ("rollout_obs_norm_vector_states", C.c_void_p), ("rollout_obs_norm_state_stack", C.c_void_p),
                ("rollout_final_norm_vector_states", C.c_void_p), ("rollout_final_norm_state_stack", C.c_void_p),
                ("mb_norm_vector_states", C.c_void_p * 4), ("mb_norm_state_stack", C.c_void_p * 4),  # (MB_MAX_BUFFERS)
                ("final_norm_vector_states", C.c_void_p), ("final_norm_state_stack", C.c_void_p)]


class NormaliseStats(C.Structure):
    _fields_ = [("struct_size", _i32), ("state_dim", _i32), ("n_rows", _i32), ("reserved", _i32), ("obs_count", C.c_double),
                ("ret_count", C.c_double), ("ret_mean", C.c_double), ("ret_var", C.c_double), ("obs_mean", C.c_void_p),
                ("obs_var", C.c_void_p), ("returns", C.c_void_p)]


def make_normalise_cfg(obs=True, reward=True, gamma=0.99, clip_obs=10.0, clip_reward=10.0, eps=1e-8):
    """``imgenv_normalise_cfg`` (the defaults are Stable-Baselines3's VecNormalize's)"""
    c = NormaliseCfg()
    c.struct_size = C.sizeof(NormaliseCfg)
    c.flags = (NORM_OBS if obs else 0) | (NORM_REWARD if reward else 0)
    c.gamma, c.clip_obs, c.clip_reward, c.eps = float(gamma), float(clip_obs), float(clip_reward), float(eps)
    return c


def make_normalise_stats(state_dim, n_rows, stats=None):
    """``imgenv_normalise_stats`` over fresh numpy arrays: ``(struct, arrays)``; ``stats``: a dict as ``World.normalise_stats()``
    returns, copied in"""
    arrays = {"obs_mean": np.zeros(state_dim, np.float64), "obs_var": np.ones(state_dim, np.float64), "returns": np.zeros(n_rows, np.float64)}
    s = NormaliseStats()
    s.struct_size = C.sizeof(NormaliseStats)
    s.state_dim, s.n_rows = int(state_dim), int(n_rows)
    s.obs_count = s.ret_count = 1e-4
    s.ret_var = 1.0
    if stats is not None:
        for name, a in arrays.items():
            a[...] = np.asarray(stats[name], np.float64).reshape(a.shape)
        s.obs_count, s.ret_count, s.ret_mean, s.ret_var = (float(stats[k]) for k in ("obs_count", "ret_count", "ret_mean", "ret_var"))
    s.obs_mean, s.obs_var, s.returns = (arrays[k].ctypes.data for k in ("obs_mean", "obs_var", "returns"))
    return s, arrays


def make_minibatch_args(j, buffer=0, scalars=(), normalise=-1, norm=None):
    """``imgenv_minibatch_args``: ``scalars`` device addresses (ints), ``norm`` one or None"""
    a = MinibatchArgs()
    a.struct_size = C.sizeof(MinibatchArgs)
    a.j, a.buffer, a.n_scalars, a.normalise = int(j), int(buffer), len(scalars), int(normalise)
    for s, ptr in enumerate(scalars[:MB_MAX_SCALARS]):
        a.scalars[s] = ptr
    a.norm = norm
    return a


#: name -> (numpy dtype, shape as a function of the Out header and the world sizes)
def out_layout(o, n_peds, hp, wp):
    R, B = o.n_local, max(o.n_beams, 1)
    return {
        "vector_states": (np.float32, (R, o.state_dim)),
        "view_maps": (np.uint8, (R, o.view_h, o.view_w)),
        "sensor_maps": (np.float16, (R, o.image_h, o.image_w)),
        "lasers_raw": (np.float32, (R, B)),
        "lasers": (np.float64, (R, B)),
        "ped_vector_states": (np.float32, (R, o.ped_vec_len)),
        "ped_maps": (np.float32, (R, 3, hp, wp)),
        "is_collisions": (np.int8, (R,)),
        "is_arrives": (np.uint8, (R,)),
        "step_ds": (np.float64, (R,)),
        "ped_min_dists": (np.float64, (R,)),
        "base_rewards": (np.int32, (R,)),
        "base_dones": (np.uint8, (R,)),
        "rewards": (np.float64, (R,)),
        "paper_rewards": (np.float64, (R,)),
        "dones": (np.uint8, (R,)),
        "dones_info": (np.int32, (R,)),
        "is_clean": (np.uint8, (R,)),
        "robot_pose": (np.float64, (R, 3)),
        "ped_state": (np.float64, (max(n_peds, 1), 4)),
        "counters": (np.int32, (4,)),
        "step_rewards": (np.float64, (R,)),
        "step_dones": (np.uint8, (R,)),
        "step_dones_info": (np.int32, (R,)),
        "step_is_clean": (np.uint8, (R,)),
        "step_is_arrives": (np.uint8, (R,)),
        "step_is_collisions": (np.int8, (R,)),
        "step_all_down": (np.uint8, (R,)),
        "hits_x": (np.float32, (R, B)),          # AgentState's remaining fields: null pointers unless FLAG_AGENT_STATE_EXTRAS
        "hits_y": (np.float32, (R, B)),
        "angular_map": (np.float32, (R, ANGULAR_BINS)),
    }


def _keep(arr, dtype):
    return np.ascontiguousarray(arr, dtype=dtype)


def _ptr(arr, ctype):
    return arr.ctypes.data_as(C.POINTER(ctype))


def make_cfg(p):
    """Build a :class:`Cfg` from a plain dict of python/numpy values (see ``World``).

    Returns ``(cfg, keepalive)``; ``keepalive`` owns the numpy buffers the struct points into.
    """
    R, P = int(p["n_robots"]), int(p["n_peds"])
    keep = {
        "robot_shape": _keep(p["robot_shape"], np.int32).reshape(R),
        "robot_size": _keep(p["robot_size"], np.float32).reshape(R, 4),
        "robot_sensor_cfg": _keep(p.get("robot_sensor_cfg", np.zeros((R, 2))), np.float32).reshape(R, 2),
        "ped_shape": _keep(p.get("ped_shape", np.zeros(P)), np.int32).reshape(P),
        "ped_size": _keep(p.get("ped_size", np.zeros((P, 6))), np.float32).reshape(P, 6),
        "ped_max_speed": _keep(p.get("ped_max_speed", np.zeros(P)), np.float32).reshape(P),
        "robot_size_last": _keep(p["robot_size_last"], np.float64).reshape(R),
    }
    c = Cfg()
    c.abi_version = ABI_VERSION
    c.struct_size = C.sizeof(Cfg)
    for k in ("view_resolution", "view_width", "view_height", "step_hz", "view_angle_begin", "view_angle_end",
              "view_min_dist", "view_max_dist", "global_resolution"):
        setattr(c, k, float(p[k]))
    c.beep_r = float(p.get("beep_r", 0.0))
    c.ped_ca_p = float(p.get("ped_ca_p", 0.0))
    for k in ("state_dim", "use_laser", "range_total", "relation_ped_robo", "ped_scene_type", "robot_ktype",
              "max_ped", "time_max"):
        setattr(c, k, int(p[k]))
    c.n_robots, c.n_peds = R, P
    c.ped_vec_dim = int(p.get("ped_vec_dim", 7))
    c.laser_norm = int(bool(p.get("laser_norm", True)))
    c.image_size[0], c.image_size[1] = int(p["image_size"][0]), int(p["image_size"][1])
    c.ped_image_size[0], c.ped_image_size[1] = int(p["ped_image_size"][0]), int(p["ped_image_size"][1])
    c.ped_image_r = float(p["ped_image_r"])
    c.laser_max = float(p["laser_max"])
    c.ped_safety_space = float(p["ped_safety_space"])
    for name in ("limiter_v", "limiter_w"):
        lim, src = getattr(c, name), p.get(name) or {}
        lim.has_velocity_limits = int(bool(src.get("has_velocity_limits", False)))
        lim.has_acceleration_limits = int(bool(src.get("has_acceleration_limits", False)))
        lim.has_jerk_limits = int(bool(src.get("has_jerk_limits", False)))
        for f in ("min_velocity", "max_velocity", "min_acceleration", "max_acceleration", "min_jerk", "max_jerk"):
            setattr(lim, f, float(src.get(f, 0.0)))
    c.robot_shape = _ptr(keep["robot_shape"], C.c_int32)
    c.robot_size = _ptr(keep["robot_size"], C.c_float)
    c.robot_sensor_cfg = _ptr(keep["robot_sensor_cfg"], C.c_float)
    c.ped_shape = _ptr(keep["ped_shape"], C.c_int32)
    c.ped_size = _ptr(keep["ped_size"], C.c_float)
    c.ped_max_speed = _ptr(keep["ped_max_speed"], C.c_float)
    c.robot_size_last = _ptr(keep["robot_size_last"], C.c_double)
    c.robot_begin = int(p.get("robot_begin", 0))
    c.robot_end = int(p.get("robot_end", R))
    c.device = int(p.get("device", 0))
    c.flags = int(p.get("flags", 0))
    c.n_worlds = int(p.get("n_worlds", 1))
    c.out_arena = None
    c.out_arena_bytes = 0
    return c, keep


def make_reset_batch(b, n_robots, n_peds):
    """``b``: dict with obstacles / robot / ped arrays (see ``worldgen.ResetLayout.as_batch``)."""
    nob = int(len(b.get("obs_shape", ())))
    P = n_peds
    cap = int(b.get("ped_traj_cap", 2))
    keep = {
        "obs_shape": _keep(b.get("obs_shape", np.zeros(0)), np.int32).reshape(nob),
        "obs_size": _keep(b.get("obs_size", np.zeros((0, 4))), np.float32).reshape(nob, 4),
        "obs_pose": _keep(b.get("obs_pose", np.zeros((0, 4))), np.float64).reshape(nob, 4),
        "robot_pose": _keep(b["robot_pose"], np.float64).reshape(n_robots, 4),
        "robot_goal": _keep(b["robot_goal"], np.float64).reshape(n_robots, 2),
        "ped_pose": _keep(b.get("ped_pose", np.zeros((P, 4))), np.float64).reshape(P, 4),
        "ped_goal": _keep(b.get("ped_goal", np.zeros((P, 2))), np.float64).reshape(P, 2),
        "ped_traj_len": _keep(b.get("ped_traj_len", np.zeros(P)), np.int32).reshape(P),
        "ped_traj": _keep(b.get("ped_traj", np.zeros((P, cap, 3))), np.float64).reshape(P, cap, 3),
    }
    r = ResetBatch()
    r.struct_size = C.sizeof(ResetBatch)
    r.n_obstacles = nob
    r.obs_shape = _ptr(keep["obs_shape"], C.c_int32)
    r.obs_size = _ptr(keep["obs_size"], C.c_float)
    r.obs_pose = _ptr(keep["obs_pose"], C.c_double)
    r.robot_pose = _ptr(keep["robot_pose"], C.c_double)
    r.robot_goal = _ptr(keep["robot_goal"], C.c_double)
    r.ped_pose = _ptr(keep["ped_pose"], C.c_double)
    r.ped_goal = _ptr(keep["ped_goal"], C.c_double)
    r.ped_traj_len = _ptr(keep["ped_traj_len"], C.c_int32)
    r.ped_traj = _ptr(keep["ped_traj"], C.c_double)
    r.ped_traj_cap = cap
    r.ignore_obstacle = int(bool(b.get("ignore_obstacle", False)))
    if b.get("ped_traj_v") is not None:  # dataset scene: recorded velocities beside the recorded positions
        keep["ped_traj_v"] = _keep(b["ped_traj_v"], np.float64).reshape(P, cap, 2)
        r.ped_traj_v = _ptr(keep["ped_traj_v"], C.c_double)
    return r, keep


#: every symbol include/imgenv.h declares
SYMBOLS = ("imgenv_backend", "imgenv_abi_version", "imgenv_last_error", "imgenv_create", "imgenv_arena_bytes",
           "imgenv_destroy", "imgenv_reset", "imgenv_step", "imgenv_step_begin", "imgenv_step_end",
           "imgenv_records", "imgenv_outputs", "imgenv_step_launches", "imgenv_timing", "imgenv_timing_read",
           "imgenv_kernel_name", "imgenv_comm_unique_id", "imgenv_comm_init", "imgenv_comm_info", "imgenv_reset_world", "imgenv_reset_worlds", "imgenv_spawn",
           "imgenv_reset_worlds_spawn", "imgenv_step_autoreset", "imgenv_step_autoreset_device", "imgenv_autoreset_last",
           "imgenv_world_placement", "imgenv_cv_resize_u8", "imgenv_build_id", "imgenv_step_flags", "imgenv_layer_mode",
           "imgenv_stack_bytes", "imgenv_stack_enable", "imgenv_stack_outputs",
           "imgenv_episodes_enable", "imgenv_episodes_outputs", "imgenv_episodes_clear",
           "imgenv_episode_log_enable", "imgenv_episode_log_outputs", "imgenv_episode_log_read",
           "imgenv_actions_enable", "imgenv_actions_outputs", "imgenv_actions_decode", "imgenv_obs_post_enable", "imgenv_obs_post_outputs",
           "imgenv_policy_enable", "imgenv_policy_outputs", "imgenv_policy_sample",
           "imgenv_policy_loss_enable", "imgenv_policy_loss_outputs", "imgenv_policy_loss",
           "imgenv_final_obs_enable", "imgenv_final_obs_outputs",
           "imgenv_rollout_enable", "imgenv_rollout_outputs", "imgenv_rollout_begin", "imgenv_rollout_gae", "imgenv_ped_maps_draw",
           "imgenv_rollout_minibatch_enable", "imgenv_rollout_minibatch_outputs", "imgenv_rollout_index", "imgenv_rollout_stats",
           "imgenv_rollout_shuffle", "imgenv_rollout_minibatch",
           "imgenv_rollout_seq_enable", "imgenv_rollout_seq_outputs", "imgenv_rollout_seq_index", "imgenv_rollout_seq_shuffle",
           "imgenv_rollout_seq_minibatch",
           "imgenv_normalise_enable", "imgenv_normalise_outputs", "imgenv_normalise_training", "imgenv_normalise_stats_get",
           "imgenv_normalise_stats_set",
           "imgenv_maps_add", "imgenv_world_maps_set", "imgenv_maps_policy", "imgenv_map_for_placement", "imgenv_world_maps",
           "imgenv_tracks_add", "imgenv_world_tracks_set", "imgenv_tracks_policy", "imgenv_tracks_for_placement", "imgenv_world_tracks",
           "imgenv_scenarios_add", "imgenv_scenarios_policy", "imgenv_scenario_for_placement", "imgenv_reset_worlds_scenarios",
           "imgenv_world_scenarios")
K_COUNT = 14


def library_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libimgenv_hip.so")


_LIB = None


def bind(lib):
    """Attach argtypes / restypes of include/imgenv.h to a loaded CDLL."""
    lib.imgenv_backend.restype = C.c_char_p
    lib.imgenv_build_id.restype = C.c_char_p
    lib.imgenv_abi_version.restype = C.c_int32
    lib.imgenv_last_error.restype = C.c_char_p
    lib.imgenv_create.argtypes = [C.POINTER(Cfg), C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    lib.imgenv_arena_bytes.argtypes = [C.POINTER(Cfg)]
    lib.imgenv_arena_bytes.restype = C.c_int64
    lib.imgenv_destroy.argtypes = [C.c_void_p]
    lib.imgenv_destroy.restype = None
    lib.imgenv_reset.argtypes = [C.c_void_p, C.POINTER(ResetBatch), C.c_void_p]
    lib.imgenv_reset_world.argtypes = [C.c_void_p, C.c_int32, C.POINTER(ResetBatch), C.c_void_p]
    lib.imgenv_reset_worlds.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(ResetBatch), C.c_void_p]
    lib.imgenv_spawn.argtypes = [C.POINTER(SpawnCfg), C.c_uint64] + [C.c_void_p] * 9
    lib.imgenv_step_autoreset_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(SpawnCfg), C.c_uint64, C.c_void_p]
    lib.imgenv_autoreset_last.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.c_void_p]
    lib.imgenv_world_placement.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_uint64)] + [C.c_void_p] * 9
    lib.imgenv_reset_worlds_spawn.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(SpawnCfg),
                                              C.POINTER(C.c_uint64), C.c_void_p]
    lib.imgenv_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.imgenv_step_flags.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.imgenv_step_autoreset.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(SpawnCfg), C.c_uint64, C.POINTER(C.c_int32), C.c_int32,
                                          C.POINTER(C.c_int32), C.c_void_p]
    lib.imgenv_step_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.imgenv_step_end.argtypes = [C.c_void_p, C.c_void_p]
    lib.imgenv_records.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    lib.imgenv_outputs.argtypes = [C.c_void_p, C.POINTER(Out)]
    lib.imgenv_step_launches.argtypes = [C.c_void_p]
    lib.imgenv_layer_mode.argtypes = [C.c_void_p]
    lib.imgenv_timing.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.imgenv_timing_read.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.imgenv_comm_unique_id.argtypes = [C.c_void_p]
    lib.imgenv_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
    lib.imgenv_comm_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.imgenv_cv_resize_u8.argtypes = [C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]
    lib.imgenv_stack_bytes.argtypes = [C.POINTER(Cfg), C.POINTER(StackCfg)]
    lib.imgenv_stack_bytes.restype = C.c_int64
    lib.imgenv_stack_enable.argtypes = [C.c_void_p, C.POINTER(StackCfg), C.POINTER(StackOut)]
    lib.imgenv_stack_outputs.argtypes = [C.c_void_p, C.POINTER(StackOut)]
    lib.imgenv_episodes_enable.argtypes = [C.c_void_p, C.POINTER(EpisodesCfg), C.POINTER(EpisodesOut)]
    lib.imgenv_episodes_outputs.argtypes = [C.c_void_p, C.POINTER(EpisodesOut)]
    lib.imgenv_episodes_clear.argtypes = [C.c_void_p, C.c_void_p]
    lib.imgenv_episode_log_enable.argtypes = [C.c_void_p, C.POINTER(EpisodeLogCfg), C.POINTER(EpisodeLogOut)]
    lib.imgenv_episode_log_outputs.argtypes = [C.c_void_p, C.POINTER(EpisodeLogOut)]
    lib.imgenv_episode_log_read.argtypes = [C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p]
    lib.imgenv_episode_log_read.restype = C.c_int64
    lib.imgenv_actions_enable.argtypes = [C.c_void_p, C.POINTER(ActionsCfg), C.POINTER(ActionsOut)]
    lib.imgenv_actions_outputs.argtypes = [C.c_void_p, C.POINTER(ActionsOut)]
    lib.imgenv_actions_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.imgenv_policy_enable.argtypes = [C.c_void_p, C.POINTER(PolicyCfg), C.POINTER(PolicyOut)]
    lib.imgenv_policy_outputs.argtypes = [C.c_void_p, C.POINTER(PolicyOut)]
    lib.imgenv_policy_sample.argtypes = [C.c_void_p, C.POINTER(PolicyArgs), C.c_void_p]
    lib.imgenv_policy_loss_enable.argtypes = [C.c_void_p, C.POINTER(PolicyLossCfg), C.POINTER(PolicyLossOut)]
    lib.imgenv_policy_loss_outputs.argtypes = [C.c_void_p, C.POINTER(PolicyLossOut)]
    lib.imgenv_policy_loss.argtypes = [C.c_void_p, C.POINTER(PolicyLossArgs), C.c_void_p]
    lib.imgenv_obs_post_enable.argtypes = [C.c_void_p, C.POINTER(ObsPostCfg), C.POINTER(ObsPostOut)]
    lib.imgenv_obs_post_outputs.argtypes = [C.c_void_p, C.POINTER(ObsPostOut)]
    lib.imgenv_final_obs_enable.argtypes = [C.c_void_p, C.POINTER(FinalObsCfg), C.POINTER(FinalObsOut)]
    lib.imgenv_final_obs_outputs.argtypes = [C.c_void_p, C.POINTER(FinalObsOut)]
    lib.imgenv_rollout_enable.argtypes = [C.c_void_p, C.POINTER(RolloutCfg), C.POINTER(RolloutOut)]
    lib.imgenv_rollout_outputs.argtypes = [C.c_void_p, C.POINTER(RolloutOut)]
    lib.imgenv_rollout_begin.argtypes = [C.c_void_p, C.c_void_p]
    lib.imgenv_rollout_gae.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.imgenv_ped_maps_draw.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.imgenv_rollout_minibatch_enable.argtypes = [C.c_void_p, C.POINTER(MinibatchCfg), C.POINTER(MinibatchOut)]
    lib.imgenv_rollout_minibatch_outputs.argtypes = [C.c_void_p, C.POINTER(MinibatchOut)]
    lib.imgenv_rollout_index.argtypes = [C.c_void_p, C.c_void_p]
    lib.imgenv_rollout_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    lib.imgenv_rollout_shuffle.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.imgenv_rollout_minibatch.argtypes = [C.c_void_p, C.POINTER(MinibatchArgs), C.c_void_p]
    lib.imgenv_rollout_seq_enable.argtypes = [C.c_void_p, C.POINTER(SeqCfg), C.POINTER(SeqOut)]
    lib.imgenv_rollout_seq_outputs.argtypes = [C.c_void_p, C.POINTER(SeqOut)]
    lib.imgenv_rollout_seq_index.argtypes = [C.c_void_p, C.c_void_p]
    lib.imgenv_rollout_seq_shuffle.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.imgenv_rollout_seq_minibatch.argtypes = [C.c_void_p, C.POINTER(SeqArgs), C.c_void_p]
    lib.imgenv_normalise_enable.argtypes = [C.c_void_p, C.POINTER(NormaliseCfg), C.POINTER(NormaliseOut)]
    lib.imgenv_normalise_outputs.argtypes = [C.c_void_p, C.POINTER(NormaliseOut)]
    lib.imgenv_normalise_training.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.imgenv_normalise_stats_get.argtypes = [C.c_void_p, C.POINTER(NormaliseStats)]
    lib.imgenv_normalise_stats_set.argtypes = [C.c_void_p, C.POINTER(NormaliseStats)]
    lib.imgenv_maps_add.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]
    lib.imgenv_world_maps_set.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]
    lib.imgenv_maps_policy.argtypes = [C.c_void_p, C.c_int32]
    lib.imgenv_map_for_placement.argtypes = [C.c_uint64, C.c_int32]
    lib.imgenv_map_for_placement.restype = C.c_int32
    lib.imgenv_world_maps.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]
    lib.imgenv_tracks_add.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.imgenv_world_tracks_set.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]
    lib.imgenv_tracks_policy.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.imgenv_tracks_for_placement.argtypes = [C.c_uint64, C.c_int32]
    lib.imgenv_tracks_for_placement.restype = C.c_int32
    lib.imgenv_world_tracks.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]
    lib.imgenv_scenarios_add.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 9
    lib.imgenv_scenarios_policy.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p]
    lib.imgenv_scenario_for_placement.argtypes = [C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32]
    lib.imgenv_scenario_for_placement.restype = C.c_int32
    lib.imgenv_reset_worlds_scenarios.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]
    lib.imgenv_world_scenarios.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]
    lib.imgenv_kernel_name.argtypes = [C.c_int]
    lib.imgenv_kernel_name.restype = C.c_char_p
    return lib


def map_for_placement(seed, n_maps):
    """``imgenv_map_for_placement``: the map an episode placed from ``seed`` runs on under the "placement" policy (needs no GPU)"""
    return int(load_library().imgenv_map_for_placement(C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(n_maps)))


def tracks_for_placement(seed, n_sets):
    """``imgenv_tracks_for_placement``: the track set an episode placed from ``seed`` replays under the "placement" policy (needs no GPU)"""
    return int(load_library().imgenv_tracks_for_placement(C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(n_sets)))


def scenario_for_placement(policy, seed0, first, n, n_scenarios):
    """``imgenv_scenario_for_placement``: the scenario placement number ``n`` replays under ``policy`` ("queue": ``(first + n) %
    n_scenarios``; "placement": a draw from ``seed0 + n``; "off": -1).  Needs no GPU."""
    m = 0xFFFFFFFFFFFFFFFF
    code = SCENARIO_POLICIES[policy] if isinstance(policy, str) else int(policy)
    return int(load_library().imgenv_scenario_for_placement(code, C.c_uint64(int(seed0) & m), C.c_uint64(int(first) & m), C.c_uint64(int(n) & m),
                                                            int(n_scenarios)))


#: the arrays of one recorded episode, in the order of ``imgenv_spawn`` / ``imgenv_scenarios_add``: name -> (dtype, shape per episode)
def scenario_arrays(R, P, O):
    return {"robot_pose": (np.float64, (R, 4)), "robot_goal": (np.float64, (R, 2)), "ped_pose": (np.float64, (P, 4)),
            "ped_goal": (np.float64, (P, 2)), "ped_traj": (np.float64, (P, 2, 3)), "ped_traj_len": (np.int32, (P,)),
            "obs_shape": (np.int32, (O,)), "obs_size": (np.float32, (O, 4)), "obs_pose": (np.float64, (O, 4))}


def pack_scenarios(layouts, R, P, O):
    """The arrays of ``imgenv_scenarios_add`` from a list of recorded episodes -- the layout objects ``spawn.native_spawn`` /
    ``EnvPos.reset`` return (or dicts with the same fields): a dict name -> array with a leading ``[n]`` axis, in the order of the C
    prototype.  Every episode must hold ``R`` robots, ``P`` pedestrians with trajectories of at most two points and ``O``
    obstacles: one cast per bank."""
    layouts = list(layouts)
    if not layouts:
        raise ValueError("no scenarios")
    spec = scenario_arrays(R, P, O)
    out = {k: np.zeros((len(layouts),) + shape, dt) for k, (dt, shape) in spec.items()}
    for s, lay in enumerate(layouts):
        get = (lambda k: lay.get(k)) if isinstance(lay, dict) else (lambda k: getattr(lay, k, None))
        for k, (dt, shape) in spec.items():
            v = get(k)
            if v is None:
                v = np.zeros(shape, dt)
            v = np.asarray(v)
            if k == "ped_traj" and v.ndim == 3 and v.shape[0] == P and v.shape[1] == 1:  # a one-point trajectory: the second is zero
                v = np.concatenate([v, np.zeros_like(v)], axis=1)
            if v.size != int(np.prod(shape)) or (v.ndim > 1 and v.shape != shape):
                raise ValueError("scenario %d: %s is %s, the bank's cast needs %s (%d robots, %d pedestrians, %d obstacles)"
                                 % (s, k, v.shape, shape, R, P, O))
            out[k][s] = v.reshape(shape)
    return out


def pack_track_sets(sets, n_peds):
    """The arrays of ``imgenv_tracks_add`` from a list of sets.  A set is ``[P, T, 5]`` rows (x, y, yaw, vx, vy) per pedestrian and
    step -- what ``PedTrajectoryDatasetWrapper.change_world()`` hands out, every series its full length -- or a dict / pair
    ``(series, lengths)`` with ``lengths[P]`` the true length of each right-padded series.  Sets are right-padded to the longest
    ``T``.  Returns ``(n_sets, cap, ped_pose [n, P, 4], ped_traj [n, P, cap, 3], ped_traj_v [n, P, cap, 2], ped_traj_len [n, P])``;
    the start pose is the first row, its quaternion ``(sin(yaw / 2), cos(yaw / 2))`` as in ``spawn.init_ped_dataset``."""
    items = []
    for one in sets:
        if isinstance(one, dict):
            d, ln = one["series"], one.get("lengths")
        elif isinstance(one, tuple) and len(one) == 2:
            d, ln = one
        else:
            d, ln = one, None
        d = np.asarray(d, np.float64)
        if d.ndim != 3 or d.shape[0] != n_peds or d.shape[2] != 5 or d.shape[1] < 1:
            raise ValueError("a track set is [%d pedestrians, steps, 5]; got %s" % (n_peds, d.shape))
        ln = np.full(n_peds, d.shape[1], np.int32) if ln is None else np.asarray(ln, np.int32).reshape(n_peds)
        if (ln < 1).any() or (ln > d.shape[1]).any():
            raise ValueError("track lengths must lie in [1, %d]" % d.shape[1])
        items.append((d, ln))
    if not items:
        raise ValueError("no track sets")
    n, cap = len(items), max(d.shape[1] for d, _ in items)
    pose, traj = np.zeros((n, n_peds, 4)), np.zeros((n, n_peds, cap, 3))
    traj_v, length = np.zeros((n, n_peds, cap, 2)), np.zeros((n, n_peds), np.int32)
    for s, (d, ln) in enumerate(items):
        T = d.shape[1]
        traj[s, :, :T], traj_v[s, :, :T], length[s] = d[:, :, :3], d[:, :, 3:5], ln
        pose[s, :, 0], pose[s, :, 1] = d[:, 0, 0], d[:, 0, 1]
        pose[s, :, 2], pose[s, :, 3] = np.sin(d[:, 0, 2] / 2.0), np.cos(d[:, 0, 2] / 2.0)
    return n, cap, pose, traj, traj_v, length


def load_library():
    """Load the HIP extension.  Raises (never falls back) when it is missing or mismatched."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            "img_env_amd: HIP extension %s is missing -- run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950).  There is no CPU fallback." % path)
    lib = C.CDLL(path)
    for s in SYMBOLS:
        if not hasattr(lib, s):
            raise RuntimeError("img_env_amd: %s does not export %s" % (path, s))
    bind(lib)
    if lib.imgenv_abi_version() != ABI_VERSION:
        raise RuntimeError("img_env_amd: ABI mismatch: library %d, python %d" % (lib.imgenv_abi_version(), ABI_VERSION))
    _LIB = lib
    return lib
