/*
 * imgenv.h -- C ABI of the MI355X-native batched img_env step() path.
 *
 * This is the drop-in boundary.  In the reference the step() path sits behind four ROS
 * services advertised by EnvService (reference src/img_env/src/img_env.cpp:716-754):
 *
 *   ~init_image_env   (src/comn_pkg/srv/InitEnv.srv:1-21)   -> imgenv_create()
 *   ~reset_image_env  (src/comn_pkg/srv/ResetEnv.srv:1-8)   -> imgenv_reset()
 *   ~step_image_env   (src/comn_pkg/srv/StepEnv.srv:1-5)    -> imgenv_step()
 *   ~ep_end_image_env (src/comn_pkg/srv/EndEp.srv)          -> per-episode results: imgenv_episode_log_*; trajectories: out of scope
 *
 * and the Python post-processing of the response (reference envs/env/yaml_env.py:392-481,
 * envs/wrapper/base.py:153-254) which this library also performs on the device, so the
 * outputs are the fields of ImageState (envs/state/state.py:4-28) plus rewards/dones.
 *
 * Conventions
 *  - plain C, no torch / HIP types in signatures; `stream` is a hipStream_t passed as void*
 *    (NULL = default stream).
 *  - every function returns 0 on success, a negative IMGENV_E* code on error; it never
 *    aborts.  imgenv_last_error() gives a thread-local message.  (The reference handlers
 *    always `return true`, img_env.cpp:726-754; Python raises on ServiceException,
 *    yaml_env.py:304-311, 367-370.)
 *  - all *input* pointers are HOST pointers and are copied during the call, except
 *    `actions` of the step functions and `records` (see below) which are DEVICE pointers.
 *  - all *output* pointers handed out by imgenv_outputs() are DEVICE pointers owned by the
 *    handle, valid until imgenv_destroy(); their contents are valid after the stream work of
 *    the last reset/step has completed and are overwritten by the next step.  They are the
 *    library's working copies, READ-ONLY for the caller: a step only rewrites what can change
 *    (a view cell no laser beam crosses holds its 200, or the footprint's 100, from the reset on;
 *    a frozen robot's rows keep their last values, agent.cpp:358-360), so whatever a caller
 *    wrote into them would stay there.  IMGENV_FLAG_CHECK_OUTPUTS detects such writes,
 *    IMGENV_FLAG_FULL_REWRITE hands out copies the caller may do anything to (below).
 *  - one handle is one world (one ImgEnv node, img_env.h:171-172) -- or imgenv_cfg.n_worlds of them,
 *    the reference's env_num nodes batched into one set of launches -- and is single-threaded
 *    like the node (ros::spin, img_env_node.cpp:8); distinct handles are independent.
 *  - fields that are float32 in the ROS messages are `float` here and are promoted to
 *    double inside exactly where the node reads them (img_env.cpp:58-81, 113-160), so the
 *    wire rounding of the reference is reproduced by construction.
 */
#ifndef IMGENV_H_
#define IMGENV_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IMGENV_ABI_VERSION 2  /* 2: imgenv_out grew (image / grid sizes, step_* arrays), spawn structs, IMGENV_FLAG_NO_VIEW_MAPS */

/* error codes */
#define IMGENV_OK 0
#define IMGENV_EINVAL (-1)    /* bad argument / unsupported configuration */
#define IMGENV_ENOMEM (-2)    /* host or device allocation failed */
#define IMGENV_EDEVICE (-3)   /* HIP runtime error (no device, launch failure, ...) */
#define IMGENV_ESTATE (-4)    /* call out of order (step before reset, ...) */

/* Agent.msg `shape` (src/comn_pkg/msg/Agent.msg:5; agent.cpp:64-77, 666-685) */
#define IMGENV_SHAPE_CIRCLE 0    /* size = [cx, cy, r]            agent.cpp:18-30  */
#define IMGENV_SHAPE_RECTANGLE 1 /* size = [xmin, xmax, ymin, ymax] agent.cpp:51-62 */
#define IMGENV_SHAPE_LEG 2       /* size = [lx, ly, lr, rx, ry, rr] agent.cpp:666-680 */

/* Env.msg `ped_scene_type` (scenefactory.h:8-24) */
#define IMGENV_SCENE_EMPTY 0
#define IMGENV_SCENE_RVO 1     /* "rvoscene"  rvoscene.h  */
#define IMGENV_SCENE_ERVO 2    /* "ervoscene" ervoscene.h */
#define IMGENV_SCENE_PEDSIM 3  /* "pedscene"  pedscene.h  */
#define IMGENV_SCENE_DATASET 4 /* "dataset": pedestrians replay recorded trajectories (img_env.cpp:295-296, 361-386) */

/* Agent.msg `ktype` of robots (agent.cpp:198, 238) */
#define IMGENV_KTYPE_DIFF 0
#define IMGENV_KTYPE_OMNI 1

/* comn_pkg/msg/SpeedLimiter.msg:1-9 (speed_limit.cpp:56-65) */
typedef struct imgenv_limiter {
    int32_t has_velocity_limits;
    int32_t has_acceleration_limits;
    int32_t has_jerk_limits;
    float min_velocity, max_velocity;
    float min_acceleration, max_acceleration;
    float min_jerk, max_jerk;
} imgenv_limiter;

/*
 * Everything InitEnv.srv carries plus the static ImageEnv / wrapper parameters that the
 * Python side of the reference keeps (yaml_env.py:133-181, base.py:153-231).
 */
typedef struct imgenv_cfg {
    int32_t abi_version;          /* must be IMGENV_ABI_VERSION */
    int32_t struct_size;          /* sizeof(imgenv_cfg), ABI guard */

    /* ---- InitEnv.srv:1-20 (img_env.cpp:58-81) ---- */
    float view_resolution;        /* metres / cell of BOTH grids after load (grid_map.cpp:28-38) */
    float view_width, view_height;/* view extent in metres (agent.cpp:79-90) */
    float step_hz;                /* YAML control_hz: the step dt in seconds (img_env.cpp:80) */
    int32_t state_dim;            /* 3 | 4 | 5 (agent.cpp:163-183) */
    int32_t use_laser;
    int32_t range_total;          /* number of beams */
    float view_angle_begin, view_angle_end;
    float view_min_dist, view_max_dist;
    float beep_r, ped_ca_p;       /* beep lottery (img_env.cpp:323-342): a robot whose action has beep (v_y) > 0 becomes, with
                                   * probability ped_ca_p, a source of radius beep_r that ERVO pedestrians move away from
                                   * (ervo_ros Agent.cpp:63-69).  The reference's Python never forwards either
                                   * (yaml_env.py:183-200 => 0 at the node, the lottery never fires); C-ABI callers may set
                                   * them.  One glibc rand() stream per world, as a fresh node process starts it.  Not
                                   * available in a robot shard (every rank would need every robot's action). */
    int32_t relation_ped_robo;    /* 1: robots are agents of the pedestrian simulator */

    /* ---- Env.msg ---- */
    float global_resolution;      /* metres / pixel of the map handed to imgenv_create; when it differs from view_resolution the
                                   * library resizes the map as GridMap::read_image does (cv::resize INTER_LINEAR to
                                   * int(px * global_resolution / view_resolution), grid_map.cpp:28-38) */
    int32_t ped_scene_type;       /* IMGENV_SCENE_* */
    int32_t n_robots;             /* robots of the WORLD (all shards) */
    int32_t n_peds;
    int32_t robot_ktype;          /* IMGENV_KTYPE_* */
    const int32_t* robot_shape;   /* [n_robots] IMGENV_SHAPE_* */
    const float* robot_size;      /* [n_robots][4]  Agent.msg size[] */
    const float* robot_sensor_cfg;/* [n_robots][2]  Agent.msg sensor_cfg[] */
    imgenv_limiter limiter_v, limiter_w;
    const int32_t* ped_shape;     /* [n_peds] */
    const float* ped_size;        /* [n_peds][6] */
    const float* ped_max_speed;   /* [n_peds] */

    /* ---- Python-side ImageEnv parameters (yaml_env.py:133-181) ---- */
    int32_t image_size[2];        /* sensor_map size (width, height) cv2.resize INTER_CUBIC shrinks the view to (yaml_env.py:433) */
    int32_t ped_image_size[2];
    int32_t max_ped;              /* ped vector has 1 + ped_vec_dim*max_ped entries; n_peds <= max_ped */
    int32_t ped_vec_dim;          /* 7 */
    double ped_image_r;
    double laser_max;
    int32_t laser_norm;
    const double* robot_size_last;/* [n_robots] YAML robot.size[i][-1] as the Python float (yaml_env.py:407) */

    /* ---- wrapper parameters (base.py:153-231) ---- */
    double ped_safety_space;
    int32_t time_max;

    /* ---- robot shard owned by this handle (multi-GPU, one process per GPU) ---- */
    int32_t robot_begin, robot_end; /* [begin, end) within the world's robots; 0,n_robots = unsharded */

    /* ---- implementation knobs ---- */
    int32_t device;               /* HIP device ordinal */
    int32_t flags;                /* IMGENV_FLAG_* */
    /* Optional caller-owned DEVICE arena for every output buffer and the records buffer, so a
     * host framework can alias them zero-copy (e.g. slices of one torch uint8 tensor).  Size it
     * with imgenv_arena_bytes(); NULL = the library allocates (and frees) its own. */
    void* out_arena;
    int64_t out_arena_bytes;

    /* ---- independent worlds in one handle: the reference's env_num processes, batched ---- */
    /* n_worlds copies of the same parameters, every one on the map of imgenv_create (or, with imgenv_maps_add, on the map of a
     * bank chosen per world and episode); n_robots and n_peds are TOTALS (multiples of n_worlds), numbered
     * world-major: world k owns robots [k n_robots / n_worlds, (k + 1) n_robots / n_worlds) and the same share of the
     * pedestrians.  Robots and pedestrians only ever see their own world.  0 or 1 = a single world.  Each world is reset
     * on its own with imgenv_reset_world(); its time limit counts from its own reset. */
    int32_t n_worlds;
    int32_t reserved_;
} imgenv_cfg;

#define IMGENV_FLAG_PRIVATE_GRIDS 1 /* oracle only: literal per-robot grid copies (img_env.cpp:620-629) */
/* How the class layer (what a robot's view looks up per map cell) is kept up to date.  Default: the library picks --
 * DENSE: the rasters fill owner layers and every step merges them over every map cell of every world, best when the robots
 * and pedestrians cover a good part of the map; SPARSE: the rasters stamp the class layer directly and stamps expire with
 * their step, nothing per cell, best for big or many maps with few agents each.  The result is the same either way. */
#define IMGENV_FLAG_COMPOSE_DENSE 2
#define IMGENV_FLAG_COMPOSE_SPARSE 4
/* (round 5) Where DENSE used to be the library's pick it now keeps COUNTS on the class layer instead: every robot and pedestrian adds
 * itself to the cells it covers and takes itself off the ones it leaves (fire-and-forget atomics, none at all while it covers
 * the same cells), so no pass over every cell merges anything per step.  IMGENV_FLAG_COMPOSE_DENSE still asks for the owner
 * layers + the per-step merge; IMGENV_FLAG_LAYER_SUM asks for the counting layer wherever it can run (the handle owns every
 * robot, views through k_view), also where the library would have stamped.  Same results in every mode. */
#define IMGENV_FLAG_LAYER_SUM 512
/* imgenv_out.view_maps is not wanted.  It only matters where the view is shrunk into the sensor_map (image_size differs from
 * the view size, every shipped config of the reference: a 400 x 400 view, 160 KB per robot, behind a 48 x 48 sensor_map):
 * the library then evaluates only the 4 x 4 view cells each sensor_map pixel reads and never writes the full-size view;
 * view_maps keeps whatever it held.  ImageState (envs/state/state.py:4-28) has no such field, so img_env_amd's envs set it. */
#define IMGENV_FLAG_NO_VIEW_MAPS 8
/* also produce AgentState.hits_x / hits_y / angular_map (imgenv_out, below) */
#define IMGENV_FLAG_AGENT_STATE_EXTRAS 16
/* Which kernels compute the views.  Default: one wavefront per robot (k_view) wherever it can run; the tiled kernels that
 * spread one robot's view over the chip (csrc/view_big.h) for views k_view cannot pack (beyond 255 x 255 cells or 255 ray
 * steps) and for shrunk sensor_maps.  IMGENV_FLAG_VIEW_TILED asks for the tiled kernels where both can run; the result is the
 * same. */
#define IMGENV_FLAG_VIEW_TILED 32
#define IMGENV_FLAG_VIEW_WAVE 64  /* (reserved: k_view is the default) */
/* Guards for the read-only output arrays (see "Conventions": imgenv_outputs() hands out the kernels' incremental working copies,
 * where the reference returns fresh copies with every service response, img_env.cpp:745-749).
 * IMGENV_FLAG_CHECK_OUTPUTS (debug): every output array is sealed with a checksum when a reset / step has been queued and
 * verified at the start of the next reset / step call; a mismatch fails that call with IMGENV_EINVAL "the caller wrote into
 * imgenv_out.<field>".  The verification synchronises the stream once per call.
 * IMGENV_FLAG_FULL_REWRITE: for callers that cannot promise to leave the arrays alone (in-place normalisation, ...).
 * imgenv_outputs() then hands out a SECOND arena (imgenv_cfg.out_arena if given) whose every byte is rewritten from the
 * kernels' private working copy at the end of every reset / step; whatever the caller does to it never reaches the kernels.
 * Costs one device-to-device copy of imgenv_arena_bytes() per call. */
#define IMGENV_FLAG_CHECK_OUTPUTS 128
#define IMGENV_FLAG_FULL_REWRITE 256
/* IMGENV_FLAG_CHECK_OUTPUTS for the first IMGENV_CHECK_FIRST_CALLS reset / step calls of the handle only; the guard then switches
 * itself off and costs nothing.  A trainer that normalises observations in place does so from its first step: it is told at once,
 * loudly, instead of training on silently corrupted views -- and a correct one pays a synchronisation per call for a fraction of
 * a second.  The Python mirror (img_env_amd.World, ImageEnv, VecImageEnv) creates every handle with it unless told otherwise
 * (params["output_guard"] = "none" | "first" | "check" | "copy"). */
#define IMGENV_FLAG_CHECK_OUTPUTS_FIRST 1024
#define IMGENV_CHECK_FIRST_CALLS 64

/* ResetEnv.srv:1-6 (img_env.cpp:162-292).  Poses are (x, y, qz, qw): geometry_msgs/Pose with a
 * planar orientation; yaw is recovered with tf::Matrix3x3(q).getRPY as the node does. */
typedef struct imgenv_reset_batch {
    int32_t struct_size;
    int32_t n_obstacles;
    const int32_t* obs_shape;     /* [n_obstacles] */
    const float* obs_size;        /* [n_obstacles][4] */
    const double* obs_pose;       /* [n_obstacles][4] */
    const double* robot_pose;     /* [n_robots][4]  (whole world) */
    const double* robot_goal;     /* [n_robots][2] */
    const double* ped_pose;       /* [n_peds][4] */
    const double* ped_goal;       /* [n_peds][2] */
    const int32_t* ped_traj_len;  /* [n_peds] */
    const double* ped_traj;       /* [n_peds][ped_traj_cap][3]  Agent.msg trajectory (x, y, z) */
    int32_t ped_traj_cap;
    int32_t ignore_obstacle;
    const double* ped_traj_v;     /* [n_peds][ped_traj_cap][2]  Agent.msg trajectory_v (vx, vy): IMGENV_SCENE_DATASET only, else NULL */
} imgenv_reset_batch;

/* Device pointers of the per-robot outputs, R = robot_end - robot_begin local robots.
 * Field meaning follows ImageState (envs/state/state.py:4-28) and _get_states
 * (yaml_env.py:446-481). */
typedef struct imgenv_out {
    int32_t struct_size;
    int32_t n_local;              /* R */
    int32_t view_h, view_w;       /* Hv, Wv */
    int32_t n_beams;              /* B (0 when !use_laser) */
    int32_t state_dim;
    int32_t ped_vec_len;          /* 1 + ped_vec_dim*max_ped */
    int32_t image_h, image_w;     /* sensor_maps size: imgenv_cfg.image_size (= the view size unless cv2.resize shrinks it) */
    int32_t grid_h, grid_w;       /* the occupancy grid after the load-time resize (grid_map.cpp:28-38) */
    float* vector_states;         /* [R][state_dim]      AgentState.state (float32 wire) */
    uint8_t* view_maps;           /* [R][Hv][Wv]         AgentState.view_map (8UC1) */
    uint16_t* sensor_maps;        /* [R][image_h][image_w] float16 bits = cv2.resize(view, image_size, INTER_CUBIC) / 255
                                   * (yaml_env.py:431-438; OpenCV copies when the sizes are equal) */
    float* lasers_raw;            /* [R][B]              AgentState.laser */
    double* lasers;               /* [R][B]              _norm_lasers (yaml_env.py:440-444) */
    float* ped_vector_states;     /* [R][ped_vec_len] */
    float* ped_maps;              /* [R][3][Hp][Wp] */
    int8_t* is_collisions;        /* [R]  AgentState.is_collision 0..3 */
    uint8_t* is_arrives;          /* [R] */
    double* step_ds;              /* [R] */
    double* ped_min_dists;        /* [R] (+inf until a ped has been seen) */
    /* ImageEnv.step base outputs (yaml_env.py:372-377) */
    int32_t* base_rewards;        /* [R] arrive - collision code */
    uint8_t* base_dones;          /* [R] */
    /* wrapper stack outputs (base.py:153-254, 69-93) */
    double* rewards;              /* [R] SensorsPaperRewardWrapper, zeroed where !is_clean (the full default stack) */
    double* paper_rewards;        /* [R] SensorsPaperRewardWrapper before the MultiRobotClean mask */
    uint8_t* dones;               /* [R] after TimeLimitWrapper */
    int32_t* dones_info;          /* [R] 0 | 1..3 collision class | 5 arrive | 10 time-out */
    uint8_t* is_clean;            /* [R] MultiRobotCleanWrapper mask used for this step */
    /* simulator state mirrors, handy for tests and GUIs */
    double* robot_pose;           /* [R][3] x, y, theta */
    double* ped_state;            /* [n_peds][4] x, y, vx, vy (world copy) */
    int32_t* counters;            /* [4]: steps since reset (n_worlds > 1: of world 0), #done robots of the last step (local),
                                   * #frozen views since the last imgenv_reset (local), #frozen views since create */
    /* The last STEP's own per-robot scalars: every imgenv_step writes them beside the arrays above, a reset never touches
     * them.  After imgenv_step_autoreset() the rows of the worlds it reset hold, above, the new episode's first observation
     * (NeverStopWrapper, base.py:198-211) and, here, what that step itself returned for them. */
    double* step_rewards;         /* [R] */
    uint8_t* step_dones;          /* [R] */
    int32_t* step_dones_info;     /* [R] */
    uint8_t* step_is_clean;       /* [R] */
    uint8_t* step_is_arrives;     /* [R] */
    int8_t* step_is_collisions;   /* [R] */
    uint8_t* step_all_down;       /* [R] 1 where all robots of the robot's world were done after that step (written by
                                   * imgenv_step_autoreset only) */
    /* The remaining fields of AgentState.msg (src/comn_pkg/msg/AgentState.msg:4-6; filled at agent.cpp:405-438, sent at
     * img_env.cpp:558-560), which ImageEnv never reads: NULL unless the handle was created with IMGENV_FLAG_AGENT_STATE_EXTRAS. */
    float* hits_x;                /* [R][B] hit * cos(beam angle): the hit points in the sensor frame */
    float* hits_y;                /* [R][B] hit * sin(beam angle) */
    float* angular_map;           /* [R][72] nearest hit per 1/72 of the field of view, view_max_dist where nothing was hit */
} imgenv_out;
#define IMGENV_ANGULAR_BINS 72    /* agent.cpp:407 */

typedef struct imgenv imgenv_t;

/* library / build identification: "hip-gfx950" for the product library */
const char* imgenv_backend(void);
/* which build: a hash of the extension's sources and compiler flags (__graft_entry__.source_id), "unstamped" for a library
 * compiled by hand.  profiles/pmc_latest.json carries the id of the library its counters were collected on. */
const char* imgenv_build_id(void);
int32_t imgenv_abi_version(void);
const char* imgenv_last_error(void);

/* init_image_env: builds all per-class static tables (footprints, FOV mask, ray tables) and
 * uploads the static occupancy grid (uint8, row-major [Hg][Wg], rows <-> world x;
 * grid_map.cpp:40-55).  Hg x Wg is the size of `static_map` as given: the map image in its own pixels when
 * global_resolution != view_resolution (the grid the handle works on is then the resized one, imgenv_out.grid_h / grid_w). */
int imgenv_create(const imgenv_cfg* cfg, const uint8_t* static_map, int32_t Hg, int32_t Wg,
                  imgenv_t** out);
/* bytes of output arena a handle created from `cfg` needs (256-byte aligned carve-outs) */
int64_t imgenv_arena_bytes(const imgenv_cfg* cfg);
void imgenv_destroy(imgenv_t* h);

/* reset_image_env: obstacles raster + ORCA obstacle tree + poses, then view + states. */
int imgenv_reset(imgenv_t* h, const imgenv_reset_batch* batch, void* stream);

/* step_image_env + Python post-processing.  actions: DEVICE float[R][3] = (v, w, beep) of the
 * local robots (ContinuousAction, envs/action/action.py:8-20).  Dead robots are zeroed
 * inside (yaml_env.py:319-331).  The call is stream-ordered: actions written by work queued on `stream` in front of it are
 * seen, and outputs of the previous call are not rewritten before work queued on `stream` in front of it has read them. */
int imgenv_step(imgenv_t* h, const float* actions, void* stream);
/* The same with per-call flags.  IMGENV_STEP_ACTIONS_READY: "the actions hold their final values when the call is made".
 * Accepted, and WITHOUT EFFECT since round 6: rounds 4-5 let such a step start its observation kernel on a side stream behind the
 * previous step's views alone, which was not ordered behind the caller's readers of the previous outputs (a replay-buffer copy
 * queued on `stream`, IMGENV_FLAG_FULL_REWRITE's own copy).  Every step now starts that kernel behind a one-wavefront gate that
 * opens when `stream` reaches the step's first kernel -- ordered behind everything queued in front of the call, at the same rate
 * (92.3 against 92.0 us per headline step). */
#define IMGENV_STEP_ACTIONS_READY 1u
int imgenv_step_flags(imgenv_t* h, const float* actions, uint32_t flags, void* stream);

/* The same step split around the one exchange a robot-sharded world needs:
 *   step_begin : pedestrian advance + pose integrate of the local robots, publishes their
 *                records into records[robot_begin:robot_end]
 *   (caller all-gathers `records` in place across ranks, e.g. RCCL ncclAllGather)
 *   step_end   : rasters + per-robot view/observation/reward kernels
 * imgenv_step == step_begin; step_end when the handle owns the whole world. */
/* `actions` must stay as they are until imgenv_step_end has been called: kernels of the step read them on the library's side
 * streams, which are joined into `stream` again at the end of imgenv_step_end (work queued on `stream` BEHIND step_end may
 * overwrite them; work queued between the two calls may not). */
int imgenv_step_begin(imgenv_t* h, const float* actions, void* stream);
int imgenv_step_end(imgenv_t* h, void* stream);
/* records: DEVICE double[n_robots][IMGENV_RECORD_DOUBLES] = x, y, theta, vx, vy, sin(theta/2), cos(theta/2), pad
 * (64 bytes per robot; the half-angle sine / cosine are cached so that the raster / view / observation kernels of
 * every rank build the robot's tf::Transform without re-evaluating them) */
#define IMGENV_RECORD_DOUBLES 8
int imgenv_records(imgenv_t* h, double** records, int64_t* bytes_per_robot);
/* reset counterpart of the exchange (robots' initial records are known to every rank from the
 * batch, so reset needs no collective). */

/* Optional: let the library run the exchange itself.  After imgenv_comm_init() on every rank,
 * imgenv_step() = step_begin; ncclAllGather (RCCL, in place, on the caller's stream); step_end -- no host
 * synchronisation and no framework collective per step.  Needs equal contiguous shards
 * (robot_begin == rank * n_local).  The 128-byte id comes from imgenv_comm_unique_id() on rank 0 and must be
 * broadcast to the other ranks by the caller (any side channel, e.g. torch.distributed).  RCCL is loaded at
 * run time (dlopen); IMGENV_EDEVICE if it is unavailable. */
#define IMGENV_COMM_ID_BYTES 128
int imgenv_comm_unique_id(void* id128);
int imgenv_comm_init(imgenv_t* h, const void* id128, int32_t rank, int32_t n_ranks);
/* what RCCL itself reports for the handle's communicator (ncclCommCount / ncclCommUserRank); IMGENV_ESTATE without one */
int imgenv_comm_info(imgenv_t* h, int32_t* n_ranks, int32_t* rank);

/* out->struct_size on entry: 0 (the caller's imgenv_out is this header's) or the size of the caller's older, shorter struct --
 * then only that many bytes are written (fields are only ever appended at the end). */
int imgenv_outputs(imgenv_t* h, imgenv_out* out);

/* Multi-world handles (imgenv_cfg.n_worlds > 1): reset ONE world while the others keep their state -- what one env
 * process of the reference does when its episode ends (ImageEnv.reset, yaml_env.py:296-317).  The batch holds that
 * world's robots (n_robots / n_worlds), pedestrians and obstacles only.  imgenv_reset() on such a handle resets every
 * world from a batch of all robots / pedestrians (world-major) with one obstacle list shared by all worlds. */
int imgenv_reset_world(imgenv_t* h, int32_t world, const imgenv_reset_batch* batch, void* stream);
/* The same for n distinct worlds at once (batches[q] belongs to worlds[q]): one upload launch and one set of reset / view
 * launches however many worlds ended their episode on this step -- NeverStopWrapper (base.py:198-211) for a whole batch
 * of envs. */
int imgenv_reset_worlds(imgenv_t* h, int32_t n, const int32_t* worlds, const imgenv_reset_batch* batches, void* stream);

/* ---- spawn: the random placement EnvPos.reset does for one episode (envs/utils/reset_helper.py:104-345), natively ----
 * A world of a multi-world handle is reset whenever its episode ends -- dozens of worlds on every step -- so the placement
 * itself has to be cheap.  Rules as in the reference (starts > clearance apart and clear of the obstacles; targets
 * > target_min_dist from their start, > clearance apart, clear of the obstacles; range_view targets in the 4 m box around
 * the start but outside its 2.5 m box; pedestrians walk to their target and, with go_back, back); the random stream is
 * the library's own (seeded per world), not Python's.  Pose types of reset_helper.py:187-300: */
#define IMGENV_POSE_FIX 0         /* [x, y, yaw] */
#define IMGENV_POSE_RAND_ANGLE 1  /* [x, y, yaw_lo, yaw_hi] */
#define IMGENV_POSE_RANGE 2       /* [x_lo, x_hi, y_lo, y_hi], yaw uniform in +-3.14 */
#define IMGENV_POSE_RANGE_YAW 3   /* [x_lo, x_hi, y_lo, y_hi, yaw_lo, yaw_hi] */
#define IMGENV_POSE_RANGE_VIEW 4  /* targets only: [x_lo, x_hi, y_lo, y_hi], drawn around the start (random_view, 62-82) */
#define IMGENV_POSE_RANGE_CIRCLE 5      /* [cx, cy]: on the episode's circle around (cx, cy) at a random angle + noise, facing the
                                         * centre (starts, 223-230); opposite the start (targets, 263-268) */
#define IMGENV_POSE_RANGE_CIRCLE_FIX 6  /* the same at the agent's own share of the circle: angle -3.14 + 6.28 i / n (226-227) */
#define IMGENV_POSE_CIRCLE_FIX 7        /* targets only: exactly opposite the start, no noise, no checks (258-262) */
#define IMGENV_POSE_RANGE_MULTI 8       /* one of several boxes, picked per draw (231-232, 269-270): *_multi / n_*_multi */

typedef struct imgenv_spawn_agent {   /* a robot or a pedestrian */
    int32_t begin_type, target_type;  /* IMGENV_POSE_* */
    double begin[6], target[6];
    double module_size;               /* 2 x the footprint's radius (reset_helper.py:167-186): what must clear the obstacles */
    const double* begin_multi;        /* IMGENV_POSE_RANGE_MULTI: [n_begin_multi][6] boxes x_lo, x_hi, y_lo, y_hi, yaw_lo, yaw_hi */
    const double* target_multi;       /* (a 4-number box of the YAML carries yaw -3.14 .. 3.14) */
    int32_t n_begin_multi, n_target_multi;
} imgenv_spawn_agent;

typedef struct imgenv_spawn_obstacle {
    int32_t shape;                    /* IMGENV_SHAPE_CIRCLE (radius uniform in size_range[0..1]) | _RECTANGLE (size_range = size) */
    int32_t pose_type;                /* IMGENV_POSE_FIX | _RANGE | _RANGE_YAW */
    double size_range[4];
    double pose[6];
} imgenv_spawn_obstacle;

typedef struct imgenv_spawn_cfg {     /* ONE world's cast */
    int32_t struct_size;
    int32_t n_robots, n_peds, n_obstacles;
    const imgenv_spawn_agent* agents;        /* [n_robots + n_peds], robots first */
    const imgenv_spawn_obstacle* obstacles;  /* [n_obstacles] */
    double clearance;                 /* free_check_robo_ped distance (1.0) */
    double target_min_dist;
    double circle_ranges[2];          /* the episode's circle radius is uniform in here (YAML circle_ranges) */
    int32_t go_back;                  /* pedestrians return to their start: 0 no, 1 yes, 2 a coin per pedestrian */
    int32_t ignore_obstacle;
} imgenv_spawn_cfg;

/* One placement into caller-owned host arrays (any of them may be NULL): robot_pose [R][4] (x, y, qz, qw), robot_goal [R][2],
 * ped_pose [P][4], ped_goal [P][2], ped_traj [P][2][3], ped_traj_len [P], obs_shape [O], obs_size [O][4], obs_pose [O][4].
 * Needs no device. */
int imgenv_spawn(const imgenv_spawn_cfg* cfg, uint64_t seed, double* robot_pose, double* robot_goal, double* ped_pose,
                 double* ped_goal, double* ped_traj, int32_t* ped_traj_len, int32_t* obs_shape, float* obs_size, double* obs_pose);
/* imgenv_reset_worlds() with a fresh placement for each listed world, world worlds[q] from seeds[q]. */
int imgenv_reset_worlds_spawn(imgenv_t* h, int32_t n, const int32_t* worlds, const imgenv_spawn_cfg* cfg, const uint64_t* seeds,
                              void* stream);
/* One env step of a handle of n_worlds reference envs the way the trainer runs them (NeverStopWrapper over the default
 * wrapper stack, base.py:198-211, one env process per world): imgenv_step(), then every world whose robots are ALL done
 * (imgenv_out.dones) starts a new episode from a fresh placement, as imgenv_reset_worlds_spawn() would, the k-th such world
 * (ascending world index) from seed seed0 + k.  The list of finished worlds is made on the device and read by the host
 * from page-locked memory, so the call returns with the step complete on `stream` (one host synchronisation, no copy).
 * worlds_out (may be NULL) receives up to cap world indices, *n_out their number. */
int imgenv_step_autoreset(imgenv_t* h, const float* actions, const imgenv_spawn_cfg* cfg, uint64_t seed0, int32_t* worlds_out,
                          int32_t cap, int32_t* n_out, void* stream);

/* imgenv_step_autoreset() without the host in the loop (csrc/spawn_device.h): the finished worlds are found, placed and reset by
 * kernels alone -- placements are drawn ahead into a pool on a side stream with the same rules and random stream as
 * imgenv_spawn() but the device's libm (a placement may differ from the host's in the last bit) -- and the call returns as
 * soon as everything is queued on `stream`: no synchronisation, nothing read back.  The FIRST call with a given spawn cfg
 * fixes seed0: the k-th world reset from then on (in step order, ascending world index within a step) takes placement
 * seed0 + k, as a loop of imgenv_step_autoreset() calls fed seed0 + (worlds reset so far) would hand them out.  RVO, ERVO and
 * empty scenes, and social-force crowds (pedscene) in handles of several worlds; at most 256 agents and 24 obstacles per world. */
int imgenv_step_autoreset_device(imgenv_t* h, const float* actions, const imgenv_spawn_cfg* cfg, uint64_t seed0, void* stream);
/* What the last such call did, for checkers and hosts that do want to know (synchronises `stream`): the worlds it reset
 * (ascending, up to cap), their number, and the placement number of the first of them. */
int imgenv_autoreset_last(imgenv_t* h, int32_t* worlds_out, int32_t cap, int32_t* n_out, uint64_t* first_placement, void* stream);
/* The placement world `world` currently runs as its device-side reset received it -- the arrays of imgenv_spawn(), any may be
 * NULL -- and its number.  Synchronises the device. */
int imgenv_world_placement(imgenv_t* h, int32_t world, uint64_t* placement, double* robot_pose, double* robot_goal, double* ped_pose,
                           double* ped_goal, double* ped_traj, int32_t* ped_traj_len, int32_t* obs_shape, float* obs_size, double* obs_pose);

/* ---- observation stacks: StateBatchWrapper (envs/wrapper/base.py:97-150) for every robot of the handle, on the device ----
 * The reference's policy never sees one frame: it sees the last image_batch sensor maps, the last state_batch vector states and
 * the last max(laser_batch, 1) laser scans of the current episode, zero-padded at the episode's start.  With stacks enabled the
 * library keeps, for every local robot and every stacked field of depth K, after any call has completed on the stream:
 *   the call reset the robot's world (imgenv_reset, imgenv_reset_world(s), imgenv_reset_worlds_spawn, the worlds an
 *   imgenv_step_autoreset / imgenv_step_autoreset_device call restarted):   stack = [0, ..., 0, F]
 *   otherwise (a step):                                                     stack = [old[1], ..., old[K-1], F]
 * F = the field's row of imgenv_out after that call, 0 = all-zero bytes; oldest first, newest last, contiguous per robot (the
 * reference's [n, k, ...] layout, vector states flattened to [n, k * state_dim], base.py:116-136).  A frozen robot's row keeps
 * repeating its last frame, as the reference pushes it.  One extra kernel launch per chain (csrc/stack.h), none when every depth is
 * 0 or 1, no host synchronisation, allocation or copy per step.
 * Depths are the YAML keys: image_batch > 0 stacks the sensor maps, 0 leaves them alone; state_batch likewise; laser_batch >= 0
 * stacks max(laser_batch, 1) scans, < 0 leaves them alone (base.py:103-105).  No depth may exceed IMGENV_STACK_MAX_DEPTH. */
#define IMGENV_STACK_MAX_DEPTH 16
typedef struct imgenv_stack_cfg {
    int32_t struct_size;          /* sizeof(imgenv_stack_cfg) */
    int32_t image_batch, state_batch, laser_batch;
    /* Optional caller-owned DEVICE memory for the stacks (a host framework can alias it zero-copy); size it with
     * imgenv_stack_bytes(), 256-byte aligned.  NULL = the library allocates (and frees) its own. */
    void* arena;
    int64_t arena_bytes;
} imgenv_stack_cfg;
/* Device pointers of the stacks, R = robot_end - robot_begin local robots (a robot shard stacks its local rows; nothing crosses
 * ranks).  Ownership as for imgenv_out: valid until imgenv_destroy(), contents valid once the stream work of the last reset / step
 * has completed; they are the library's working copies, READ-ONLY for the caller -- the next step's shift reads them back, so
 * whatever a caller wrote would travel through the stack.  The IMGENV_FLAG_CHECK_OUTPUTS* guards do NOT cover them.  A field of
 * depth 1 costs nothing: its pointer IS the array imgenv_outputs() hands out ([R][1][...] is the same bytes; with
 * IMGENV_FLAG_FULL_REWRITE that is the public copy) and it takes no arena space.  Deeper stacks are always fed from the kernels'
 * private working arrays, also under IMGENV_FLAG_FULL_REWRITE. */
typedef struct imgenv_stack_out {
    int32_t struct_size;          /* on entry 0 or sizeof(imgenv_stack_out) */
    int32_t n_local;              /* R */
    int32_t image_depth, state_depth, laser_depth; /* effective depths; 0 = the field is not stacked and its pointer is NULL */
    int32_t reserved_;
    uint16_t* sensor_maps;        /* [R][image_depth][image_h][image_w]  float16 bits */
    float* vector_states;         /* [R][state_depth * state_dim] */
    double* lasers;               /* [R][laser_depth][B]; NULL on a handle without lasers whatever laser_batch says */
} imgenv_stack_out;
/* bytes of stack memory a handle created from `cfg` needs for `s`: the sum over the fields of depth >= 2 of
 * R * depth * frame bytes, each rounded up to 256 (0 when nothing is deeper than 1).  Negative IMGENV_E* code for a bad
 * configuration or a depth above the cap.  Needs no device, like imgenv_arena_bytes(). */
int64_t imgenv_stack_bytes(const imgenv_cfg* cfg, const imgenv_stack_cfg* s);
/* Legal once per handle, after imgenv_create() and before its first reset (IMGENV_ESTATE otherwise); IMGENV_EINVAL for a depth
 * above the cap or an arena that is too short or misaligned.  `out` (may be NULL) receives the pointers; imgenv_stack_outputs()
 * hands them out again later.  A handle that never calls it behaves, launch for launch, as if this section did not exist. */
int imgenv_stack_enable(imgenv_t* h, const imgenv_stack_cfg* s, imgenv_stack_out* out);
int imgenv_stack_outputs(imgenv_t* h, imgenv_stack_out* out);

/* ---- episode statistics: TestEpisodeWrapper (envs/wrapper/evaluation_wrapper/TestEpisodeWrapper.py:8-119) and its
 * TrajectoryPathHelper (evaluation_wrapper/utils.py:5-133) for every robot of the handle, on the device ----
 * The reference evaluates a policy by wrapping ONE env in TestEpisodeWrapper: how its episodes end (arrive / collision classes /
 * time-out, by dones_info), steps to arrive, mean v and |w|, and per episode the variance and sign changes of w and the mean
 * |acceleration| and |jerk| of the commands.  With episode statistics enabled the library keeps the same for every local robot,
 * plus the episode's return and length, with no host in the loop -- also behind imgenv_step_autoreset_device, where the host never
 * learns that an episode ended.  One extra kernel launch per chain (csrc/episodes.h), no host synchronisation, allocation or copy
 * per step; everything in float64 / int32, one fixed operation order per robot (results are deterministic).
 *
 * After a step (any imgenv_step* call), per local robot with an open episode (TestEpisodeWrapper.py:37-45, utils.py:26-28, 60-100):
 *   the command is (v, w) of the robot's `actions` row, promoted to double, (0, 0) where imgenv_out.step_is_clean is 0
 *   (MultiRobotCleanWrapper masks info["speeds"], base.py:58, 83); steps += 1; v_sum += v; w_sum += |w|; the open episode's path
 *   sums take the command (n, sum v, sum w, sum w^2, sum |w|, sum |acc| and |jerk| of v and w from the last two commands with
 *   acc = (x - prev) / dt, sign changes of w counted against the previous command, 0 before the first);
 *   ep_return += imgenv_out.step_rewards; ep_len += imgenv_out.step_is_clean (the reference keeps neither).
 * At a reset of the robot's world (imgenv_reset, imgenv_reset_world(s), imgenv_reset_worlds_spawn, the worlds an
 * imgenv_step_autoreset / imgenv_step_autoreset_device call restarted), reading the LAST step's imgenv_out.step_dones_info
 * (TestEpisodeWrapper.py:47-85):
 *   steps > min_steps: the episode is COUNTED -- ends[bin] += 1 (bins below; a reset of an unfinished robot, code 0, is
 *   `aborted`: the reference's wrapper exits there), episodes += 1, speed_steps += steps, arrive_steps += steps where the code is
 *   5, the episode's figures w_variance = sum w^2 / n - (sum w / n)^2, w_zero, v_acc = sum |acc v| / max(n - 1, 1), w_acc, v_jerk =
 *   sum |jerk v| / max(n - 2, 1), w_jerk, v_avg = sum v / n, w_avg = sum |w| / n -- each but w_zero rounded to 4 places,
 *   rint(x * 1e4) / 1e4 -- are added to the robot's totals, return_sum += ep_return, len_sum += ep_len, last_* record the
 *   episode, and the path sums restart.
 *   otherwise the episode is too short to count (the reference's `tmp_steps > 3`): short_episodes += 1 and its path sums are NOT
 *   restarted -- its commands ride into the next counted episode, as in the reference, whose helper is only emptied by a
 *   counted reset.
 *   Either way steps, ep_return and ep_len restart, and an episode is open from now on.
 * Enabling marks every robot "no episode open": steps are ignored until the first reset after enabling, which folds nothing. */
typedef struct imgenv_episodes_cfg {
    int32_t struct_size;          /* sizeof(imgenv_episodes_cfg) */
    int32_t min_steps;            /* an episode counts when it took MORE steps than this; the reference's is 3 (TestEpisodeWrapper.py:48) */
    double dt;                    /* the YAML's control_hz: the divisor of the acceleration / jerk terms (utils.py:86-100) */
} imgenv_episodes_cfg;
#define IMGENV_EP_ARRIVE 0        /* rows of imgenv_episodes_out.ends: dones_info 5 */
#define IMGENV_EP_TIMEOUT 1       /* 10 */
#define IMGENV_EP_COLLISION 2     /* 1 static, then 2 pedestrian, 3 other robot */
#define IMGENV_EP_ABORTED 5       /* any other code: the caller reset an unfinished robot */
#define IMGENV_EP_END_BINS 6
#define IMGENV_EP_FIGURES 8       /* rows of figure_sums: w_variance, w_zero, v_acc, w_acc, v_jerk, w_jerk, v_avg, w_avg */
#define IMGENV_EP_OPEN_F64 15     /* rows of open_f64: n, sum v, sum w, sum w^2, sum |w|, sum |acc v|, sum |acc w|, sum |jerk v|,
                                   * sum |jerk w|, prev v, prev w, last-but-one v, last-but-one w, w_zero, ep_return */
/* Device pointers of the per-robot statistics, R = robot_end - robot_begin local robots (a robot shard keeps its local rows).
 * Two-dimensional arrays are [row][R]: one row per quantity, robots contiguous.  Ownership as for imgenv_out: owned by the handle,
 * valid until imgenv_destroy(), contents valid once the stream work of the last reset / step has completed, READ-ONLY for the
 * caller (they are the running sums themselves). */
typedef struct imgenv_episodes_out {
    int32_t struct_size;          /* on entry 0 or sizeof(imgenv_episodes_out) */
    int32_t n_local;              /* R */
    /* totals over the robot's counted episodes (TestEpisodeWrapper.py:15-35) */
    int32_t* ends;                /* [IMGENV_EP_END_BINS][R]  arrive_num, stuck_num, static / ped / other_coll_num, aborted */
    int32_t* episodes;            /* [R] counted episodes (cur_episode) */
    int32_t* short_episodes;      /* [R] episodes too short to count */
    int32_t* speed_steps;         /* [R] speed_step: steps of the counted episodes */
    int32_t* arrive_steps;        /* [R] steps: steps of the episodes that arrived */
    int32_t* len_sum;             /* [R] clean steps of the counted episodes */
    double* v_sum;                /* [R] sum of v over every step (not only those of counted episodes, as in the reference) */
    double* w_sum;                /* [R] sum of |w| */
    double* figure_sums;          /* [IMGENV_EP_FIGURES][R]  the rounded figures summed over the counted episodes */
    double* return_sum;           /* [R] returns of the counted episodes */
    /* the robot's last counted episode: a trainer polls last_episode for completions */
    int32_t* last_code;           /* [R] dones_info it ended with */
    int32_t* last_steps;          /* [R] */
    int32_t* last_len;            /* [R] */
    int32_t* last_episode;        /* [R] its number, 1-based (= episodes when it was counted); 0: none yet */
    double* last_return;          /* [R] */
    /* the open episode */
    double* open_f64;             /* [IMGENV_EP_OPEN_F64][R] */
    int32_t* open_steps;          /* [R] steps since the robot's last reset (tmp_steps) */
    int32_t* open_len;            /* [R] of which clean */
    int32_t* open;                /* [R] 1 once a reset after enabling has opened an episode */
} imgenv_episodes_out;
/* Legal at any time; the memory is the library's.  IMGENV_EINVAL for a wrong struct_size, dt <= 0 (or not finite), min_steps < 0,
 * or a second call whose cfg differs from the first's; a second call with the same cfg changes nothing and hands out the same
 * pointers.  `out` may be NULL.  A handle that never calls it behaves, launch for launch, as if this section did not exist. */
int imgenv_episodes_enable(imgenv_t* h, const imgenv_episodes_cfg* cfg, imgenv_episodes_out* out);
/* IMGENV_ESTATE before imgenv_episodes_enable() */
int imgenv_episodes_outputs(imgenv_t* h, imgenv_episodes_out* out);
/* TestEpisodeWrapper.__init__'s zeros (TestEpisodeWrapper.py:15-35) again, ordered on `stream`: every total, last_* and the open
 * episode's sums and counters become 0 (one memset); `open` keeps its value, so what follows of an episode in flight still counts
 * if it is long enough. */
int imgenv_episodes_clear(imgenv_t* h, void* stream);

/* ---- episode log: one record per finished episode, with what it ran on ----
 * The reference writes one line per episode of a fixed test set (PedTrajectoryDatasetWrapper.out2logfile, BarnDataSetWrapper.
 * out2logfile: which world, how it ended, v_avg ... w_zero, path_time, steps), and TestEpisodeWrapper keeps per-episode lists
 * (w_variance_array, ...).  The statistics above are running totals per robot; the log is their per-episode half: a ring of records
 * in device memory.  Every reset chain (imgenv_reset, imgenv_reset_world(s), imgenv_reset_worlds_spawn / _scenarios, the resets inside
 * imgenv_step_autoreset / imgenv_step_autoreset_device) appends one record per episode it closes, on the caller's stream, with no
 * host synchronisation, allocation or copy: one extra launch per RESET chain (csrc/episode_log.h, in front of the fold); a step
 * chain launches nothing new.
 *
 * A reset chain covers robot rows in a fixed order (every local robot ascending, or robot by robot of the worlds it lists, in list
 * order); each covered robot with an open episode (imgenv_episodes_out.open != 0) appends one record, in that order -- the log is
 * deterministic: chains in stream order, rows in chain order.  Record q (counted from enabling) lives in slot q % capacity.
 *   robot     the local row; world = row / robots-per-world (0 on a robot shard)
 *   code      the last step's imgenv_out.step_dones_info;  steps, len, ep_return: open_steps, open_len and the open return
 *   counted   steps > min_steps;  episode: the robot's `episodes` after this fold (0 when not counted)
 *   figures   the IMGENV_EP_FIGURES figures this fold adds to figure_sums (zeros when not counted: a short episode's commands ride
 *             into the next counted one, as above)
 *   map, tracks, scenario_raw, placement   what the episode ran on, noted when it OPENED -- every covered robot, open or not, takes
 *             them for the episode that starts: its world's map of the bank (0 without one), its track set (-1 without a bank or
 *             where the reset brought its own tracks), the scenario of a host reset or IMGENV_EPLOG_SCN_DEVICE where the device
 *             placed the world (-1 without a scenario bank), and the world's placement number (imgenv_world_placement; ~0: none).
 *   Episodes already open when the log is enabled carry map -1, tracks -1, scenario_raw -1 and placement ~0.
 * imgenv_episodes_clear does not touch the log; `episode` follows the cleared counter. */
#define IMGENV_EPLOG_MAX_CAPACITY (1 << 22)
#define IMGENV_EPLOG_I32 10   /* rows of i32: robot, world, code, steps, len, counted, episode, map, tracks, scenario_raw */
#define IMGENV_EPLOG_F64 9    /* rows of f64: ep_return, then the IMGENV_EP_FIGURES figures in their order */
#define IMGENV_EPLOG_SCN_DEVICE (-2) /* scenario_raw: placed by the device; the id follows from `placement` */
typedef struct imgenv_episode_log_cfg {
    int32_t struct_size;          /* sizeof(imgenv_episode_log_cfg) */
    int32_t capacity;             /* records the ring holds: 1 .. IMGENV_EPLOG_MAX_CAPACITY */
} imgenv_episode_log_cfg;
typedef struct imgenv_episode_log_out {
    int32_t struct_size;          /* on entry 0 or sizeof(imgenv_episode_log_out) */
    int32_t capacity;
    uint64_t* n_written;          /* [1]  records appended since enabling; record q lives in slot q % capacity */
    int32_t* i32;                 /* [IMGENV_EPLOG_I32][capacity] */
    double* f64;                  /* [IMGENV_EPLOG_F64][capacity] */
    uint64_t* placement;          /* [capacity] place_serial of the episode's world when it opened, ~0: none */
} imgenv_episode_log_out;
typedef struct imgenv_episode_record {  /* 128 bytes, what imgenv_episode_log_read hands to the host */
    uint64_t seq, placement;
    int32_t robot, world, code, steps, len, counted, episode, map, tracks, scenario;
    double ep_return, figures[8];
} imgenv_episode_record;
/* IMGENV_ESTATE before imgenv_episodes_enable(); IMGENV_EINVAL for a wrong struct_size, a capacity outside 1 ..
 * IMGENV_EPLOG_MAX_CAPACITY, or a second call with another capacity; the same capacity again changes nothing and hands out the same
 * pointers.  IMGENV_ENOMEM, like IMGENV_EDEVICE, leaves the handle unchanged.  The memory is the library's (zeroed); `out` may be
 * NULL.  A handle that never calls it behaves, launch for launch, as if this section did not exist. */
int imgenv_episode_log_enable(imgenv_t* h, const imgenv_episode_log_cfg* cfg, imgenv_episode_log_out* out);
/* IMGENV_ESTATE before imgenv_episode_log_enable() */
int imgenv_episode_log_outputs(imgenv_t* h, imgenv_episode_log_out* out);
/* The records on the host.  Synchronises `stream`, like imgenv_world_scenarios.  *oldest = max(0, n_written - capacity) and
 * *n_written as they stand then (either may be NULL); the records with seq in [max(first, oldest), min(first + max, n_written)) are
 * copied to rec[] in order and their number is returned (a negative IMGENV_E* on failure).  rec may be NULL when max is 0.
 * `scenario` is what imgenv_world_scenarios would have answered for the record's world while the episode ran: scenario_raw where the
 * host reset the world, the scenario the placement's policy epoch gives its placement number for IMGENV_EPLOG_SCN_DEVICE, -1 without
 * a bank.  The handle's CURRENT seed0 and epoch table are used: read before the pool of imgenv_step_autoreset_device is rebuilt for
 * another spawn cfg. */
int64_t imgenv_episode_log_read(imgenv_t* h, uint64_t first, int32_t max, imgenv_episode_record* rec, uint64_t* oldest, uint64_t* n_written,
                                void* stream);

/* ---- action decoding: VelActionWrapper.action (envs/wrapper/base.py:37-66, envs/action/action.py:8-38) and the `speeds` of
 * info (base.py:58) as MultiRobotCleanWrapper masks them (base.py:81-83), for every local robot, on the device ----
 * The step functions take float32 [R][3] = (v, w, beep).  A policy trained on a YAML with discrete_action: True emits one index
 * into discrete_actions per robot; one trained on continuous_actions emits raw floats that the wrapper clips.  With action
 * decoding enabled the library turns either into the (v, w, beep) rows itself: imgenv_actions_decode queues ONE launch
 * (k_actions, csrc/actions.h) on the caller's stream that fills the handle-owned `actions` and `speeds`; the caller then passes
 * imgenv_actions_out.actions to any imgenv_step*, imgenv_step_begin or imgenv_step_autoreset* call ON THE SAME STREAM.  No step
 * entry point changes, and a handle that never enables this behaves, launch for launch, as if this section did not exist.
 *
 * Per local robot r (a robot shard decodes its local rows; `raw` is [R] or [R][n_cols], contiguous, naturally aligned):
 *   TABLE mode, integer raw [R]        actions[r] = table[raw[r]] (a two-column row of the YAML has beep 0, action.py:29-30).  An
 *                                      index outside [0, n_table) gives (0, 0, 0) and is counted in n_bad; it is never read.
 *                                      (Python would wrap a negative index: a stated deviation.)
 *   TABLE mode, float raw [R][n_cols]  ContinuousAction(*x) (base.py:43): rounded to float32, not clipped, beep 0 when n_cols is 2
 *   CLIP mode, float raw [R][n_cols]   column i: x = float32(raw), x = x >= float32(lo_i) ? x : float32(lo_i), then
 *                                      x = x <= float32(hi_i) ? x : float32(hi_i) (np.clip per component, base.py:45-51; float64
 *                                      input is rounded first -- rounding is monotone, so this is the reference's clip in double
 *                                      put on the float32 wire); beep 0 when n_cols is 2.  Integer raw is IMGENV_EINVAL.
 *   a component that is not finite -- as it came, or once it is float32 (a double beyond float32 that nothing clipped) -- makes
 *   the whole row (0, 0, 0) and is counted in n_bad.  The reference would carry a NaN into the node; the library must not: cell
 *   indices are rounded poses.  n_bad is a counter (it only grows), not an error state.
 *   speeds[r] = (v, w) of the decoded row where the robot is clean, (0, 0) where it is not: `clean` is MultiRobotCleanWrapper's
 *   state as the last step left it (1 after a reset) -- the is_clean of BEFORE the step, which the step then hands out as
 *   imgenv_out.step_is_clean and which the reference masks info["speeds"] with.
 * Ordering: the decode sits on the caller's stream in front of the step's first launch, and every reader of the actions is
 * ordered behind that launch; `actions` and `speeds` are overwritten only by the next decode, which the caller queues behind the
 * end of the step's chain.  The decode counts as one launch in the imgenv_step_launches of the step that follows it. */
#define IMGENV_ACTIONS_TABLE 0
#define IMGENV_ACTIONS_CLIP 1
#define IMGENV_ACTIONS_MAX_TABLE 4096
#define IMGENV_RAW_I32 0   /* `dtype` of imgenv_actions_decode */
#define IMGENV_RAW_I64 1
#define IMGENV_RAW_F32 2
#define IMGENV_RAW_F64 3
typedef struct imgenv_actions_cfg {
    int32_t struct_size;          /* sizeof(imgenv_actions_cfg) */
    int32_t mode;                 /* IMGENV_ACTIONS_TABLE (the YAML's discrete_action: True) | IMGENV_ACTIONS_CLIP */
    int32_t n_cols;               /* columns of a float `raw` row: 2 (v, w) or 3 (v, w, beep) -- the YAML's act_dim */
    int32_t n_table;              /* TABLE mode: rows of `table`, 1 .. IMGENV_ACTIONS_MAX_TABLE */
    const float* table;           /* TABLE mode: HOST [n_table][3] = v, w, beep, every value finite; copied by the call */
    float clip[3][2];             /* CLIP mode: (lo, hi) of column i < n_cols (the YAML's continuous_actions), finite, lo <= hi */
} imgenv_actions_cfg;
/* Device pointers, R = robot_end - robot_begin local robots; owned by the handle, valid until imgenv_destroy(), contents valid
 * once the stream work of the last imgenv_actions_decode has completed, READ-ONLY for the caller. */
typedef struct imgenv_actions_out {
    int32_t struct_size;          /* on entry 0 or sizeof(imgenv_actions_out) */
    int32_t n_local;              /* R */
    float* actions;               /* [R][3]  what the step functions take */
    float* speeds;                /* [R][2]  info["speeds"] */
    int32_t* n_bad;               /* [1]     rows zeroed so far (out-of-range index, non-finite component) */
} imgenv_actions_out;
/* Legal at any time; the memory is the library's.  IMGENV_EINVAL for a wrong struct_size, an unknown mode, n_cols outside {2, 3},
 * TABLE mode with a null, empty, over-long or non-finite table, CLIP mode with lo > hi or a bound that is not finite in a column
 * < n_cols, or a second call whose cfg differs from the first's (same cfg: nothing changes, same pointers).  `out` may be NULL. */
int imgenv_actions_enable(imgenv_t* h, const imgenv_actions_cfg* cfg, imgenv_actions_out* out);
/* IMGENV_ESTATE before imgenv_actions_enable() */
int imgenv_actions_outputs(imgenv_t* h, imgenv_actions_out* out);
/* `raw`: DEVICE pointer, [R] of dtype I32 / I64 (TABLE mode only) or [R][n_cols] of F32 / F64, aligned to its element size, valid
 * until the launch has run.  IMGENV_ESTATE before imgenv_actions_enable() or before the first reset; IMGENV_EINVAL for a null or
 * misaligned `raw`, an unknown dtype, or integer `raw` in CLIP mode. */
int imgenv_actions_decode(imgenv_t* h, const void* raw, int32_t dtype, void* stream);

/* ---- the policy head: sample the action from the policy's distribution, on the device ----
 * A policy emits neither an index nor a raw row: it emits logits over the YAML's discrete_actions, or a mean and a log-std over
 * its continuous_actions.  With the policy head enabled, imgenv_policy_sample queues ONE launch (k_policy_*, csrc/policy.h) on the
 * caller's stream that draws the action (or takes the mode), computes its log-probability and the distribution's entropy, decodes
 * it into the handle-owned imgenv_actions_out.actions / speeds exactly as imgenv_actions_decode would have decoded the drawn index
 * / the drawn raw row, adds the bad rows to imgenv_actions_out.n_bad, and -- with IMGENV_POLICY_STORE -- keeps the action, its
 * log-probability and the caller's value estimate in the slot of the rollout window the next transition starts from.  Ordering,
 * ownership and the imgenv_step_launches accounting (one launch, counted with the step that follows) are imgenv_actions_decode's.
 * Opt-in: a handle that never enables it launches exactly what it launched before.
 *
 * Random numbers: Philox4x32-10, stateless.  counter = (g lo, g hi, draw lo, draw hi) with g = robot_begin + r the GLOBAL robot
 * number -- a robot shard draws what the whole world draws -- key = (seed lo, seed hi); `seed` is the cfg's, `draw` the caller's
 * (one per call: the library keeps no generator state).  u = float(x0 >> 8) * 2^-24, in [0, 1).
 *
 * CATEGORICAL (needs imgenv_actions_enable in TABLE mode), per local robot row of A = n_table float32 logits, float32 throughout:
 *   a -inf logit is a masked action and is legal.  A NaN, a +inf or a row without a finite logit is a bad row: actions (0, 0, 0),
 *   index -1, logp 0, entropy 0, counted in n_bad.  Otherwise, with m = max_k l_k: e_k = expf(l_k - m) (0 where masked),
 *   s = sum e_k, logp_k = (l_k - m) - logf(s), entropy = -sum over e_k > 0 of (e_k / s) logp_k.  The draw: target = u s; index =
 *   the smallest k with e_k > 0 whose inclusive cumulative sum exceeds target; if none does (u s rounded up to s), the largest k
 *   with e_k > 0.  A masked action is never chosen.  DETERMINISTIC: the smallest k with l_k == m.  The order of every sum and of
 *   the cumulative sum is fixed (csrc/policy.h states it; it depends on A alone): two runs give identical bits.
 * GAUSSIAN (needs CLIP mode), C = n_cols independent normals per row: sigma = expf(log_std); u1 = float((x0 >> 8) + 1) * 2^-24,
 *   u2 = float(x1 >> 8) * 2^-24, rho = sqrtf(-2 logf(u1)), z0 = rho cosf(2 pi u2), z1 = rho sinf(2 pi u2); column 2 takes z0 of a
 *   second block whose counter has draw hi ^ 0x80000000.  raw = mean + sigma z; logp = sum_c (-0.5 z^2 - log_std - 0.5 ln 2 pi),
 *   the log-probability of the UNCLIPPED sample; entropy = sum_c (0.5 + 0.5 ln 2 pi + log_std).  DETERMINISTIC: z = 0.  A mean,
 *   log_std, sigma or raw that is not finite makes a bad row: raw 0, actions (0, 0, 0), logp 0, entropy 0, counted.  actions =
 *   the CLIP rule of imgenv_actions_decode on raw.
 * STORE (cfg.flags; needs imgenv_rollout_enable first): pol_raw / pol_logp / pol_value are [.][T][R] arrays in the layout
 *   imgenv_minibatch_args.scalars takes (row stride R), a separate all-or-nothing allocation.  A sample without NO_STORE writes
 *   slot n = the rollout cursor at the time of the call (imgenv_rollout_out.n, the host's); pol_value[n] only where `values` is
 *   given.  n < 0 (before imgenv_rollout_begin) or n >= T is IMGENV_ESTATE; n == T is legal for VALUE_ONLY alone, which copies
 *   `values` into pol_value[n] -- the bootstrap value of the window's last state -- and does nothing else (it is no part of a step
 *   and is not counted in imgenv_step_launches).  Nothing is queued on failure. */
#define IMGENV_POLICY_CATEGORICAL 0      /* needs imgenv_actions_enable in TABLE mode: A = n_table logits per robot */
#define IMGENV_POLICY_GAUSSIAN    1      /* needs CLIP mode: C = n_cols (2 or 3) independent normals per robot */
#define IMGENV_POLICY_STORE       1      /* cfg.flags: keep the policy columns in the rollout ring (needs imgenv_rollout_enable) */
#define IMGENV_POLICY_DETERMINISTIC   1  /* args.flags: the mode instead of a draw */
#define IMGENV_POLICY_LOG_STD_PER_ROW 2  /* args.flags: log_std is [R][C] instead of [C] */
#define IMGENV_POLICY_NO_STORE        4  /* args.flags: this call does not touch the ring (evaluation between windows) */
#define IMGENV_POLICY_VALUE_ONLY      8  /* args.flags: only values -> pol_value[n] (the bootstrap slot, n == T allowed) */
typedef struct imgenv_policy_cfg {
    int32_t struct_size;          /* sizeof(imgenv_policy_cfg) */
    int32_t kind;                 /* IMGENV_POLICY_CATEGORICAL | IMGENV_POLICY_GAUSSIAN */
    int32_t flags;                /* 0 | IMGENV_POLICY_STORE */
    int32_t reserved;             /* 0 */
    uint64_t seed;                /* the Philox key */
} imgenv_policy_cfg;
/* Device pointers, R = robot_end - robot_begin local robots; owned by the handle, valid until imgenv_destroy(), contents valid once
 * the stream work of the last imgenv_policy_sample has completed, READ-ONLY for the caller. */
typedef struct imgenv_policy_out {
    int32_t struct_size;          /* on entry 0 or sizeof(imgenv_policy_out) */
    int32_t n_local;              /* R */
    int32_t n_params;             /* A or C */
    int32_t horizon;              /* T or 0 */
    int32_t* index;               /* [R]        CATEGORICAL: the action drawn, -1 for a bad row; NULL for GAUSSIAN */
    float* raw;                   /* [R][C]     GAUSSIAN: the unclipped sample (what PPO's loss needs); NULL for CATEGORICAL */
    float* logp;                  /* [R] */
    float* entropy;               /* [R] */
    float* pol_raw;               /* [C'][T][R] STORE only: C' = 1 (the index as float32, exact up to 4096; -1 bad) or C */
    float* pol_logp;              /* [T][R]     STORE only */
    float* pol_value;             /* [T+1][R]   STORE only */
} imgenv_policy_out;
typedef struct imgenv_policy_args {
    int32_t struct_size;          /* sizeof(imgenv_policy_args) */
    int32_t flags;                /* IMGENV_POLICY_DETERMINISTIC | _LOG_STD_PER_ROW | _NO_STORE, or _VALUE_ONLY alone */
    uint64_t draw;                /* the draw number: the caller's, a new one for every call that must differ */
    const float* params;          /* DEVICE f32: logits [R][A] | mean [R][C] */
    const float* log_std;         /* DEVICE f32 [C] or [R][C]; GAUSSIAN only */
    const float* values;          /* DEVICE f32 [R] or NULL */
} imgenv_policy_args;
/* Legal once imgenv_actions_enable() has been called (IMGENV_ESTATE before it; with IMGENV_POLICY_STORE also before
 * imgenv_rollout_enable()).  IMGENV_EINVAL for a wrong struct_size, an unknown kind or flag, reserved != 0, a kind the handle's
 * action mode does not serve (CATEGORICAL needs TABLE, GAUSSIAN needs CLIP), or a second call whose cfg differs from the first's
 * (same cfg: nothing changes, same pointers).  IMGENV_ENOMEM leaves the handle as it was.  `out` may be NULL. */
int imgenv_policy_enable(imgenv_t* h, const imgenv_policy_cfg* cfg, imgenv_policy_out* out);
/* IMGENV_ESTATE before imgenv_policy_enable() */
int imgenv_policy_outputs(imgenv_t* h, imgenv_policy_out* out);
/* The pointers of `args` are DEVICE pointers, contiguous, 4-byte aligned, valid until the launch has run.  IMGENV_ESTATE before
 * imgenv_policy_enable() or before the first reset, for a storing call outside the window (see STORE above) and for VALUE_ONLY on a
 * head without IMGENV_POLICY_STORE; IMGENV_EINVAL for a wrong struct_size, an unknown flag, VALUE_ONLY beside another flag,
 * LOG_STD_PER_ROW on a categorical head, a null or misaligned params (log_std for GAUSSIAN, values for VALUE_ONLY) or a
 * misaligned values. */
int imgenv_policy_sample(imgenv_t* h, const imgenv_policy_args* args, void* stream);

/* ---- PPO's loss: log-probabilities of STORED actions under new parameters, the loss and its gradients, on the device ----
 * For every minibatch of every epoch a trainer evaluates the stored actions under the network's new outputs and needs the
 * clipped-surrogate loss and its gradient on those outputs.  imgenv_policy_loss queues THREE launches (k_ploss_*,
 * csrc/policy_loss.h: the rows, one fold, the gradients) on the caller's stream, without atomics and in a fixed order of every
 * sum: two calls give identical bits.  Opt-in: a handle that never enables it allocates and launches exactly what it did; the
 * launches are no part of a step and are not counted in imgenv_step_launches.
 *
 * Over the B = args.rows rows, row i with weight w_i (imgenv_minibatch_out.mb_weight), in float32 per row, float64 in the sums:
 *   W        = max(sum_i w_i, 1)
 *   logp_i, H_i   log-probability of the stored action and entropy under the new parameters -- CATEGORICAL: imgenv_policy_sample's
 *              arithmetic on the same lanes (unchanged logits give the stored logp bit for bit; a -inf logit has p = 0 and adds
 *              nothing to H); GAUSSIAN: z = (raw - mean) / expf(log_std), logp = sum_c (-0.5 z^2 - log_std - 0.5 ln 2 pi),
 *              H = sum_c (0.5 + 0.5 ln 2 pi + log_std)
 *   r_i      = expf(logp_i - old_logp_i)
 *   pg_i     = -min(r_i adv_i, clamp(r_i, 1 - clip, 1 + clip) adv_i)
 *   vl_i     = 0.5 (v_i - ret_i)^2, or with IMGENV_PLOSS_CLIP_VALUE 0.5 max((v_i - ret_i)^2, (vc_i - ret_i)^2),
 *              vc_i = old_v_i + clamp(v_i - old_v_i, -clip_vf, clip_vf)
 *   loss     = sum_i w_i (pg_i + vf_coef vl_i - ent_coef H_i) / W
 *   stats[8] = loss, sum w pg / W, sum w vl / W, sum w H / W, sum w ((r - 1) - ln r) / W (approximate KL),
 *              sum w [|r - 1| > clip] / W (clip fraction), sum w (unclamped), 0
 * and the gradients of loss, closed forms: with active_i = (r_i adv_i <= clamp(r_i) adv_i), g_i = (w_i / W)(active_i ? -adv_i r_i : 0),
 * gH_i = -ent_coef w_i / W:
 *   CATEGORICAL  d_params[i][k] = g_i ([k == a_i] - p_ik) - gH_i p_ik (ln p_ik + H_i); a masked k gets exactly 0
 *   GAUSSIAN     d_params[i][c] = g_i z_ic / sigma_c;  d_log_std[i][c] = g_i (z_ic^2 - 1) + gH_i;  d_log_std_shared[c] = their sum
 *                over the rows (what a shared log_std [C] receives)
 *   d_values[i]  = vf_coef (w_i / W) (v_i - ret_i); with CLIP_VALUE where the clipped square is strictly the larger:
 *                vf_coef (w_i / W) (vc_i - ret_i) [|v_i - old_v_i| <= clip_vf]
 * A row is BAD with a NaN or +inf parameter, no finite logit, a stored action that is no integer in [0, A) or is masked (-inf)
 * under the new logits, a Gaussian log_std whose sigma or z is not finite, or a non-finite old_logp, adv, ret, value, old value,
 * ratio or weight.  A bad row and a row of weight 0 (the slots behind a minibatch's valid list) count as weight 0 and every
 * output and gradient of theirs is +0; n_bad, written fresh by every call, counts the bad rows whose own weight was not 0. */
#define IMGENV_PLOSS_CLIP_VALUE 1        /* args.flags (beside IMGENV_POLICY_LOG_STD_PER_ROW = 2) */
typedef struct imgenv_policy_loss_cfg {
    int32_t struct_size;          /* sizeof(imgenv_policy_loss_cfg) */
    int32_t max_rows;             /* the largest B of a call, >= 1 */
    int32_t reserved[2];          /* 0 */
} imgenv_policy_loss_cfg;
/* Device pointers; owned by the handle, valid until imgenv_destroy(), contents valid once the stream work of the last
 * imgenv_policy_loss has completed (rows [0, args.rows) of the row arrays), READ-ONLY for the caller. */
typedef struct imgenv_policy_loss_out {
    int32_t struct_size;          /* on entry 0 or sizeof(imgenv_policy_loss_out) */
    int32_t n_params;             /* A or C */
    int32_t max_rows;
    int32_t reserved;
    float* logp;                  /* [max_rows] */
    float* entropy;               /* [max_rows] */
    float* ratio;                 /* [max_rows] */
    float* pg;                    /* [max_rows] */
    float* vl;                    /* [max_rows] */
    float* d_params;              /* [max_rows][A | C], rows packed: row i at i * n_params */
    float* d_log_std;             /* [max_rows][C]  GAUSSIAN; NULL for CATEGORICAL */
    float* d_log_std_shared;      /* [C]            GAUSSIAN; NULL for CATEGORICAL */
    float* d_values;              /* [max_rows] */
    float* stats;                 /* [8] */
    int32_t* n_bad;               /* [1] */
    float* inv_w;                 /* [1] (float)(1 / W) */
} imgenv_policy_loss_out;
typedef struct imgenv_policy_loss_args {
    int32_t struct_size;          /* sizeof(imgenv_policy_loss_args) */
    int32_t flags;                /* IMGENV_PLOSS_CLIP_VALUE | IMGENV_POLICY_LOG_STD_PER_ROW */
    int32_t rows;                 /* B: 1 .. max_rows */
    int32_t reserved;             /* 0 */
    const float* params;          /* the network's NEW outputs, DEVICE f32: logits [B][A] | mean [B][C] */
    const float* log_std;         /* [C] or [B][C]; GAUSSIAN only */
    const float* values;          /* [B] */
    const float* action[3];       /* [B] each: the index as float32 (pol_raw) | the C raw columns; the rest NULL */
    const float* old_logp;        /* [B] */
    const float* old_value;       /* [B]; NULL without IMGENV_PLOSS_CLIP_VALUE */
    const float* adv;             /* [B] */
    const float* ret;             /* [B] */
    const float* weight;          /* [B] */
    float clip, clip_vf, vf_coef, ent_coef;
} imgenv_policy_loss_args;
/* Legal once imgenv_policy_enable() has been called (IMGENV_ESTATE before it); it does not need the rollout.  One all-or-nothing
 * block, every array on a 256-byte boundary.  IMGENV_EINVAL for a wrong struct_size, max_rows < 1, reserved != 0 or a second
 * call whose cfg differs (same cfg: nothing changes, same pointers).  IMGENV_ENOMEM leaves the handle as it was.  `out` may be NULL. */
int imgenv_policy_loss_enable(imgenv_t* h, const imgenv_policy_loss_cfg* cfg, imgenv_policy_loss_out* out);
/* IMGENV_ESTATE before imgenv_policy_loss_enable() */
int imgenv_policy_loss_outputs(imgenv_t* h, imgenv_policy_loss_out* out);
/* The [B] inputs are what imgenv_rollout_minibatch leaves in mb_scalars' rows and mb_weight.  Pointers are DEVICE pointers,
 * contiguous, 4-byte aligned, valid until the launches have run.  IMGENV_ESTATE before imgenv_policy_loss_enable(); IMGENV_EINVAL
 * for a wrong struct_size, an unknown flag, reserved != 0, rows out of 1 .. max_rows, a null or misaligned pointer (log_std for
 * GAUSSIAN, old_value with CLIP_VALUE, action[c] for c < 1 | C), clip < 0 or NaN, clip_vf < 0 or NaN with CLIP_VALUE, and
 * LOG_STD_PER_ROW on a categorical head.  Nothing is queued on failure. */
int imgenv_policy_loss(imgenv_t* h, const imgenv_policy_loss_args* args, void* stream);

/* ---- observation post-processing: StatePedVectorWrapper (envs/wrapper/base.py:19-34) and InfoLogWrapper's
 * bool_get_close_to_human (base.py:250-252) for every local robot, on the device ----
 * One extra launch at the end of every chain (k_obs_post, csrc/obs_post.h; behind the stacks and the episode statistics): a step
 * covers every local robot, a reset the robots of the worlds it resets.  Per robot row of imgenv_out.ped_vector_states:
 *   n = min(int(row[0]), max_ped); ped_vector_norm[0] = row[0];
 *   for j < n, c < 7: ped_vector_norm[1 + 7 j + c] = float32((double(row[1 + 7 j + c]) - avg[c]) / std[c]) -- the reference's
 *   float32 slice minus and divided by float64 constants, stored back into the float32 row; the padding behind n is copied.
 *   close_to_human[r] = imgenv_out.ped_min_dists[r] < close_dist (the reference's close_dist is 1).
 * The results go to arrays of their own: imgenv_out.ped_vector_states stays the raw vector (normalising it in place is not
 * offered: the observation kernel and the output guards own that array). */
#define IMGENV_OBS_PED_NORM 1     /* needs imgenv_cfg.ped_vec_dim == 7 */
#define IMGENV_OBS_CLOSE 2        /* needs a handle with pedestrians */
typedef struct imgenv_obs_post_cfg {
    int32_t struct_size;          /* sizeof(imgenv_obs_post_cfg) */
    int32_t flags;                /* IMGENV_OBS_PED_NORM | IMGENV_OBS_CLOSE, at least one */
    double avg[7], std[7];        /* PED_NORM: the reference's are (0, 0, 0, 0, 0.25, 0.25, 0) and (6, 6, 0.6, 0.9, 0.5, 0.5, 6) */
    double close_dist;            /* CLOSE */
} imgenv_obs_post_cfg;
typedef struct imgenv_obs_post_out {
    int32_t struct_size;          /* on entry 0 or sizeof(imgenv_obs_post_out) */
    int32_t n_local;              /* R */
    float* ped_vector_norm;       /* [R][1 + 7 max_ped]; NULL without IMGENV_OBS_PED_NORM */
    uint8_t* close_to_human;      /* [R]; NULL without IMGENV_OBS_CLOSE */
} imgenv_obs_post_out;
/* Legal at any time (the arrays are zero until the next chain has run); the memory is the library's, ownership as for
 * imgenv_actions_out.  IMGENV_EINVAL for a wrong struct_size, no or unknown flags, PED_NORM with std[c] == 0, a constant that is
 * not finite or ped_vec_dim != 7, CLOSE on a handle without pedestrians or with a close_dist that is not a number, or a second
 * call whose cfg differs from the first's (same cfg: nothing changes, same pointers).  `out` may be NULL. */
int imgenv_obs_post_enable(imgenv_t* h, const imgenv_obs_post_cfg* cfg, imgenv_obs_post_out* out);
/* IMGENV_ESTATE before imgenv_obs_post_enable() */
int imgenv_obs_post_outputs(imgenv_t* h, imgenv_obs_post_out* out);

/* ---- final observations: what an episode ended on (Gym's final_observation / terminal_observation), kept on the device ----
 * Every reset hands out the new episode's first observation in the rows of the robots it resets (NeverStopWrapper,
 * base.py:198-211): the observation the last action led to is written over in place.  A trainer that bootstraps the value of a
 * truncated episode (TimeLimitWrapper, dones_info == 10) needs it, and behind imgenv_step_autoreset_device the host never learns
 * which rows were reset.  With this feature every reset chain -- imgenv_reset, imgenv_reset_world(s), their spawn and scenario
 * variants, imgenv_step_autoreset, imgenv_step_autoreset_device -- starts with ONE extra launch (k_final_obs, csrc/final_obs.h)
 * that copies the present rows of the selected fields, for the robots that chain covers, into "final" arrays of the same shape
 * and row numbering, and adds 1 to final_count[row] of each of them.  A step chain launches nothing.  Rows no reset has covered
 * keep what they held (zero at first); nothing is cleared per step: final_count tells a fresh capture from an old one.  After
 * imgenv_step_autoreset(_device) the rows with imgenv_out.step_all_down set hold this step's final observation.  The handle's
 * first chain of launches captures nothing: there is no observation yet.
 * The copy is taken from the kernels' working arrays, also under IMGENV_FLAG_FULL_REWRITE; the final arrays are no part of
 * the output arena, so the output guards do not cover them.  Read-only for the caller; stream order as for imgenv_out.
 * Memory: one more copy of the selected fields, R x the sum of their row sizes + 4 R.  The default set at 48 x 48 views, 360
 * beams, ped_vec_len 71 and 48 x 48 pedestrian maps is 20 + 4608 + 2880 + 284 + 27648 + 18 = 35458 bytes per robot, 78 % of
 * it ped_maps. */
#define IMGENV_FINAL_VECTOR_STATES 1
#define IMGENV_FINAL_SENSOR_MAPS 2
#define IMGENV_FINAL_LASERS 4          /* needs use_laser */
#define IMGENV_FINAL_PED_VECTOR_STATES 8
#define IMGENV_FINAL_PED_MAPS 16
#define IMGENV_FINAL_IS_COLLISIONS 32
#define IMGENV_FINAL_IS_ARRIVES 64
#define IMGENV_FINAL_STEP_DS 128
#define IMGENV_FINAL_PED_MIN_DISTS 256
#define IMGENV_FINAL_VIEW_MAPS 512     /* not with IMGENV_FLAG_NO_VIEW_MAPS */
#define IMGENV_FINAL_LASERS_RAW 1024   /* needs use_laser */
#define IMGENV_FINAL_STACKS 2048       /* the stacks of depth >= 2 of imgenv_stack_enable(), whole [K][frame] rows, as the
                                        * step's push left them and before the reset restarts them */
#define IMGENV_FINAL_PED_NORM 4096     /* imgenv_obs_post_out.ped_vector_norm */
#define IMGENV_FINAL_IMAGE_STATE 511   /* the nine fields of ImageState (state.py:4-28): the first nine bits */
#define IMGENV_FINAL_ALL 8191
#define IMGENV_FINAL_NORM_STATES 8192  /* imgenv_normalise_out.norm_vector_states and, where it exists, norm_state_stack: needs
                                        * imgenv_normalise_enable() with IMGENV_NORM_OBS first (IMGENV_EINVAL otherwise); not part
                                        * of IMGENV_FINAL_ALL */
typedef struct imgenv_final_obs_cfg {
    int32_t struct_size;          /* sizeof(imgenv_final_obs_cfg) */
    int32_t fields;               /* IMGENV_FINAL_* bits, at least one */
} imgenv_final_obs_cfg;
typedef struct imgenv_final_obs_out {
    int32_t struct_size;          /* on entry 0 or sizeof(imgenv_final_obs_out) */
    int32_t n_local;              /* R */
    /* shapes and types as the fields of imgenv_out; NULL where not selected */
    float* vector_states;
    uint16_t* sensor_maps;
    double* lasers;
    float* ped_vector_states;
    float* ped_maps;
    int8_t* is_collisions;
    uint8_t* is_arrives;
    double* step_ds;
    double* ped_min_dists;
    uint8_t* view_maps;
    float* lasers_raw;
    /* IMGENV_FINAL_STACKS: shapes as imgenv_stack_out's; NULL for a field whose depth is below 2 (its stack of depth 1 is the
     * field itself: select the field) */
    uint16_t* stack_sensor_maps;
    float* stack_vector_states;
    double* stack_lasers;
    float* ped_vector_norm;       /* IMGENV_FINAL_PED_NORM: [R][1 + 7 max_ped] */
    uint32_t* final_count;        /* [R] captures of the row so far */
} imgenv_final_obs_out;
/* Legal at any time; the memory is the library's and lives until imgenv_destroy().  IMGENV_EINVAL for a wrong struct_size, no
 * or unknown bits, a field the handle does not produce (LASERS / LASERS_RAW without use_laser, VIEW_MAPS under
 * IMGENV_FLAG_NO_VIEW_MAPS, STACKS on a handle none of whose stacks is deeper than 1), or a second call whose cfg differs from
 * the first's (same cfg: nothing changes, same pointers).  IMGENV_ESTATE for STACKS before imgenv_stack_enable() and for
 * PED_NORM before imgenv_obs_post_enable() with IMGENV_OBS_PED_NORM.  IMGENV_ENOMEM when the arrays cannot be allocated; the
 * handle is then unchanged.  `out` may be NULL. */
int imgenv_final_obs_enable(imgenv_t* h, const imgenv_final_obs_cfg* cfg, imgenv_final_obs_out* out);
/* IMGENV_ESTATE before imgenv_final_obs_enable() */
int imgenv_final_obs_outputs(imgenv_t* h, imgenv_final_obs_out* out);

/* ---- rollout storage: a trainer's [T, R, ...] arrays kept on the device, and the advantage pass over them ----
 * The arrays of imgenv_out are working copies: the next step rewrites them and the stacks shift in place, so a trainer copies
 * every observation field, reward, done, mask and action away after every step.  With this feature the library does that, with ONE
 * extra launch per chain (k_rollout, csrc/rollout.h: the last launch of the chain, behind the observation post-processing whose
 * output it may read), and it knows two things a trainer does not: which rows a reset chain has just overwritten -- also behind
 * imgenv_step_autoreset_device -- and which transitions count (step_is_clean, dones_info).
 *
 * R = local robots, T = horizon, F = final_capacity.  Slot s of an obs array is the observation transition s starts from:
 *   obs_<field>    [T+1][R][row]   the selected fields, shapes and types of a row as in imgenv_out / imgenv_stack_out /
 *                                  imgenv_obs_post_out; always read from the kernels' working arena, also under
 *                                  IMGENV_FLAG_FULL_REWRITE
 *   actions        f32 [T][R][3]   the (v, w, beep) rows the step consumed (the decoded ones where imgenv_actions_decode feeds it)
 *   rewards        f32 [T][R]      imgenv_out.step_rewards rounded once to float32
 *   dones, is_clean u8 [T][R]      imgenv_out.step_dones, step_is_clean
 *   dones_info     i32 [T][R]      imgenv_out.step_dones_info
 *   final_idx      i32 [T+1][R]    -1, or the entry of the final list that holds what slot s showed for this row before a reset
 *                                  chain overwrote it (>= F: the entry was dropped)
 *   final_<field>  [F][row]        the overwritten rows
 *   final_slot, final_row i32 [F]  where each entry came from
 *   final_n        u32 [2]         entries so far, dropped ones included: reset chain number k since imgenv_rollout_begin reads
 *                                  final_n[k & 1] and writes final_n[(k + 1) & 1]; imgenv_rollout_out.resets is k, so the current
 *                                  count is final_n[resets & 1]
 * The cursor n (transitions stored) is kept by the host.  Nothing is stored before the first imgenv_rollout_begin().  From then on
 *   a step chain writes the transition into slot n and the observation it led to into slot n + 1, and n advances;
 *   a reset chain -- whoever queued it: imgenv_reset, imgenv_reset_world(s) and their variants, imgenv_step_autoreset(_device) --
 *     moves the rows of slot n it covers into the final list (entries are numbered in the chain's row order) and writes the new
 *     episode's first observation into slot n.  A row reset twice at the same slot keeps the later entry.
 * With n == T every step entry point (imgenv_step, _begin, _flags, imgenv_step_autoreset, _device) fails with IMGENV_EINVAL
 * ("rollout full: imgenv_rollout_begin") before it queues anything.
 * Memory: (T + 1) R x the selected rows + F x the same + 22 T R + 4 (T + 1) R + 8 F + 8 bytes (each array on a 256-byte
 * boundary).  The five single-frame fields at 48 x 48 views, 360 beams, ped_vec_len 71 and 48 x 48 pedestrian maps is about 35 KB per robot and slot -- about 18 GB for T = 128 at 4096 robots, 78 % of
 * it ped_maps: select what the policy reads, or IMGENV_ROLLOUT_PED_MAPS_DRAWN (7.8 KB per robot and slot, about 4.1 GB).  Single frames unless STACKS is selected.  Read-only for the caller; stream order as
 * for imgenv_out; no part of the output arena. */
#define IMGENV_ROLLOUT_SENSOR_MAPS 1
#define IMGENV_ROLLOUT_VECTOR_STATES 2
#define IMGENV_ROLLOUT_LASERS 4             /* needs use_laser */
#define IMGENV_ROLLOUT_PED_VECTOR_STATES 8
#define IMGENV_ROLLOUT_PED_MAPS 16
#define IMGENV_ROLLOUT_PED_NORM 32          /* imgenv_obs_post_out.ped_vector_norm: needs imgenv_obs_post_enable with IMGENV_OBS_PED_NORM */
#define IMGENV_ROLLOUT_STACKS 64            /* the whole [K][frame] rows of every stack of depth >= 2 of imgenv_stack_enable() */
#define IMGENV_ROLLOUT_ALL 127
/* the two below need imgenv_normalise_enable() first (IMGENV_EINVAL otherwise) and are not part of IMGENV_ROLLOUT_ALL */
#define IMGENV_ROLLOUT_NORM_STATES 128      /* imgenv_normalise_out.norm_vector_states and, where it exists, norm_state_stack (IMGENV_NORM_OBS);
                                             * the ring's pointers are imgenv_normalise_out.rollout_* / mb_norm_* */
#define IMGENV_ROLLOUT_NORM_REWARDS 256     /* `rewards` holds imgenv_normalise_out.norm_rewards instead of step_rewards (IMGENV_NORM_REWARD);
                                             * selects no field of its own: at least one other bit is needed */
/* not part of IMGENV_ROLLOUT_ALL: the ring keeps NO ped_maps (obs_ped_maps and final_ped_maps stay NULL, nothing is allocated for
 * them, k_rollout moves 78 % fewer bytes at the five single-frame fields) and the minibatches draw mb_ped_maps from the stored
 * ped_vector_states instead (imgenv_ped_maps_draw below has the definition): bit for bit the maps IMGENV_ROLLOUT_PED_MAPS would have
 * stored.  Needs IMGENV_ROLLOUT_PED_VECTOR_STATES in the same cfg and excludes IMGENV_ROLLOUT_PED_MAPS (IMGENV_EINVAL otherwise, and
 * for pedestrian maps beyond 16384 cells).  In imgenv_minibatch_cfg.fields the bit selects mb_ped_maps like any field; the
 * minibatch needs mb_ped_vector_states only if the caller selects that too. */
#define IMGENV_ROLLOUT_PED_MAPS_DRAWN 512
typedef struct imgenv_rollout_cfg {
    int32_t struct_size;          /* sizeof(imgenv_rollout_cfg) */
    int32_t horizon;              /* T >= 1 */
    int32_t final_capacity;       /* F >= 1 */
    int32_t fields;               /* IMGENV_ROLLOUT_* bits, at least one */
} imgenv_rollout_cfg;
typedef struct imgenv_rollout_out {
    int32_t struct_size;          /* on entry 0 or sizeof(imgenv_rollout_out) */
    int32_t n_local;              /* R */
    int32_t horizon;              /* T */
    int32_t final_capacity;       /* F */
    int32_t n;                    /* the cursor: transitions stored since imgenv_rollout_begin(); -1 before the first one */
    int32_t resets;               /* reset chains stored since imgenv_rollout_begin() */
    /* [T+1][R][row]; NULL where not selected (the stacks: where the depth is below 2 -- select the field itself) */
    uint16_t* obs_sensor_maps;
    float* obs_vector_states;
    double* obs_lasers;
    float* obs_ped_vector_states;
    float* obs_ped_maps;
    float* obs_ped_vector_norm;
    uint16_t* obs_stack_sensor_maps;
    float* obs_stack_vector_states;
    double* obs_stack_lasers;
    /* [F][row], NULL as above */
    uint16_t* final_sensor_maps;
    float* final_vector_states;
    double* final_lasers;
    float* final_ped_vector_states;
    float* final_ped_maps;
    float* final_ped_vector_norm;
    uint16_t* final_stack_sensor_maps;
    float* final_stack_vector_states;
    double* final_stack_lasers;
    float* actions;
    float* rewards;
    uint8_t* dones;
    uint8_t* is_clean;
    int32_t* dones_info;
    int32_t* final_idx;
    int32_t* final_slot;
    int32_t* final_row;
    uint32_t* final_n;
} imgenv_rollout_out;
/* Legal at any time; the memory is the library's (allocated all or nothing) and lives until imgenv_destroy().  IMGENV_EINVAL for
 * a wrong struct_size, horizon < 1, final_capacity < 1, (horizon + 1) x R beyond 2^31 - 1, no or unknown bits, a field the handle
 * does not produce (LASERS without use_laser, STACKS on a handle none of whose stacks is deeper than 1), or a second call whose cfg
 * differs from the first's (same cfg: nothing changes, same pointers).  IMGENV_ESTATE for STACKS before imgenv_stack_enable() and
 * for PED_NORM before imgenv_obs_post_enable() with IMGENV_OBS_PED_NORM.  IMGENV_ENOMEM when the arrays cannot be allocated; the
 * handle is then unchanged.  `out` may be NULL. */
int imgenv_rollout_enable(imgenv_t* h, const imgenv_rollout_cfg* cfg, imgenv_rollout_out* out);
/* the same struct with the cursor (n, resets) of this moment.  IMGENV_ESTATE before imgenv_rollout_enable() */
int imgenv_rollout_outputs(imgenv_t* h, imgenv_rollout_out* out);
/* Start (over): one launch copies the rows of slot n into slot 0 -- the first time the live arrays -- then final_idx becomes -1 and
 * final_n 0 by stream-ordered fills, and n = 0.  Nothing synchronises.  IMGENV_ESTATE before imgenv_rollout_enable() or before a
 * chain of launches has completed on the handle (there is no observation yet). */
int imgenv_rollout_begin(imgenv_t* h, void* stream);
/* Generalised advantage estimation over the n stored transitions, one launch (k_rollout_gae).  DEVICE pointers: `values` f32
 * [T+1][R], the caller's value estimate of every slot; `final_values` f32 [F], its estimate of every final entry, or NULL; `adv`
 * and `ret` f32 [T][R], of which rows t >= n are left untouched.  Everything is float32, per row and t = n - 1 .. 0:
 *   gl = gamma * lam                                                          (once)
 *   e        = final_idx[t+1][row]
 *   terminal = dones && dones_info != 10
 *   nv   = terminal ? 0 : e >= 0 ? ((e < F && final_values) ? final_values[e] : 0) : values[t+1][row]
 *   cont = (dones || e >= 0) ? 0 : 1
 *   if (!is_clean) { adv = 0; ret = 0; gae = 0 }
 *   else { m = gamma * nv; s = rewards + m; delta = s - values[t][row];
 *          c = gl * gae; c = cont ? c : 0; gae = delta + c; adv = gae; ret = gae + values[t][row] }
 * A real end bootstraps from nothing; a row whose next slot a reset overwrote (a time-out, or a caller's reset in mid-episode)
 * from the value of what the reset overwrote; anything else from the next slot, a time-out nobody has reset yet included.
 * IMGENV_EINVAL for a null values / adv / ret, IMGENV_ESTATE before imgenv_rollout_begin(). */
int imgenv_rollout_gae(imgenv_t* h, const float* values, const float* final_values, float gamma, float lam, float* adv, float* ret, void* stream);

/* ---- pedestrian maps drawn from pedestrian vectors ----
 * imgenv_out.ped_maps is a pure function of imgenv_out.ped_vector_states: k_obs stamps the discs from the float32 (px, py, vx, vy) it
 * stores as the first four of every pedestrian's seven floats, in rank order.  This draws the map again (k_ped_draw,
 * csrc/ped_draw.h), bit for bit, so that a trainer keeps the vector row (4 ped_vec_len bytes) instead of the map (12 Hp Wp bytes).
 * DEVICE pointers: ped_vectors f32 [.][PV], PV = ped_vec_len; rows i32 [n] or NULL; out f32 [n][3][Hp][Wp], (Hp, Wp) =
 * imgenv_cfg.ped_image_size.  Row i of out is drawn from row (rows ? rows[i] : i) of ped_vectors; every cell of it is written:
 *   n_ped = v[0] truncated to an integer and clamped to [0, (PV - 1) / 7]; 0 where v[0] is negative or not finite
 *   for q = 0 .. n_ped - 1, ascending: (px, py, vx, vy) = v[1 + 7 q .. 4 + 7 q]
 *     the pedestrian is skipped where (double)px > 3 or < -3, likewise py, or where px or py is not a number
 *     tmx = -(double)px + 3; tmy = -(double)py + 3
 *     jj runs over [floor((tmx - r) / res), floor((tmx + r) / res)), kk over the same with tmy, r = ped_image_r, res = 6 / Hp;
 *       floor(x / res) is floor(x * (1 / res)) where res is a power of two, Python's x // res otherwise
 *     cell (jj, kk) inside [0, Hp) x [0, Wp) takes the disc where ((jj + 0.5) res - tmx)^2 + ((kk + 0.5) res - tmy)^2 < r^2, in
 *       float64 and in this order
 *   a cell ends with the disc of the highest q that covers it: planes (1.0f, vx, vy), vx and vy copied bit for bit (-0.0f stays);
 *     a cell under no disc is 0.0f in all three planes
 *   a source row index below 0 gives an all-zero map (an index at or beyond the rows of ped_vectors is the caller's error)
 * One launch on `stream`: nothing synchronises and no state of the handle changes; no feature needs to be enabled.  n == 0 succeeds
 * and launches nothing.  IMGENV_EINVAL for a null handle, ped_vectors or out, n < 0, a handle without pedestrians (n_peds == 0 at
 * imgenv_create) and for pedestrian maps of more than 16384 cells (the kernel keeps a word of LDS per cell). */
int imgenv_ped_maps_draw(imgenv_t* h, const float* ped_vectors, const int32_t* rows, int64_t n, float* out, void* stream);

/* ---- rollout minibatches: which stored transitions count, a random order over them, their statistics, the gather ----
 * Between "T steps collected" and "optimiser step" a trainer finds the transitions that count (is_clean != 0: a frozen robot of
 * MultiRobotCleanWrapper has advantage 0), normalises its advantages over exactly those, draws a fresh order over them every epoch
 * and gathers every minibatch into contiguous tensors.  Here all of that is kernels over the ring (csrc/minibatch.h); nothing
 * reads the device from the host.  k = t * R + row numbers the stored transitions, 0 <= k < n * R (n the cursor).
 *
 * All arrays are the library's, one all-or-nothing allocation, each on a 256-byte boundary, no part of the output arena:
 *   valid        i32 [T R]      imgenv_rollout_index: the k with is_clean[k] != 0, ascending
 *   valid_n      u32            their count V
 *   order        i32 [T R]      imgenv_rollout_shuffle: order[p] = valid[pi(p)] for p < V, -1 from V on
 *   norm         f32 [2]        imgenv_rollout_stats' default target: (mean, 1 / sqrt(var + eps))
 *   tile_count, tile_base i32 [ceil(T R / 4096)], stat_part f64 [the same], stat_mean f64   scratch of the index and the statistics
 *   per buffer (imgenv_minibatch_buffer), B = batch:
 *   mb_<field>   [B][row]       the selected fields' rows, shapes and types as obs_<field>
 *   mb_actions f32 [B][3], mb_rewards f32 [B], mb_dones u8 [B], mb_dones_info i32 [B]   the ring's scalars of transition k
 *   mb_index     i32 [B]        k, -1 for a slot behind the valid list
 *   mb_weight    f32 [B]        1, or 0 for such a slot: a loss is (per_sample * w).sum() / w.sum().clamp(min = 1)
 *   mb_scalars   f32 [IMGENV_MB_MAX_SCALARS][B]   the caller's arrays at k
 * The index has a generation: the pair (n, chains queued on the handle so far) at the time of imgenv_rollout_index.  A later step
 * chain, reset chain or imgenv_rollout_begin makes it stale: imgenv_rollout_stats, _shuffle and _minibatch then fail with
 * IMGENV_ESTATE ("rollout changed since imgenv_rollout_index") before they queue anything.  Stream order as for imgenv_out: queue
 * these calls on the stream of the chains, or behind an event of it. */
#define IMGENV_MB_MAX_SCALARS 6
#define IMGENV_MB_MAX_BUFFERS 4
typedef struct imgenv_minibatch_cfg {
    int32_t struct_size;          /* sizeof(imgenv_minibatch_cfg) */
    int32_t batch;                /* B >= 1 */
    int32_t buffers;              /* 1 .. IMGENV_MB_MAX_BUFFERS */
    int32_t fields;               /* IMGENV_ROLLOUT_* bits, a subset of the rollout's; 0: all of them (mb_ped_maps too where the rollout
                                   * has IMGENV_ROLLOUT_PED_MAPS_DRAWN: one more launch per minibatch, k_ped_draw behind the gather) */
} imgenv_minibatch_cfg;
typedef struct imgenv_minibatch_buffer {
    /* [B][row]; NULL where not selected */
    uint16_t* mb_sensor_maps;
    float* mb_vector_states;
    double* mb_lasers;
    float* mb_ped_vector_states;
    float* mb_ped_maps;
    float* mb_ped_vector_norm;
    uint16_t* mb_stack_sensor_maps;
    float* mb_stack_vector_states;
    double* mb_stack_lasers;
    float* mb_actions;
    float* mb_rewards;
    uint8_t* mb_dones;
    int32_t* mb_dones_info;
    int32_t* mb_index;
    float* mb_weight;
    float* mb_scalars;
} imgenv_minibatch_buffer;
typedef struct imgenv_minibatch_out {
    int32_t struct_size;          /* on entry 0 or sizeof(imgenv_minibatch_out) */
    int32_t n_local;              /* R */
    int32_t horizon;              /* T */
    int32_t batch;                /* B */
    int32_t buffers;
    int32_t fields;               /* the bits in effect */
    int32_t* valid;
    int32_t* order;
    uint32_t* valid_n;
    float* norm;
    int32_t* tile_count;
    int32_t* tile_base;
    double* stat_part;
    double* stat_mean;
    imgenv_minibatch_buffer buf[IMGENV_MB_MAX_BUFFERS];  /* buf[b] all NULL for b >= buffers */
} imgenv_minibatch_out;
/* Legal once imgenv_rollout_enable() has been called (IMGENV_ESTATE before).  IMGENV_EINVAL for a wrong struct_size, batch < 1,
 * buffers outside 1 .. 4, unknown bits, a bit the rollout does not store, or a second call whose cfg differs from the first's
 * (same cfg: `out` is filled again, nothing changes).  IMGENV_ENOMEM when the arrays cannot be allocated; the handle is then
 * unchanged.  `out` may be NULL.  Nothing is launched, and no chain of the handle changes. */
int imgenv_rollout_minibatch_enable(imgenv_t* h, const imgenv_minibatch_cfg* cfg, imgenv_minibatch_out* out);
/* IMGENV_ESTATE before imgenv_rollout_minibatch_enable() */
int imgenv_rollout_minibatch_outputs(imgenv_t* h, imgenv_minibatch_out* out);
/* valid = the ascending list of every k < n R with is_clean[k] != 0, valid_n = its length: a stable compaction in three launches
 * (count per tile of 4096 flags, one workgroup's scan of the tile counts, scatter per tile); no workgroup waits for another.
 * Records the generation.  IMGENV_ESTATE before imgenv_rollout_minibatch_enable(), before imgenv_rollout_begin() or with n == 0. */
int imgenv_rollout_index(imgenv_t* h, void* stream);
/* Mean and inverse standard deviation of x -- a DEVICE f32 [T][R] array of the caller, typically adv -- over the valid list, in
 * float64: mean = sum x / V; then, in a second pass, var = sum (x - mean)^2 / V: the POPULATION variance (divisor V), not the
 * unbiased one torch.std defaults to.  norm_out (DEVICE f32 [2]; NULL: the library's norm) = ((float)mean, (float)(1 / sqrt(var +
 * eps))); V == 0: (0, 1); var + eps == 0: (mean, 1).  Four launches, partial sums in a fixed order, no atomics: two runs give
 * identical bits.  IMGENV_EINVAL for a null x or eps < 0, IMGENV_ESTATE for a stale or missing index. */
int imgenv_rollout_stats(imgenv_t* h, const float* x, double eps, float* norm_out, void* stream);
/* order[p] = valid[pi(p)] for p < valid_n (read on the device), -1 for valid_n <= p < T R; one launch.  pi is a cycle-walking,
 * unbalanced, alternating Feistel network; all arithmetic uint32, wrapping:
 *   fmix(x): x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13; x *= 0xc2b2ae35; x ^= x >> 16
 *   key[r] = fmix(seed_lo ^ (r * 0x9E3779B9)) ^ seed_hi, r = 0 .. 5
 *   V = valid_n; b = max(2, bit_length(V - 1)); hb = b / 2; ha = b - hb; mA = 2^ha - 1; mB = 2^hb - 1
 *   L = x >> hb; R = x & mB; even r: L ^= fmix(R + key[r]) & mA; odd r: R ^= fmix(L + key[r]) & mB; x = (L << hb) | R;
 *   the six rounds repeat while x >= V.  V <= 1: the identity.
 * IMGENV_ESTATE for a stale or missing index. */
int imgenv_rollout_shuffle(imgenv_t* h, uint32_t seed_lo, uint32_t seed_hi, void* stream);
typedef struct imgenv_minibatch_args {
    int32_t struct_size;          /* sizeof(imgenv_minibatch_args) */
    int32_t j;                    /* minibatch number >= 0: the slots take order[j B .. j B + B - 1] */
    int32_t buffer;               /* 0 .. buffers - 1 */
    int32_t n_scalars;            /* 0 .. IMGENV_MB_MAX_SCALARS */
    int32_t normalise;            /* an index into scalars, or -1 */
    int32_t reserved;             /* 0 */
    const float* scalars[IMGENV_MB_MAX_SCALARS];  /* DEVICE f32 arrays indexed by k, row stride R: [T][R] or [T+1][R] */
    const float* norm;            /* DEVICE f32 [2] for `normalise`; NULL: the library's norm */
} imgenv_minibatch_args;
/* Minibatch j into buffer `buffer`, one launch (k_rollout_gather).  Slot i takes k = order[j B + i], -1 from T R on.
 *   k >= 0: mb_<field>[i] = obs_<field>[k], the ring's actions / rewards / dones / dones_info of k, mb_index = k, mb_weight = 1,
 *           mb_scalars[s][i] = scalars[s][k], for s == normalise (x - norm[0]) * norm[1] in float32 (two roundings);
 *   k <  0: every byte of the slot's rows 0, mb_index = -1, mb_weight and every scalar 0.
 * Rows of mb_scalars from n_scalars on are left as they are.  IMGENV_EINVAL for a wrong struct_size, j < 0, a buffer, n_scalars or
 * normalise out of range or a null scalars[s]; IMGENV_ESTATE for a stale or missing index or before imgenv_rollout_shuffle() on
 * this index. */
int imgenv_rollout_minibatch(imgenv_t* h, const imgenv_minibatch_args* args, void* stream);

/* ---- running normalisation of the observation vector and of the reward (Stable-Baselines3's VecNormalize / RunningMeanStd) ----
 * Off by default: a handle that never calls imgenv_normalise_enable() launches what it launched before.  With it every chain ends
 * with at most two more launches (k_norm_part, k_norm_apply; csrc/normalise.h has the order of every sum), behind the stacks and
 * the observation post-processing and in front of the rollout storage, which may store their output.
 * State, float64, the library's: obs_count, obs_mean[state_dim], obs_var[state_dim]; ret_count, ret_mean, ret_var; returns[R], the
 * running discounted return of each robot's open episode.  Initial values: counts 1e-4, means 0, variances 1, returns 0.
 *   a step chain, training on:  returns[r] = returns[r] * gamma + step_rewards[r] for the rows with step_is_clean != 0; the batch --
 *     those rows' vector_states (float32 promoted) and new returns -- is reduced to (c, mean, M2) and merged into the running
 *     triples (Chan: delta = bm - mean; tot = count + c; mean += delta * c / tot; var = (var * count + M2 + delta * delta * count *
 *     c / tot) / tot); an empty batch leaves every bit; afterwards returns[r] = 0 where step_dones[r] is set;
 *   a reset chain, training on: the batch is the vector_states of the rows it covers, all of them; their returns become 0; the
 *     return statistics and norm_rewards are untouched;
 *   every chain, with the updated statistics, for the rows it covers (a step: all, frozen or not):
 *     norm_vector_states[r][d] = (float)clamp((x - obs_mean[d]) / sqrt(obs_var[d] + eps), -clip_obs, clip_obs), every frame of a
 *     state stack of depth >= 2 likewise into norm_state_stack (zero padding is normalised like any value; only the newest frame
 *     enters the statistics), and on a step norm_rewards[r] = clamp(step_rewards[r] / sqrt(ret_var + eps), -clip_reward, clip_reward);
 *   training off (imgenv_normalise_training): only the last item; no statistic and no return changes.
 * Every sum is taken in a fixed order without atomics: two runs give identical bits.  The arrays are no part of the output arena;
 * read-only for the caller; stream order as for imgenv_out. */
#define IMGENV_NORM_OBS 1
#define IMGENV_NORM_REWARD 2
typedef struct imgenv_normalise_cfg {
    int32_t struct_size;          /* sizeof(imgenv_normalise_cfg) */
    int32_t flags;                /* IMGENV_NORM_OBS | IMGENV_NORM_REWARD, at least one */
    double gamma;                 /* the returns' discount, 0 .. 1 (SB3: 0.99) */
    double clip_obs, clip_reward; /* > 0 (SB3: 10, 10) */
    double eps;                   /* > 0 (SB3: 1e-8) */
} imgenv_normalise_cfg;
typedef struct imgenv_normalise_out {
    int32_t struct_size;          /* on entry 0 or sizeof(imgenv_normalise_out) */
    int32_t n_local;              /* R */
    int32_t state_dim;
    int32_t state_depth;          /* K of norm_state_stack, 0 without one */
    float* norm_vector_states;    /* [R][state_dim]; NULL without IMGENV_NORM_OBS */
    float* norm_state_stack;      /* [R][K][state_dim]; NULL without IMGENV_NORM_OBS or where imgenv_stack_enable() -- called BEFORE
                                   * imgenv_normalise_enable() -- keeps no state stack of depth >= 2 */
    double* norm_rewards;         /* [R]; NULL without IMGENV_NORM_REWARD */
    double* stats;                /* [2][4 + 2 state_dim]: obs_count | ret_count | ret_mean | ret_var | obs_mean | obs_var; the
                                   * word of this moment is stats_word (a host-side count, as imgenv_rollout_out.n) */
    double* returns;              /* [2][R]; the word of this moment is returns_word; NULL without IMGENV_NORM_REWARD */
    int32_t stats_word, returns_word;
    int32_t training, reserved;
    /* IMGENV_ROLLOUT_NORM_STATES, once imgenv_rollout_enable() / imgenv_rollout_minibatch_enable() have run (NULL before; ask
     * imgenv_normalise_outputs() again): the ring's [T+1][R][row] and final list's [F][row] arrays of the two fields, and each
     * minibatch buffer's [B][row] -- imgenv_rollout_out and imgenv_minibatch_buffer keep their layout */
    float* rollout_obs_norm_vector_states;
    float* rollout_obs_norm_state_stack;
    float* rollout_final_norm_vector_states;
    float* rollout_final_norm_state_stack;
    float* mb_norm_vector_states[IMGENV_MB_MAX_BUFFERS];
    float* mb_norm_state_stack[IMGENV_MB_MAX_BUFFERS];
    /* IMGENV_FINAL_NORM_STATES, once imgenv_final_obs_enable() has run: [R][row] captures; imgenv_final_obs_out keeps its layout */
    float* final_norm_vector_states;
    float* final_norm_state_stack;
} imgenv_normalise_out;
/* host arrays for checkpoints: obs_mean / obs_var [state_dim], returns [n_rows] are the caller's (returns may be NULL) */
typedef struct imgenv_normalise_stats {
    int32_t struct_size;          /* sizeof(imgenv_normalise_stats) */
    int32_t state_dim, n_rows, reserved;  /* must equal the handle's state_dim and R */
    double obs_count, ret_count, ret_mean, ret_var;
    double* obs_mean;
    double* obs_var;
    double* returns;
} imgenv_normalise_stats;
/* Legal at any time, after imgenv_stack_enable() where the normalised stack is wanted; the memory is the library's.  IMGENV_EINVAL
 * for a wrong struct_size, no or unknown flags, a clip or eps that is not finite or not positive, gamma outside [0, 1], state_dim
 * + 1 > 64, or a second call (enabling twice).  A robot-sharded handle (robot_begin / robot_end) may enable it: its statistics are over
 * its LOCAL rows only -- every rank keeps its own, nothing is exchanged -- and a listed reset chain on it stays refused with
 * IMGENV_EINVAL before anything is queued (imgenv_step_autoreset_device: "needs all robots of every world on this handle";
 * csrc/tail_rows.h), which leaves every statistic and return as it was.  Training starts on.  `out` may be NULL. */
int imgenv_normalise_enable(imgenv_t* h, const imgenv_normalise_cfg* cfg, imgenv_normalise_out* out);
/* the same struct with the words of this moment.  IMGENV_ESTATE before imgenv_normalise_enable() */
int imgenv_normalise_outputs(imgenv_t* h, imgenv_normalise_out* out);
/* on != 0: the chains queued from now on update the statistics; 0: they only apply them (evaluation).  A host-side switch: nothing
 * is launched, `stream` is unused.  IMGENV_ESTATE before imgenv_normalise_enable() */
int imgenv_normalise_training(imgenv_t* h, int32_t on, void* stream);
/* The statistics and the returns of this moment into / out of host memory.  Both SYNCHRONISE the device.  _set makes the next
 * chain read the given values (a checkpoint, or a trainer's statistics handed to an evaluation handle); the normalised arrays
 * change with that chain, not before.  IMGENV_EINVAL for a wrong struct_size, state_dim or n_rows, null obs_mean / obs_var, or
 * (_set) a count, variance or return that is not finite, a count <= 0 or a variance < 0; IMGENV_ESTATE before imgenv_normalise_enable(). */
int imgenv_normalise_stats_get(imgenv_t* h, imgenv_normalise_stats* stats);
int imgenv_normalise_stats_set(imgenv_t* h, const imgenv_normalise_stats* stats);

/* ---- sequence minibatches: the window cut into chunks of L steps per row, for recurrent policies ----
 * imgenv_rollout_shuffle permutes single transitions; an LSTM or GRU policy needs each row's steps in order.  Here the window is
 * cut into sequences (csrc/sequences.h): with R local rows, horizon T, cursor n and a chunk length 1 <= L <= T there are
 * C = ceil(n / L) chunks per row (C_max = ceil(T / L)), and sequence q = c R + row, 0 <= q < C R, covers row `row`'s transitions
 * t = c L .. min(c L + L, n) - 1.  Chunks are aligned to the WINDOW, not to episodes: an episode boundary inside a chunk is marked
 * (mb_first), not split -- the env-major convention, the network resets its state where mb_first is set.  Needs
 * imgenv_rollout_enable(); does NOT need imgenv_rollout_minibatch_enable().
 *
 * All arrays are the library's, one all-or-nothing allocation, each on a 256-byte boundary:
 *   seq_flag     u8  [C_max R]  imgenv_rollout_seq_index: 1 iff any covered transition has is_clean != 0
 *   seq_valid    i32 [C_max R]  the q with seq_flag set, ascending;  seq_valid_n u32  their count Vs
 *   seq_order    i32 [C_max R]  imgenv_rollout_seq_shuffle: seq_order[p] = seq_valid[pi(p)] for p < Vs, -1 from Vs on
 *   tile_count, tile_base i32 [ceil(C_max R / 4096)]   the index's scratch
 *   per buffer (imgenv_seq_buffer), Bs = batch, TIME-MAJOR: x[l] is the contiguous batch a recurrent network consumes at step l
 *   mb_<field>   [L][Bs][row]   the selected fields' rows, shapes and types as obs_<field>
 *   mb_actions f32 [L][Bs][3], mb_rewards f32, mb_dones u8, mb_dones_info i32 [L][Bs]   the ring's scalars of transition k
 *   mb_index     i32 [L][Bs]    k = t R + row, -1 for a step that does not exist
 *   mb_weight    f32 [L][Bs]    is_clean[k] != 0 ? 1 : 0; 0 for a step that does not exist
 *   mb_first     u8  [L][Bs]    final_idx[t][row] >= 0: a reset chain rewrote slot t's observation, the row's episode STARTS at
 *                               this step (the device-side reset, the host-side ones, a caller's reset in mid-episode or at n = 0).
 *                               It does NOT say whether slot 0 continues the previous window: imgenv_rollout_begin clears final_idx,
 *                               and the caller's stored initial state (mb_seq_state) carries that.
 *   mb_scalars   f32 [IMGENV_MB_MAX_SCALARS][L][Bs]   the caller's arrays at k
 *   mb_seq       i32 [Bs]       q, or -1 for a slot behind the valid list
 *   mb_seq_len   i32 [Bs]       the steps of the slot with k >= 0
 *   mb_seq_state[a] u8 [Bs][state_bytes[a]]   the caller's row at the sequence's FIRST step, k0 = c L R + row; zeros where q = -1
 * The index has a generation exactly as imgenv_rollout_index's: a later chain or imgenv_rollout_begin makes it stale, and
 * imgenv_rollout_seq_shuffle / _seq_minibatch then fail with IMGENV_ESTATE ("rollout changed since imgenv_rollout_seq_index")
 * before they queue anything. */
#define IMGENV_SEQ_MAX_STATES 2
typedef struct imgenv_seq_cfg {
    int32_t struct_size;          /* sizeof(imgenv_seq_cfg) */
    int32_t length;               /* L: 1 .. the rollout's horizon */
    int32_t batch;                /* Bs >= 1 sequences per minibatch */
    int32_t buffers;              /* 1 .. IMGENV_MB_MAX_BUFFERS */
    int32_t fields;               /* IMGENV_ROLLOUT_* bits, a subset of the rollout's; 0: all of them */
    int32_t state_bytes[IMGENV_SEQ_MAX_STATES];  /* the row of caller array a: a multiple of 4, at most 65536; 0: none */
    int32_t reserved;             /* 0 */
} imgenv_seq_cfg;
typedef struct imgenv_seq_buffer {
    /* [L][Bs][row]; NULL where not selected */
    uint16_t* mb_sensor_maps;
    float* mb_vector_states;
    double* mb_lasers;
    float* mb_ped_vector_states;
    float* mb_ped_maps;
    float* mb_ped_vector_norm;
    uint16_t* mb_stack_sensor_maps;
    float* mb_stack_vector_states;
    double* mb_stack_lasers;
    float* mb_norm_vector_states;  /* IMGENV_ROLLOUT_NORM_STATES: here, not in imgenv_normalise_out */
    float* mb_norm_state_stack;
    float* mb_actions;
    float* mb_rewards;
    uint8_t* mb_dones;
    int32_t* mb_dones_info;
    int32_t* mb_index;
    float* mb_weight;
    uint8_t* mb_first;
    float* mb_scalars;
    int32_t* mb_seq;
    int32_t* mb_seq_len;
    uint8_t* mb_seq_state[IMGENV_SEQ_MAX_STATES];
} imgenv_seq_buffer;
typedef struct imgenv_seq_out {
    int32_t struct_size;          /* on entry 0 or sizeof(imgenv_seq_out) */
    int32_t n_local;              /* R */
    int32_t horizon;              /* T */
    int32_t length;               /* L */
    int32_t batch;                /* Bs */
    int32_t buffers;
    int32_t fields;               /* the bits in effect */
    int32_t max_sequences;        /* C_max R */
    int32_t state_bytes[IMGENV_SEQ_MAX_STATES];
    uint8_t* seq_flag;
    int32_t* seq_valid;
    int32_t* seq_order;
    uint32_t* seq_valid_n;
    int32_t* tile_count;
    int32_t* tile_base;
    imgenv_seq_buffer buf[IMGENV_MB_MAX_BUFFERS];  /* buf[b] all NULL for b >= buffers */
} imgenv_seq_out;
/* Legal once imgenv_rollout_enable() has been called (IMGENV_ESTATE before).  IMGENV_EINVAL for a wrong struct_size, length outside
 * 1 .. T, batch < 1, buffers outside 1 .. 4, unknown bits, a bit the rollout does not store, a state_bytes that is negative, no
 * multiple of 4 or above 65536, C_max R >= 2^31, or a second call whose cfg differs from the first's (same cfg: `out` is filled
 * again, nothing changes).  IMGENV_ENOMEM when the arrays cannot be allocated; the handle is then unchanged.  `out` may be NULL.
 * Nothing is launched, and no chain of the handle changes. */
int imgenv_rollout_seq_enable(imgenv_t* h, const imgenv_seq_cfg* cfg, imgenv_seq_out* out);
/* IMGENV_ESTATE before imgenv_rollout_seq_enable() */
int imgenv_rollout_seq_outputs(imgenv_t* h, imgenv_seq_out* out);
/* seq_flag, then seq_valid / seq_valid_n by imgenv_rollout_index's stable compaction over the flags: four launches, no workgroup
 * waits for another.  Records the generation.  IMGENV_ESTATE before imgenv_rollout_seq_enable(), before imgenv_rollout_begin() or
 * with n == 0. */
int imgenv_rollout_seq_index(imgenv_t* h, void* stream);
/* seq_order[p] = seq_valid[pi(p)] for p < seq_valid_n (read on the device), -1 for seq_valid_n <= p < C_max R; one launch; pi and
 * its keys are imgenv_rollout_shuffle's, over Vs.  IMGENV_ESTATE for a stale or missing index. */
int imgenv_rollout_seq_shuffle(imgenv_t* h, uint32_t seed_lo, uint32_t seed_hi, void* stream);
typedef struct imgenv_seq_args {
    int32_t struct_size;          /* sizeof(imgenv_seq_args) */
    int32_t j;                    /* minibatch number >= 0: the slots take seq_order[j Bs .. j Bs + Bs - 1] */
    int32_t buffer;               /* 0 .. buffers - 1 */
    int32_t n_scalars;            /* 0 .. IMGENV_MB_MAX_SCALARS */
    int32_t normalise;            /* an index into scalars, or -1 */
    int32_t reserved;             /* 0 */
    const float* scalars[IMGENV_MB_MAX_SCALARS];  /* DEVICE f32 arrays indexed by k, row stride R: [T][R] or [T+1][R] */
    const float* norm;            /* DEVICE f32 [2] for `normalise`, the caller's; may be NULL only where normalise is -1 */
    const void* states[IMGENV_SEQ_MAX_STATES];  /* DEVICE [T or T+1][R][state_bytes[a]], 16-byte aligned; unused where state_bytes[a] is 0 */
} imgenv_seq_args;
/* Minibatch j into buffer `buffer`, one launch (k_rollout_seq_gather); under IMGENV_ROLLOUT_PED_MAPS_DRAWN a second one, k_ped_draw
 * with the buffer's own mb_index as its rows.  Slot i < Bs takes q = seq_order[j Bs + i], -1 from C_max R on; step l < L of it is
 * t = c L + l, k = t R + row where q >= 0 and t < n, else k = -1.
 *   k >= 0: mb_<field>[l][i] = obs_<field>[k], the ring's actions / rewards / dones / dones_info of k, mb_index = k, mb_weight =
 *           is_clean[k] != 0, mb_first = final_idx[t][row] >= 0, mb_scalars[s][l][i] = scalars[s][k], for s == normalise
 *           (x - norm[0]) * norm[1] in float32 (two roundings);
 *   k <  0: every byte of the step's rows 0, mb_index = -1, mb_weight, mb_first and every scalar 0.
 * The buffer is fully defined after every gather but for the rows of mb_scalars from n_scalars on.  IMGENV_EINVAL for a wrong
 * struct_size, j < 0, a buffer, n_scalars or normalise out of range, a null scalars[s], a null norm with normalise >= 0, a null or
 * misaligned states[a] where state_bytes[a] > 0; IMGENV_ESTATE for a stale or missing index or before
 * imgenv_rollout_seq_shuffle() on this index. */
int imgenv_rollout_seq_minibatch(imgenv_t* h, const imgenv_seq_args* args, void* stream);

/* ---- map bank: several static maps in one handle, one of them per world and episode ----
 * The reference trains one policy over a set of maps: its trainer is started from several YAML files side by side
 * (create_launch.py:57-65, one node per (env_name, env_num) pair), each env process loads its own global_map.map_file
 * (yaml_env.py:163, 203).  Here the maps form a bank inside ONE handle and every world of it runs its current episode on one of
 * them, so a set of maps still costs one chain of launches per step.  Every world owns its copy of every grid layer and the hot
 * kernels read only that copy; the bank is read by resets alone.
 *
 * imgenv_maps_add: legal once per handle, after imgenv_create() and before its first reset (IMGENV_ESTATE otherwise, also on a
 * second call).  `maps` is HOST memory [n][Hg][Wg] in the same pixels as the map handed to imgenv_create(); Hg x Wg must equal
 * that map's size (IMGENV_EINVAL: one grid size per handle -- the world stride, the index divisions and the crop tiling are per
 * handle).  The bank becomes [create's map, maps[0], ..., maps[n-1]]: map 0 is always the map of imgenv_create(), every world
 * starts on map 0, and a handle that never selects another map behaves exactly as one without a bank, launch for launch.  Each
 * added map goes through the same load-time resize as the first (global_resolution != view_resolution) and gets its own image
 * for the tiled big-view kernels where the handle keeps one.  IMGENV_EINVAL on a robot shard (robot_begin / robot_end not the
 * whole world): banks in sharded, multi-GPU handles are out of scope.  IMGENV_ENOMEM when the bank cannot be allocated; the
 * handle is then unchanged. */
int imgenv_maps_add(imgenv_t* h, int32_t n, const uint8_t* maps, int32_t Hg, int32_t Wg);
/* World worlds[q] starts from map map_ids[q] at its NEXT reset of any kind queued on `stream` after this call (imgenv_reset,
 * imgenv_reset_world(s), imgenv_reset_worlds_spawn, the resets inside imgenv_step_autoreset / imgenv_step_autoreset_device);
 * until then its current episode is untouched.  The choice stays until it is replaced (by this call, or by a draw under
 * IMGENV_MAPS_BY_PLACEMENT).  Host arrays, copied during the call.  An out-of-range map id, an out-of-range world or a world listed
 * twice: IMGENV_EINVAL, and nothing is applied.  One small launch; no synchronisation. */
int imgenv_world_maps_set(imgenv_t* h, int32_t n, const int32_t* worlds, const int32_t* map_ids, void* stream);
/* Who chooses the map of a new episode.  IMGENV_MAPS_KEEP (the default): imgenv_world_maps_set alone.  IMGENV_MAPS_BY_PLACEMENT:
 * every reset that draws its placement from a 64-bit seed draws the map with it, map = imgenv_map_for_placement(seed, n_maps) --
 * on the host for imgenv_reset_worlds_spawn (seeds[q]) and imgenv_step_autoreset (seed0 + k), and INSIDE the device-side reset
 * chain for imgenv_step_autoreset_device (seed0 + placement number: k_respawn computes it where the placement number is known and
 * the map restore of the same chain reads it from device memory): no host read-back, no synchronisation, no additional launch --
 * the map curriculum without the host in the loop.  Such a draw also becomes the world's choice for later resets; resets from
 * explicit batches (imgenv_reset, imgenv_reset_world(s)) never draw and keep the world's choice.  May be called at any time; takes
 * effect with the next call that resets.  On a handle with one map it is accepted and changes nothing. */
#define IMGENV_MAPS_KEEP 0
#define IMGENV_MAPS_BY_PLACEMENT 1
int imgenv_maps_policy(imgenv_t* h, int32_t policy);
/* The draw itself: a pure function, needs no device, exported so that checkers and trainers can reproduce it.  An integer mix of
 * the seed (splitmix64's finaliser) reduced to [0, n_maps) by multiply-shift of its upper 32 bits: no modulo bias beyond 2^-32, no
 * floating point -- one definition (csrc/map_bank.h) compiled for host and device, which agree bit for bit.  n_maps <= 1 gives 0. */
int32_t imgenv_map_for_placement(uint64_t seed, int32_t n_maps);
/* map_ids[n_worlds]: the map each world's CURRENT episode runs on (all 0 without a bank).  Synchronises `stream`, like
 * imgenv_autoreset_last(). */
int imgenv_world_maps(imgenv_t* h, int32_t* map_ids, void* stream);

/* ---- track bank: recorded crowds in one handle, one set of tracks per world and episode ----
 * The dataset pedestrian scene (IMGENV_SCENE_DATASET; img_env.cpp:294-296, 361-386) replays recorded ETH / UCY tracks that the
 * reference's PedTrajectoryDatasetWrapper (PedTrajectoryDatasetWrapper.py:15-291) hands to every reset.  A recorded crowd is the
 * same kind of object as a static map: a small set of immutable arrays an episode starts from.  Here the sets form a bank inside
 * the handle; a reset that brings no tracks of its own takes the world's set from it, on the device, so dataset worlds can be
 * reset by imgenv_reset_worlds_spawn, imgenv_step_autoreset and imgenv_step_autoreset_device like every other scene.  The step
 * kernels read the per-world tables they always read: a reset COPIES the chosen set into the world's rows (k_tracks_install,
 * Pw * cap * 48 bytes per world reset: 24 KB for 10 pedestrians of 50 records); nothing is added to a step.
 *
 * imgenv_tracks_add: legal once per handle, after imgenv_create() and before its first reset (IMGENV_ESTATE otherwise, also on a
 * second call).  All arrays are HOST memory with the fields and meaning of imgenv_reset_batch for ONE world, repeated per set:
 * ped_pose [n_sets][Pw][4] (x, y, qz, qw), ped_traj [n_sets][Pw][cap][3], ped_traj_v [n_sets][Pw][cap][2], ped_traj_len
 * [n_sets][Pw], each in [1, cap]; Pw = n_peds / n_worlds.  Each set is converted once into what a reset stages for such a batch
 * (img_env.cpp:220-250: the yaw of the quaternion, atan2(vy, vx) of the host's libm beside the velocities, records behind a
 * pedestrian's length zero), so a bank-fed reset leaves the state an explicit batch of the same tracks leaves, bit for bit.
 * The handle's trajectory tables are allocated here with max(cap, 2) records per pedestrian; a later explicit batch with a longer
 * ped_traj_cap still re-lays them out, the bank keeps its own stride.  IMGENV_EINVAL: the scene is not IMGENV_SCENE_DATASET, the
 * handle has no pedestrians or is a robot shard, n_sets < 1 or cap < 1, a length outside [1, cap], a value that is not finite.
 * IMGENV_ENOMEM when the bank cannot be allocated, IMGENV_EDEVICE when filling it fails; the handle is then unchanged. */
int imgenv_tracks_add(imgenv_t* h, int32_t n_sets, int32_t cap, const double* ped_pose, const double* ped_traj,
                      const double* ped_traj_v, const int32_t* ped_traj_len);
/* World worlds[q] takes set set_ids[q] at its NEXT bank-fed reset queued on `stream` after this call (under
 * IMGENV_TRACKS_KEEP; the other policies replace the choice); its running episode is untouched.  Host arrays, copied during the
 * call.  An out-of-range set id, an out-of-range world, a world listed twice: IMGENV_EINVAL, and nothing is applied;
 * IMGENV_ESTATE on a handle without a bank.  One small launch; no synchronisation. */
int imgenv_world_tracks_set(imgenv_t* h, int32_t n, const int32_t* worlds, const int32_t* set_ids, void* stream);
/* Which resets are bank-fed, and who chooses their set.
 * A reset batch that carries ped_traj_v behaves as on a handle without a bank: it never consults the bank, does not advance the
 * CYCLE count, and imgenv_world_tracks reports -1 for its world.  On a handle WITH a bank a batch without ped_traj_v is
 * bank-fed -- what imgenv_reset_worlds_spawn / imgenv_step_autoreset build, an explicit batch with ped_traj_v == NULL -- and
 * the batch's own ped_pose / ped_traj / ped_traj_len are ignored (they may be NULL); without a bank it stays IMGENV_EINVAL.
 * imgenv_step_autoreset_device accepts a dataset handle once it has a bank.  The sampler still places the YAML's n_peds
 * pedestrians and the result is discarded, as EnvPos.reset does before init_ped_dataset overwrites them
 * (reset_helper.py:417-432): the robots' placements and the placement numbering do not depend on the bank, and
 * imgenv_world_placement keeps reporting the SAMPLER's pedestrian poses -- the recorded ones are identified by imgenv_world_tracks.
 *   IMGENV_TRACKS_KEEP (the default): the set of imgenv_world_tracks_set (set 0 until then).
 *   IMGENV_TRACKS_BY_PLACEMENT: set = imgenv_tracks_for_placement(seed, n_sets) with the placement's seed -- seeds[q] for
 *     imgenv_reset_worlds_spawn, seed0 + k for imgenv_step_autoreset, seed0 + placement number inside the device-side chain.
 *     A bank-fed reset without a seed (an explicit batch) keeps the world's choice.
 *   IMGENV_TRACKS_CYCLE: the reference wrapper's own order: a world's e-th bank-fed reset since this call (e = 0, 1, ...) takes
 *     set (e / repeat) % n_sets -- PedTrajectoryDatasetWrapper.reset with repeated_time_per_env = repeat and cur_world.
 *     DEVIATION: after the last set the reference calls sys.exit(); this wraps to set 0.
 * Every resolved set also becomes the world's choice for KEEP.  repeat < 1 or an unknown policy: IMGENV_EINVAL; IMGENV_ESTATE
 * without a bank.  Takes effect with the next call that resets; it zeroes the per-world counts, for which it waits for the
 * device (not a call for the hot loop). */
#define IMGENV_TRACKS_KEEP 0
#define IMGENV_TRACKS_BY_PLACEMENT 1
#define IMGENV_TRACKS_CYCLE 2
int imgenv_tracks_policy(imgenv_t* h, int32_t policy, int32_t repeat);
/* The draw under IMGENV_TRACKS_BY_PLACEMENT: imgenv_map_for_placement(seed + 0xBB67AE8584CAA73B, n_sets), the sum modulo 2^64 --
 * the salt (the fractional bits of sqrt 3) keeps a handle with both banks from tying map m to set m.  A pure function, one
 * definition (csrc/track_bank.h) compiled for host and device.  n_sets <= 1 gives 0. */
int32_t imgenv_tracks_for_placement(uint64_t seed, int32_t n_sets);
/* set_ids[n_worlds]: the set each world's CURRENT episode replays, -1 where its last reset brought its own tracks (every world
 * before its first reset, and all of them without a bank).  Synchronises `stream`, like imgenv_world_maps(). */
int imgenv_world_tracks(imgenv_t* h, int32_t* set_ids, void* stream);

/* ---- scenario bank: recorded episodes in one handle, replayed by the device-side reset ----
 * The reference has two sources for an episode's placement (envs/env/yaml_env.py:223-244): `cfg_type: yaml` draws a fresh one
 * (EnvPos.reset; here imgenv_spawn and the device-side sampler), `cfg_type: bag` replays the recorded ResetEnv requests of a file
 * written by save_envs_bag, the k-th reset taking request reset_index % len(reset_reqs) -- how a fixed test set is run: the same
 * N episodes for every policy and checkpoint.  Here the recorded episodes form a bank inside the handle.  The device-side reset
 * never samples where it hands a placement out: it copies placement number n out of a pool slot filled ahead from that number
 * alone, and with a policy other than OFF the fill copies a scenario of the bank instead of sampling (k_scenario_fill,
 * csrc/scenario_bank.h) and derives the same data from it (obstacle instances, RVO polygons + BSP, pedscene segments).  Every
 * kernel behind the pool is what it was.
 *
 * imgenv_scenarios_add: legal once per handle, before the first imgenv_step_autoreset_device (IMGENV_ESTATE on a second call).
 * n episodes in imgenv_spawn()'s array layout with a leading [n] axis, HOST memory, copied during the call; Rw = n_robots /
 * n_worlds, Pw = n_peds / n_worlds, O = n_obstacles:
 *   robot_pose [n][Rw][4], robot_goal [n][Rw][2], ped_pose [n][Pw][4], ped_goal [n][Pw][2], ped_traj [n][Pw][2][3],
 *   ped_traj_len [n][Pw], obs_shape [n][O], obs_size [n][O][4], obs_pose [n][O][4]
 * (pedestrian arrays may be NULL with Pw == 0, obstacle arrays with O == 0).  IMGENV_EINVAL with a message that names the scenario:
 * a value that is not finite, a zero quaternion, a ped_traj_len outside 0..2, a shape that is neither circle nor rectangle, an
 * empty or oversized obstacle footprint, Rw + Pw > 256 or O > 24 (the device-side reset's limits), n < 1, a robot shard, and -- on
 * handles with RVO agents -- a scenario whose obstacle polygons and their BSP do not fit a pool slot.
 * Limits: a trajectory of at most 2 points per pedestrian (what a slot holds and what EnvPos produces); one cast per bank;
 * a scenario carries no map id -- with a map bank the caller keeps the worlds on the map the episodes were recorded on
 * (IMGENV_MAPS_KEEP); a dataset handle's recorded crowds still come from the track bank, over the scenario's pedestrians. */
int imgenv_scenarios_add(imgenv_t* h, int32_t n, int32_t n_obstacles, const double* robot_pose, const double* robot_goal,
                         const double* ped_pose, const double* ped_goal, const double* ped_traj, const int32_t* ped_traj_len,
                         const int32_t* obs_shape, const float* obs_size, const double* obs_pose);
/* What fills the pool of imgenv_step_autoreset_device from now on.
 *   IMGENV_SCENARIOS_OFF (the default): the sampler, exactly as on a handle without a bank.
 *   IMGENV_SCENARIOS_QUEUE: placement number k (the k-th world the device resets, counted over the whole handle) replays
 *     scenario (first + k) % n -- the reference's reset_index % len(reset_reqs), shared by the handle's worlds: one pass of n
 *     resets runs every scenario once.
 *   IMGENV_SCENARIOS_BY_PLACEMENT: a draw from the placement's seed, imgenv_scenario_for_placement.
 * May be called between any two calls: the pool's slots, drawn under the old policy, are invalidated on `stream` and the next
 * imgenv_step_autoreset_device refills them before it hands any out -- the first reset behind the call obeys the new policy.
 * No host synchronisation.  imgenv_step_autoreset_device then refuses (IMGENV_EINVAL) a spawn cfg whose n_robots / n_peds /
 * n_obstacles differ from the bank's; the cfg is still needed for the counts and the fingerprint, nothing else about the call
 * changes.  imgenv_step_autoreset, the HOST-side auto-reset, keeps sampling and ignores the bank.
 * IMGENV_ESTATE without a bank (also for OFF), IMGENV_EINVAL for an unknown policy. */
#define IMGENV_SCENARIOS_OFF 0
#define IMGENV_SCENARIOS_QUEUE 1
#define IMGENV_SCENARIOS_BY_PLACEMENT 2
int imgenv_scenarios_policy(imgenv_t* h, int32_t policy, uint64_t first, void* stream);
/* The scenario placement number n takes: QUEUE (first + n) % n_scenarios, the sum modulo 2^64; BY_PLACEMENT
 * imgenv_map_for_placement(seed0 + n + 0x3C6EF372FE94F82B, n_scenarios) -- the salt (the fractional bits of sqrt 5) is distinct
 * from the track bank's, so the three banks' draws of one seed are not tied.  -1 under OFF or with n_scenarios < 1.  A pure
 * function, needs no device; one definition (csrc/scenario_bank.h) compiled for host and device. */
int32_t imgenv_scenario_for_placement(int32_t policy, uint64_t seed0, uint64_t first, uint64_t n, int32_t n_scenarios);
/* imgenv_reset_worlds() with the bank's episode ids[q] for world worlds[q]: the first reset, and callers that choose by hand.
 * Host code only -- the batches are built from the bank's host copy and go through imgenv_reset_worlds (ped_traj_v is NULL, so a
 * dataset handle with a track bank takes its crowd from that bank); the device's placement count does not advance.  A
 * pedestrian recorded with ped_traj_len 0 is refused here as any reset batch refuses it.  IMGENV_EINVAL for an id out of range,
 * IMGENV_ESTATE without a bank. */
int imgenv_reset_worlds_scenarios(imgenv_t* h, int32_t n, const int32_t* worlds, const int32_t* ids, void* stream);
/* ids[n_worlds]: the scenario each world's CURRENT episode came from, -1 where its reset did not come from the bank (the sampler,
 * an explicit batch, a host spawn; every world before its first reset, all of them without a bank).  Synchronises `stream`.  After
 * the pool has been rebuilt for another spawn cfg the worlds report -1 until their next reset. */
int imgenv_world_scenarios(imgenv_t* h, int32_t* ids, void* stream);

/* The two OpenCV resizes of the path for one-channel 8-bit images, as the library performs them (OpenCV 4.2.0's generic
 * fixed-point CPU path restated, csrc/cv_resize.h): host buffers, no device needed.  kind 0: INTER_LINEAR, 1: INTER_CUBIC. */
int imgenv_cv_resize_u8(int kind, const uint8_t* src, int32_t sh, int32_t sw, uint8_t* dst, int32_t dh, int32_t dw);

/* number of kernels launched by the last step (bench / profiling aid) */
int imgenv_step_launches(imgenv_t* h);
/* how the handle keeps its class layer and schedules its steps (what imgenv_create decided; tests and probes assert on it):
 * bits 0-1: 0 composed owner layers + k_compose, 1 stamps, 2 counts (SUM); bit 2: robot shard in SUM mode (bitmaps in the
 * records, k_remote); bit 3: early-observation steps; bit 4: the social-force crowd a step ahead */
int imgenv_layer_mode(imgenv_t* h);

/* Live per-kernel timing with HIP events recorded on the stream the kernels are launched on.
 * mode 0: off; 1: every launch of every kernel; 2: every 8th launch of kernel `which` only (sampling keeps the
 * event barriers out of most steps).  Kernel ids (K_PED_UPDATE is part of the K_INTEGRATE launch): */
#define IMGENV_K_ORCA 0
#define IMGENV_K_PED_UPDATE 1
#define IMGENV_K_INTEGRATE 2
#define IMGENV_K_RASTER 3
#define IMGENV_K_COMPOSE 4
#define IMGENV_K_VIEW 5
#define IMGENV_K_OBS 6
#define IMGENV_K_TAIL 7
#define IMGENV_K_CROP 8      /* big views (csrc/view_big.h): k_crop_big; IMGENV_K_VIEW is then k_beams_big */
#define IMGENV_K_FULLVIEW 9  /* k_fullview_big */
#define IMGENV_K_TAPS 10     /* k_taps_big */
#define IMGENV_K_MOVE_RASTER 11 /* k_move_raster: K_INTEGRATE + K_RASTER as one launch (small / pedestrian-free handles) */
#define IMGENV_K_EXCHANGE 12    /* the in-library ncclAllGather of the robot records (imgenv_comm_init), between K_INTEGRATE and K_RASTER */
#define IMGENV_K_REMOTE 13      /* k_remote: a robot shard takes the other ranks' robots from their records, behind the exchange */
#define IMGENV_K_COUNT 14
int imgenv_timing(imgenv_t* h, int mode, int which);
/* synchronises the recorded events and returns accumulated milliseconds / launch counts per kernel
 * id since the last imgenv_timing() call; arrays of IMGENV_K_COUNT entries */
int imgenv_timing_read(imgenv_t* h, double* total_ms, int64_t* launches);
const char* imgenv_kernel_name(int id);

#ifdef __cplusplus
}
#endif
#endif /* IMGENV_H_ */
