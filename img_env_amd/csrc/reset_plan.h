// reset_plan.h -- what a host-side reset decides and computes before it touches a device: the refusals of its batches, what each
// world's batch uploads (obstacle instances, RVO polygons with their BSP, social-force segments, pedestrian, trajectory, waypoint
// and robot rows), how far the handle's tables grow, and the sizes and refusals of the device-side reset's placement pool.  Host
// code, nothing of HIP: plain C++17, compiled by g++ for tests/host/reset_plan_check.cpp.  imgenv_hip.hip prepares, refuses, then
// commits: nothing here writes the handle, the row fills write into the memory the caller gives them (the
// page-locked blocks the reset kernel reads).
//
// A refusal returns its IMGENV_E* code and leaves its text in `msg`; the caller hands both on (imgenv_last_error).
#pragma once
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/imgenv.h"
#include "host_tables.h"  // RvoObstacles, get_corners
#include "sfm.h"          // SFM_MAX_WP
#include "spawn_slot.h"   // SPAWN_MAX_AGENTS, SPAWN_MAX_OBST, SPAWN_BSP_CAP, SPAWN_FILL_PERIOD
#include "tfm.h"

typedef char ResetMsg[512];
#define RESET_REFUSE(code, ...) return snprintf(msg, sizeof(ResetMsg), __VA_ARGS__), (code)

// ---------------------------------------------------------------------------------------- what the reset kernels read
// one copy of k_reset_apply's segment table: page-locked host bytes -> device
struct StageSeg {
    unsigned char* dst;
    const unsigned char* src;
    size_t bytes;
};
// One obstacle for k_reset_obstacles.  Its footprint samples (agent.cpp:18-30, 51-62: a 0.01 m lattice, for circles the points
// within the radius) are generated on the fly from the lattice bounds computed here: random obstacle radii (EnvPos draws a fresh
// one per episode, reset_helper.py:131-133) then cost nothing -- no per-size sample list to upload, cache or free.
struct ObstInst {
    double x, y, sh, ch;  // pose; sin / cos of yaw/2, evaluated on the host
    double cx, cy, r;     // circle: centre offset and radius (sizes[0..2]); rectangle: unused
    int m0, m1, n0, n1;   // lattice range: circle -bb..bb with bb = ceil(r / 0.01); rectangle floor(min / 0.01)..ceil(max / 0.01)
    int shape, world;
};
struct ResetRobot {  // per local robot
    double gx, gy;
    Tf2 world_target;
};

// ---------------------------------------------------------------------------------------- what the path reads of the handle
struct ResetFacts {
    int W = 1, Rw = 0, Pw = 0, r0 = 0, RL = 0, NA = 0;
    int scene = 0;                // IMGENV_SCENE_*
    bool track_bank = false;      // imgenv_tracks_add has been called: a dataset batch without ped_traj_v is fed from the bank
    bool dev_reset_used = false;  // the device-side reset has taken over the per-world RVO tables
    int cap_obst = 0, cap_nodes = 0;  // RVO vertices / BSP nodes a world's slice has room for
    int sfm_cap_obs = 0;          // pedscene: segments a crowd has room for
    int traj_cap = 0;             // points per pedestrian in the trajectory table
    int sfm_n = 0;                // agents of one pedscene crowd (0: none)
    bool sfm_per_world = false;   // the per-world crowd tables exist (W > 1)
    bool has_traj = false;        // the trajectory table exists
};
inline bool reset_bank_fed(const ResetFacts& f, const imgenv_reset_batch& b) { return f.track_bank && f.scene == IMGENV_SCENE_DATASET && !b.ped_traj_v; }

// ---------------------------------------------------------------------------------------- prepare: one world from its batch
// init_shape_circle / init_shape_rectangle (agent.cpp:18-30, 51-62) and the pose as k_reset_obstacles takes it
inline ObstInst obstacle_instance(int shape, const double* sizes, const double* pose, int world) {
    const double yaw = tf_yaw_from_quaternion_zw(pose[2], pose[3]);
    ObstInst oi;
    oi.x = pose[0]; oi.y = pose[1]; oi.sh = sin(yaw * 0.5); oi.ch = cos(yaw * 0.5);
    oi.world = world;
    oi.shape = shape;
    oi.cx = sizes[0]; oi.cy = sizes[1]; oi.r = sizes[2];
    if (shape == IMGENV_SHAPE_CIRCLE) {
        const int bb = (int)ceil(sizes[2] / 0.01);
        oi.m0 = oi.n0 = -bb;
        oi.m1 = oi.n1 = bb;
    } else {
        oi.m0 = (int)floor(sizes[0] / 0.01); oi.m1 = (int)ceil(sizes[1] / 0.01);
        oi.n0 = (int)floor(sizes[2] / 0.01); oi.n1 = (int)ceil(sizes[3] / 0.01);
    }
    return oi;
}
inline bool obstacle_footprint_ok(const ObstInst& oi) {
    return !((long long)(oi.m1 - oi.m0 + 1) * (long long)(oi.n1 - oi.n0 + 1) > (1ll << 26) || oi.m1 < oi.m0 || oi.n1 < oi.n0);
}
// Agent::get_corners (agent.cpp:626-651) of an obstacle at (x, y) with sin / cos of yaw/2: the segment pa -> pb PedScene::addObs
// takes (pedscene.h:22-26) and the four vertices RVOScene::addObs takes (rvoscene.h:19-26)
inline void obstacle_polygon(int shape, const double* sizes, double x, double y, double sh, double ch, double seg[4], float v[8]) {
    const Tf2 bw = tf_from_pose_sc(x, y, sh, ch);
    get_corners(shape, sizes, bw, seg[0], seg[1], seg[2], seg[3]);
    const float pax = (float)seg[0], pay = (float)seg[1], pbx = (float)seg[2], pby = (float)seg[3];
    v[0] = pax; v[1] = pay; v[2] = pax; v[3] = pby; v[4] = pbx; v[5] = pby; v[6] = pbx; v[7] = pay;
}

struct ResetWorld {  // what one world's batch brings, as far as refusals and growth need it (the rows go straight into page-locked memory)
    int world = 0;
    std::vector<ObstInst> inst;   // for k_reset_obstacles
    RvoObstacles rvo;             // RVOScene::addObs + processObs (img_env.cpp:283)
    std::vector<double> sfm_obs;  // [n][4] pedscene segments
    bool fed = false;             // its pedestrians come from the track bank (k_tracks_install)
    int traj_need = 0;            // points per pedestrian its trajectory rows need (0: it brings none)
};
inline void reset_prepare_world(const ResetFacts& f, int world, const imgenv_reset_batch& b, ResetWorld& w) {
    w.world = world;
    w.inst.clear();
    w.rvo.clear();
    w.sfm_obs.clear();
    for (int q = 0; q < b.n_obstacles; q++) {
        double sizes[4];
        for (int j = 0; j < 4; j++) sizes[j] = (double)b.obs_size[4 * q + j];
        const double* p = b.obs_pose + 4 * q;
        const ObstInst oi = obstacle_instance(b.obs_shape[q], sizes, p, world);
        w.inst.push_back(oi);
        double seg[4];
        float v[8];
        obstacle_polygon(oi.shape, sizes, p[0], p[1], oi.sh, oi.ch, seg, v);
        if (!b.ignore_obstacle && f.scene == IMGENV_SCENE_PEDSIM) w.sfm_obs.insert(w.sfm_obs.end(), seg, seg + 4);
        if (!b.ignore_obstacle && f.NA > 0) w.rvo.add(v, 4);
    }
    w.rvo.process();
    w.fed = f.Pw > 0 && reset_bank_fed(f, b);
    w.traj_need = f.Pw > 0 && !w.fed ? b.ped_traj_cap : 0;
}

// pedestrians (img_env.cpp:220-250): pose rows for reset_ped, trajectory lengths, and the trajectory rows re-strided from the
// batch's ped_traj_cap to the table's `stride`, zero-padded.  A bank-fed world: zeros that the install replaces, nothing else.
inline void reset_ped_rows(int Pw, const imgenv_reset_batch& b, bool fed, int stride, double* ped3, int* tlen, double* traj) {
    if (fed) {
        memset(ped3, 0, sizeof(double) * 3 * (size_t)Pw);
        return;
    }
    memset(traj, 0, sizeof(double) * 3 * (size_t)Pw * stride);
    for (int j = 0; j < Pw; j++) {
        const double* p = b.ped_pose + 4 * j;
        ped3[3 * j] = p[0];
        ped3[3 * j + 1] = p[1];
        ped3[3 * j + 2] = tf_yaw_from_quaternion_zw(p[2], p[3]);
        tlen[j] = b.ped_traj_len[j];
        for (int q = 0; q < tlen[j]; q++) memcpy(&traj[((size_t)j * stride + q) * 3], b.ped_traj + ((size_t)j * b.ped_traj_cap + q) * 3, 24);
    }
}
// trajectory_v (img_env.cpp:246-247) + the yaw _step_ped_dataset derives from it, with the host's libm
inline void reset_traj_v_rows(int Pw, const imgenv_reset_batch& b, int stride, double* tv) {
    memset(tv, 0, sizeof(double) * 3 * (size_t)Pw * stride);
    for (int j = 0; j < Pw; j++)
        for (int q = 0; q < b.ped_traj_len[j]; q++) {
            const double* v = b.ped_traj_v + ((size_t)j * b.ped_traj_cap + q) * 2;
            double* o = &tv[((size_t)j * stride + q) * 3];
            o[0] = v[0];
            o[1] = v[1];
            o[2] = atan2(v[1], v[0]);
        }
}
// PedScene::setWayPoint (pedscene.h:38-46): [goal r=1, trajectory r=z] per pedestrian, cut at SFM_MAX_WP; the deque holds them in
// order and addWaypoint leaves destination = waypoints.front() without popping it (ped_agent.cpp:97-100)
struct WaypointRows {
    double *wx, *wy, *wr;  // [Pw][SFM_MAX_WP]
    int* dq;               // [Pw][SFM_MAX_WP]
    int *dq_n, *dest, *last;  // [Pw]
};
inline void reset_waypoint_rows(int Pw, const imgenv_reset_batch& b, const WaypointRows& o) {
    const size_t n = (size_t)Pw * SFM_MAX_WP;
    memset(o.wx, 0, n * 8); memset(o.wy, 0, n * 8); memset(o.wr, 0, n * 8); memset(o.dq, 0, n * 4);
    for (int j = 0; j < Pw; j++) {
        const size_t at = (size_t)j * SFM_MAX_WP;
        o.wx[at] = b.ped_goal[2 * j];
        o.wy[at] = b.ped_goal[2 * j + 1];
        o.wr[at] = 1.0;
        int nw = 1;
        for (int q = 0; q < b.ped_traj_len[j] && nw < SFM_MAX_WP; q++, nw++) {
            const double* tp = b.ped_traj + ((size_t)j * b.ped_traj_cap + q) * 3;
            o.wx[at + nw] = tp[0];
            o.wy[at + nw] = tp[1];
            o.wr[at + nw] = tp[2];
        }
        for (int q = 0; q < nw; q++) o.dq[at + q] = q;
        o.dq_n[j] = nw;
        o.dest[j] = 0;
        o.last[j] = -1;
    }
}
// robots (img_env.cpp:252-282): init_pose rows (x, y, yaw, sin / cos of yaw/2) for every robot of the world, set_goal
// (agent.cpp:144-154) for those of the shard [r0, r0 + RL).  rr: the world's first local robot (a shard exists for W == 1 only).
inline void reset_robot_rows(const ResetFacts& f, int world, const imgenv_reset_batch& b, double* rob3, ResetRobot* rr) {
    const int g_lo = world * f.Rw, l_lo = f.W > 1 ? g_lo : 0;
    for (int i = 0; i < f.Rw; i++) {
        const double* p = b.robot_pose + 4 * i;
        const double yaw = tf_yaw_from_quaternion_zw(p[2], p[3]);
        rob3[5 * i] = p[0];
        rob3[5 * i + 1] = p[1];
        rob3[5 * i + 2] = yaw;
        rob3[5 * i + 3] = sin(yaw * 0.5);
        rob3[5 * i + 4] = cos(yaw * 0.5);
        const int l = g_lo + i - f.r0;
        if (l >= 0 && l < f.RL) {
            ResetRobot& q = rr[l - l_lo];
            q.gx = b.robot_goal[2 * i];
            q.gy = b.robot_goal[2 * i + 1];
            q.world_target = tf_inverse(tf_from_pose(q.gx, q.gy, yaw));
        }
    }
}

// ---------------------------------------------------------------------------------------- refuse
// Everything that can be wrong with a reset is found by these two, BEFORE the call touches the handle's state or the device: a
// reset that fails part-way would leave host and device copies of the earlier worlds out of step.  The first reads the batches
// as given (prepare dereferences their arrays), the second what prepare made of them.
inline int reset_check_batches(const ResetFacts& f, int n, const imgenv_reset_batch* b, int peds_per_batch, ResetMsg& msg) {
    if (!b) RESET_REFUSE(IMGENV_EINVAL, "null argument");
    for (int q = 0; q < n; q++) {
        if (b[q].struct_size != (int32_t)sizeof(imgenv_reset_batch)) RESET_REFUSE(IMGENV_EINVAL, "reset batch ABI mismatch");
        // (bank-fed: a dataset handle with a track bank takes the pedestrians of a batch without ped_traj_v from the bank, and the
        // batch's own pedestrian arrays are ignored)
        const bool fed = reset_bank_fed(f, b[q]);
        if (b[q].n_obstacles < 0 || (f.Pw > 0 && !fed && b[q].ped_traj_cap < 1)) RESET_REFUSE(IMGENV_EINVAL, "bad reset batch");
        if (b[q].n_obstacles > 0 && (!b[q].obs_shape || !b[q].obs_size || !b[q].obs_pose)) RESET_REFUSE(IMGENV_EINVAL, "reset batch %d: null obstacle arrays", q);
        if (!b[q].robot_pose || !b[q].robot_goal) RESET_REFUSE(IMGENV_EINVAL, "reset batch %d: null robot arrays", q);
        for (int o = 0; o < b[q].n_obstacles; o++)
            if (b[q].obs_shape[o] != IMGENV_SHAPE_CIRCLE && b[q].obs_shape[o] != IMGENV_SHAPE_RECTANGLE)
                RESET_REFUSE(IMGENV_EINVAL, "reset batch %d, obstacle %d: unsupported shape %d", q, o, b[q].obs_shape[o]);
        if (peds_per_batch > 0 && !fed) {
            if (!b[q].ped_pose || !b[q].ped_traj_len || !b[q].ped_traj) RESET_REFUSE(IMGENV_EINVAL, "reset batch %d: null pedestrian arrays", q);
            if (f.scene == IMGENV_SCENE_DATASET && !b[q].ped_traj_v)
                RESET_REFUSE(IMGENV_EINVAL, "dataset scene: ped_traj_v is missing from the reset batch");
            if (f.scene == IMGENV_SCENE_PEDSIM && !b[q].ped_goal) RESET_REFUSE(IMGENV_EINVAL, "pedscene: ped_goal is missing from the reset batch");
            for (int j = 0; j < peds_per_batch; j++)
                if (b[q].ped_traj_len[j] < 1 || b[q].ped_traj_len[j] > b[q].ped_traj_cap)
                    RESET_REFUSE(IMGENV_EINVAL, "reset batch %d, ped %d: bad trajectory length %d", q, j, b[q].ped_traj_len[j]);
        }
    }
    return IMGENV_OK;
}
inline int reset_check_worlds(const ResetFacts& f, const ResetWorld* w, int n, ResetMsg& msg) {
    for (int q = 0; q < n; q++) {
        for (size_t o = 0; o < w[q].inst.size(); o++)
            if (!obstacle_footprint_ok(w[q].inst[o])) RESET_REFUSE(IMGENV_EINVAL, "obstacle %d: degenerate or oversized footprint", (int)o);
        if (f.dev_reset_used && ((int)w[q].rvo.ob.size() > f.cap_obst || (int)w[q].rvo.nodes.size() > f.cap_nodes))
            RESET_REFUSE(IMGENV_ESTATE, "world %d: more RVO obstacle vertices than the handle has room for, after imgenv_step_autoreset_device has taken over "
                                        "the per-world obstacle tables (reset every world with imgenv_reset first)", w[q].world);
        if (f.scene == IMGENV_SCENE_PEDSIM && f.W > 1 && (int)w[q].sfm_obs.size() / 4 > f.sfm_cap_obs)
            RESET_REFUSE(IMGENV_EINVAL, "world %d: more than %d obstacles in a pedscene world of a multi-world handle", w[q].world, f.sfm_cap_obs);
    }
    return IMGENV_OK;
}

// ---------------------------------------------------------------------------------------- commit: growth, once per call
// The capacities after this reset, from the largest need of its worlds: twice the need for the RVO slices and the segment array
// of a single-world handle, exactly the longest ped_traj_cap for the trajectory table.  A capacity that stays is returned as it is.
struct ResetGrowth {
    int cap_obst = 0, cap_nodes = 0, traj_cap = 0, sfm_cap_obs = 0;
    bool rvo_moved = false;  // a slice stride changed: both tables are allocated anew and every world's slice is staged again
    bool traj_moved = false;
    bool sfm_moved = false;
};
inline ResetGrowth reset_growth(const ResetFacts& f, const ResetWorld* w, int n) {
    int need_obst = 0, need_nodes = 0, need_traj = 0, need_seg = 0;
    for (int q = 0; q < n; q++) {
        need_obst = std::max(need_obst, (int)w[q].rvo.ob.size());
        need_nodes = std::max(need_nodes, (int)w[q].rvo.nodes.size());
        need_traj = std::max(need_traj, w[q].traj_need);
        need_seg = std::max(need_seg, (int)w[q].sfm_obs.size() / 4);
    }
    ResetGrowth g;
    g.cap_obst = need_obst > f.cap_obst ? need_obst * 2 : f.cap_obst;
    g.cap_nodes = need_nodes > f.cap_nodes ? need_nodes * 2 : f.cap_nodes;
    g.rvo_moved = g.cap_obst != f.cap_obst || g.cap_nodes != f.cap_nodes;
    g.traj_cap = std::max(need_traj, f.traj_cap);
    g.traj_moved = g.traj_cap != f.traj_cap;
    const bool one_crowd = f.scene == IMGENV_SCENE_PEDSIM && f.W == 1;  // (several worlds: fixed slices, reset_check_worlds)
    g.sfm_cap_obs = one_crowd && need_seg > f.sfm_cap_obs ? need_seg * 2 : f.sfm_cap_obs;
    g.sfm_moved = g.sfm_cap_obs != f.sfm_cap_obs;
    return g;
}
// The worlds whose RVO slices this reset stages, each exactly once: the listed ones (null: all), or every world where the slices moved
inline std::vector<int> reset_rvo_worlds(int W, const ResetGrowth& g, const int* list, int n) {
    std::vector<int> r;
    if (!list || g.rvo_moved) {
        for (int k = 0; k < W; k++) r.push_back(k);
    } else {
        r.assign(list, list + n);
    }
    return r;
}
// world q's column of the [4][W] per-world RVO table: obstacle base, node base, #obstacles, root
inline void rvo_table_put(std::vector<int>& wobst, int W, int q, int cap_obst, int cap_nodes, const RvoObstacles& r) {
    wobst[q] = q * cap_obst;
    wobst[(size_t)W + q] = q * cap_nodes;
    wobst[2 * (size_t)W + q] = (int)r.ob.size();
    wobst[3 * (size_t)W + q] = r.root;
}

// ---------------------------------------------------------------------------------------- the device-side reset's pool
// slots: every world can need a placement in a single step; see SPAWN_FILL_PERIOD
inline int spawn_pool_slots(int W) { return (SPAWN_FILL_PERIOD + 2) * std::max(64, W); }
// RVO obstacle vertices / BSP nodes a pool slot has room for, whatever the handle's own tables hold (the set-up only ever raises
// it to the handle's capacity)
inline int spawn_slot_cap(int nob) { return std::max(16, std::min(SPAWN_BSP_CAP, 16 * std::max(nob, 1))); }
inline int spawn_pool_check(const ResetFacts& f, const imgenv_spawn_cfg& cfg, ResetMsg& msg) {
    const int na = cfg.n_robots + cfg.n_peds, nob = cfg.n_obstacles;
    if (na > SPAWN_MAX_AGENTS || nob > SPAWN_MAX_OBST)
        RESET_REFUSE(IMGENV_EINVAL, "device-side auto-reset places at most %d agents and %d obstacles per world", SPAWN_MAX_AGENTS, SPAWN_MAX_OBST);
    if (f.scene == IMGENV_SCENE_DATASET && !f.track_bank)  // (with a track bank the chain's k_tracks_install brings them)
        RESET_REFUSE(IMGENV_EINVAL, "device-side auto-reset: dataset scenes (recorded crowds come with the reset call) are reset by the host (imgenv_step_autoreset)");
    const bool sfm = f.scene == IMGENV_SCENE_PEDSIM && f.sfm_n > 0;
    if (sfm && (f.W < 2 || !f.sfm_per_world))
        RESET_REFUSE(IMGENV_EINVAL, "device-side auto-reset of a pedscene world needs a handle of several worlds (n_worlds > 1: the per-world crowd tables)");
    if (sfm && !cfg.ignore_obstacle && nob > f.sfm_cap_obs)
        RESET_REFUSE(IMGENV_EINVAL, "device-side auto-reset: %d obstacles, a pedscene world of this handle has room for %d", nob, f.sfm_cap_obs);
    if (f.Pw > 0 && (f.traj_cap < 2 || !f.has_traj)) RESET_REFUSE(IMGENV_ESTATE, "device-side auto-reset: reset every world once first (trajectories of two points)");
    for (int a = 0; a < na; a++) {
        const imgenv_spawn_agent& g = cfg.agents[a];
        if (g.begin_type == IMGENV_POSE_RANGE_MULTI && (g.n_begin_multi < 1 || !g.begin_multi)) RESET_REFUSE(IMGENV_EINVAL, "range_multi start without ranges");
        if (g.target_type == IMGENV_POSE_RANGE_MULTI && (g.n_target_multi < 1 || !g.target_multi)) RESET_REFUSE(IMGENV_EINVAL, "range_multi target without ranges");
    }
    return IMGENV_OK;
}
