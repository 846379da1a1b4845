// scenario_bank.h -- recorded episodes in one handle (include/imgenv.h: imgenv_scenarios_add): the reference's `cfg_type: bag`
// (envs/env/yaml_env.py:223-244), where the k-th reset replays the k-th recorded ResetEnv request instead of drawing a fresh one.
//
// The device-side reset (csrc/spawn_device.h) never samples inside k_respawn: it copies placement number n out of pool slot
// n % S, and a slot is filled ahead, on a side stream, from the placement's number alone.  A recorded episode list is a second
// way to fill a slot: k_scenario_fill copies scenario scenario_for_placement(n) of the bank into the slot and then derives what
// the sampler's fill derives (sp_slot_finish: obstacle instances, pedscene segments, RVO polygons + BSP).  Everything behind the
// pool -- k_finished_dev, k_respawn, k_tracks_install, the map restore, the obstacle raster, the views -- is untouched.
//
// The host half (scenarios_convert, scenario_to_arrays) is plain C++: tests/host/scenario_bank_check.cpp runs it under the
// sanitizers without a device.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <cmath>

#include "../../include/imgenv.h"
#include "map_bank.h"
#include "spawn_slot.h"

// The 64-bit salt of IMGENV_SCENARIOS_BY_PLACEMENT: the fractional bits of sqrt(5) (0.2360679...).  The scenario of a placement is
// map_for_placement over seed + salt: a handle with a map bank, a track bank and a scenario bank ties none of the three draws
// to another (the map bank draws from the seed itself, the track bank adds the bits of sqrt(3)).
#define SCENARIO_PLACEMENT_SALT 0x3C6EF372FE94F82Bull

// The scenario placement number n takes.  QUEUE: the reference's reset_index % len(reset_reqs), `first` being the queue's
// position at placement 0 (the sum wraps modulo 2^64 before the remainder, on the host as on the device).  BY_PLACEMENT: a draw
// from the placement's seed.  -1 under IMGENV_SCENARIOS_OFF or without scenarios.  Integers only; one definition for the host
// (imgenv_scenario_for_placement, imgenv_world_scenarios) and the device (k_scenario_fill).
MAP_BANK_HD static inline int32_t scenario_for_placement(int32_t policy, uint64_t seed0, uint64_t first, uint64_t n, int32_t n_scenarios) {
    if (n_scenarios < 1) return -1;
    if (policy == IMGENV_SCENARIOS_QUEUE) return (int32_t)((first + n) % (uint64_t)(uint32_t)n_scenarios);
    if (policy == IMGENV_SCENARIOS_BY_PLACEMENT) return map_for_placement(seed0 + n + SCENARIO_PLACEMENT_SALT, n_scenarios);
    return -1;
}

// ---------------------------------------------------------------------------------------- host: arrays <-> slot records
#define SCENARIO_BAD_FINITE 1      // a value that is not finite
#define SCENARIO_BAD_QUATERNION 2  // qz = qw = 0
#define SCENARIO_BAD_TRAJ_LEN 3    // ped_traj_len outside 0..2
#define SCENARIO_BAD_SHAPE 4       // an obstacle that is neither a circle nor a rectangle
#define SCENARIO_BAD_FOOTPRINT 5   // an obstacle whose footprint lattice is empty or beyond 2^26 samples (obstacle_footprint_ok's bound)

static inline const char* scenario_error_text(int code) {
    switch (code) {
        case SCENARIO_BAD_FINITE: return "a value that is not finite";
        case SCENARIO_BAD_QUATERNION: return "a zero quaternion";
        case SCENARIO_BAD_TRAJ_LEN: return "a trajectory length outside 0..2";
        case SCENARIO_BAD_SHAPE: return "an unsupported obstacle shape";
        case SCENARIO_BAD_FOOTPRINT: return "a degenerate or oversized obstacle footprint";
    }
    return "?";
}

static inline bool scenario_finite(const double* p, int n) {
    for (int q = 0; q < n; q++)
        if (!std::isfinite(p[q])) return false;
    return true;
}

// n recorded episodes in imgenv_spawn()'s array layout with a leading [n] axis -> SlotAgent [n][Rw + Pw] (robots first) and
// SlotObstacle [n][O], what k_spawn_fill leaves in a slot for such a placement: a robot's record carries its goal as a
// one-point trajectory like the sampler's, a pedestrian's records behind its length are zero, the padding words are zero.
// Returns 0, or SCENARIO_BAD_* with the scenario in *where and the agent (robots first) or obstacle in *which; nothing is read
// behind a bad value.  With n_peds == 0 / O == 0 the pedestrian / obstacle arrays are not touched (they may be null).
static inline int scenarios_convert(int n, int Rw, int Pw, int O, const double* robot_pose, const double* robot_goal, const double* ped_pose,
                                    const double* ped_goal, const double* ped_traj, const int32_t* ped_traj_len, const int32_t* obs_shape,
                                    const float* obs_size, const double* obs_pose, SlotAgent* agents, SlotObstacle* obst, int* where, int* which) {
    const int na = Rw + Pw;
    for (int s = 0; s < n; s++) {
        *where = s;
        for (int a = 0; a < na; a++) {
            *which = a;
            const bool robot = a < Rw;
            const size_t at = robot ? (size_t)s * Rw + a : (size_t)s * Pw + (a - Rw);
            const double* p = (robot ? robot_pose : ped_pose) + 4 * at;
            const double* g = (robot ? robot_goal : ped_goal) + 2 * at;
            if (!scenario_finite(p, 4) || !scenario_finite(g, 2)) return SCENARIO_BAD_FINITE;
            if (p[2] == 0.0 && p[3] == 0.0) return SCENARIO_BAD_QUATERNION;
            SlotAgent& o = agents[(size_t)s * na + a];
            memset(&o, 0, sizeof(o));
            o.x = p[0]; o.y = p[1]; o.qz = p[2]; o.qw = p[3];
            o.gx = g[0]; o.gy = g[1];
            if (robot) {
                o.traj[0][0] = g[0];
                o.traj[0][1] = g[1];
                o.traj_len = 1;
                continue;
            }
            const int len = ped_traj_len[at];
            if (len < 0 || len > 2) return SCENARIO_BAD_TRAJ_LEN;
            if (!scenario_finite(ped_traj + 6 * at, 3 * len)) return SCENARIO_BAD_FINITE;
            memcpy(o.traj, ped_traj + 6 * at, sizeof(double) * 3 * (size_t)len);
            o.traj_len = len;
        }
        for (int q = 0; q < O; q++) {
            *which = q;
            const size_t at = (size_t)s * O + q;
            const double* p = obs_pose + 4 * at;
            const float* z = obs_size + 4 * at;
            if (!scenario_finite(p, 4)) return SCENARIO_BAD_FINITE;
            for (int j = 0; j < 4; j++)
                if (!std::isfinite(z[j])) return SCENARIO_BAD_FINITE;
            if (p[2] == 0.0 && p[3] == 0.0) return SCENARIO_BAD_QUATERNION;
            const int shape = obs_shape[at];
            if (shape != IMGENV_SHAPE_CIRCLE && shape != IMGENV_SHAPE_RECTANGLE) return SCENARIO_BAD_SHAPE;
            // the footprint lattice of init_shape_circle / init_shape_rectangle (agent.cpp:18-62), bounded as a host reset bounds it
            double m0, m1, n0, n1;
            if (shape == IMGENV_SHAPE_CIRCLE) {
                m1 = n1 = ceil((double)z[2] / 0.01);
                m0 = n0 = -m1;
            } else {
                m0 = floor((double)z[0] / 0.01); m1 = ceil((double)z[1] / 0.01);
                n0 = floor((double)z[2] / 0.01); n1 = ceil((double)z[3] / 0.01);
            }
            if (m1 < m0 || n1 < n0 || (m1 - m0 + 1.0) * (n1 - n0 + 1.0) > 67108864.0) return SCENARIO_BAD_FOOTPRINT;
            SlotObstacle& o = obst[at];
            memset(&o, 0, sizeof(o));
            o.x = p[0]; o.y = p[1]; o.qz = p[2]; o.qw = p[3];
            for (int j = 0; j < 4; j++) o.size[j] = z[j];
            o.shape = shape;
        }
    }
    return 0;
}

// One scenario's records back into the arrays of imgenv_spawn() / imgenv_reset_batch (ped_traj_cap 2): the host resets
// (imgenv_reset_worlds_scenarios) build their batches from the bank's host copy with it.
static inline void scenario_to_arrays(int Rw, int Pw, int O, const SlotAgent* agents, const SlotObstacle* obst, double* robot_pose, double* robot_goal,
                                      double* ped_pose, double* ped_goal, double* ped_traj, int32_t* ped_traj_len, int32_t* obs_shape, float* obs_size,
                                      double* obs_pose) {
    for (int a = 0; a < Rw + Pw; a++) {
        const SlotAgent& o = agents[a];
        const int j = a < Rw ? a : a - Rw;
        double* p = (a < Rw ? robot_pose : ped_pose) + 4 * (size_t)j;
        double* g = (a < Rw ? robot_goal : ped_goal) + 2 * (size_t)j;
        p[0] = o.x; p[1] = o.y; p[2] = o.qz; p[3] = o.qw;
        g[0] = o.gx; g[1] = o.gy;
        if (a >= Rw) {
            memcpy(ped_traj + 6 * (size_t)j, o.traj, sizeof(o.traj));
            ped_traj_len[j] = o.traj_len;
        }
    }
    for (int q = 0; q < O; q++) {
        const SlotObstacle& o = obst[q];
        obs_shape[q] = o.shape;
        memcpy(obs_size + 4 * (size_t)q, o.size, sizeof(o.size));
        double* p = obs_pose + 4 * (size_t)q;
        p[0] = o.x; p[1] = o.y; p[2] = o.qz; p[3] = o.qw;
    }
}

// ---------------------------------------------------------------------------------------- device
// The bank as the fill receives it, by value and on its own: SpawnDev, which every kernel of the chain takes, does not grow
// (docs/HISTORY.md section 4: what a struct the compiler can no longer keep in scalar registers costs).
struct ScenarioSel {
    const SlotAgent* agents;    // [n][n_robots + n_peds]
    const SlotObstacle* obst;   // [n][n_obstacles]
    int n, policy;              // IMGENV_SCENARIOS_*
    unsigned long long first;   // QUEUE: the queue's position at placement 0
};

#if defined(__HIPCC__)
// One pool slot from the bank.  k_spawn_fill's launch shape (one wave64 workgroup per slot, grid S, on the fill's side stream:
// nothing for csrc/launch_plan.h to decide) and its slot / serial arithmetic; instead of dev_spawn_world the lanes copy the
// scenario of placement n into the slot, 64 records at a time -- the cast is rarely a multiple of 64, and there may be no obstacle
// at all.  The derivation reads the obstacles from the bank (every lane the same words), not from the slot just written.
__global__ __launch_bounds__(WAVE) void k_scenario_fill(SpawnDev c, ScenarioSel b) {
    __shared__ SpawnScratch L;
    const int s = blockIdx.x;
    const unsigned long long done = c.consumed[1];
    const unsigned long long S = (unsigned long long)c.S;
    unsigned long long n = done - done % S + (unsigned long long)s;
    if (n < done) n += S;
    if (c.slot_serial[s] == n) return;
    const int id = scenario_for_placement(b.policy, c.seed0, b.first, n, b.n);  // (uniform: scalar registers)
    const int na = c.n_robots + c.n_peds, nob = c.n_obstacles;
    const SlotAgent* __restrict__ src_a = b.agents + (size_t)(id < 0 ? 0 : id) * na;
    const SlotObstacle* __restrict__ src_o = b.obst + (size_t)(id < 0 ? 0 : id) * nob;
    SlotAgent* ag = c.s_agents + (size_t)s * na;
    SlotObstacle* ob = c.s_obst + (size_t)s * (nob > 0 ? nob : 1);
    for (int q = lane_id(); q < na; q += WAVE) ag[q] = src_a[q];
    for (int q = lane_id(); q < nob; q += WAVE) ob[q] = src_o[q];
    L.status = id >= 0 ? 0 : 17;  // (a launch without a policy: the host never makes one)
    sp_slot_finish(c, L, s, n, src_o);
}

// The [W] words imgenv_world_scenarios reads for worlds the HOST reset last: scn[world] = the scenario of the reset (-1: not from
// the bank) and mark[world] = the placement number the world held at that moment -- a later device-side reset gives the world a
// new number, so "mark == place_serial" says that the host's reset is still the world's latest.  list == nullptr: every world.
__global__ void k_scenario_mark(int* __restrict__ scn, unsigned long long* __restrict__ mark, const unsigned long long* __restrict__ place_serial,
                                const int* __restrict__ list, const int* __restrict__ ids, int n) {
    const int q = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (q >= n) return;
    const int world = list ? list[q] : q;
    scn[world] = ids ? ids[q] : -1;
    mark[world] = place_serial ? place_serial[world] : ~0ull;
}
#endif
