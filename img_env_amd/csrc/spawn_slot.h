// spawn_slot.h -- what one pool slot of the device-side reset (csrc/spawn_device.h) holds of a placement, and the limits of one
// world's cast.  Plain C++: the host half of the scenario bank (csrc/scenario_bank.h) writes the same records.
#pragma once

#define SPAWN_MAX_AGENTS 256  // robots + pedestrians of one world (the distance tests take them 64 at a time)
#define SPAWN_MAX_OBST 24     // obstacles of one world
#define SPAWN_BSP_CAP 256     // RVO obstacle vertices of one world, splits included
#define SPAWN_FILL_PERIOD 2   // the pool is refilled on every second call; it holds 4 W placements: a refill sees the count of
                              // two steps ago at worst, and up to W worlds can finish on each of the steps until the next one

struct SlotAgent {  // a robot or a pedestrian as ResetEnv.srv carries it
    double x, y, qz, qw, gx, gy;
    double traj[2][3];
    int traj_len, pad;
};
struct SlotObstacle {
    double x, y, qz, qw;
    float size[4];
    int shape, pad;
};
