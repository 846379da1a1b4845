// tail_rows.h -- which robot rows a launch of the chain tail (k_stack, k_episodes, k_obs_post) covers, for the kernels and, as
// plain C++, for tests/host/tail_rows_check.cpp.
//
// A step covers every local robot: rows 0 .. RL-1.  A reset chain covers the robots of the worlds it lists, in list order, Rw
// rows each; the length of the list is the host's (n_worlds) or, behind a device-side reset, a kernel's count (*n_dev, which then
// wins).  A reset chain without a list (imgenv_reset) covers every local robot like a step.
//
// Invariant: a listed chain runs on a whole handle only -- r0 == 0 and RL == n_worlds x Rw -- so world w's robot i is local row
// w * Rw + i and no listed row can lie outside the handle.  The host code keeps it:
//   imgenv_create refuses n_worlds > 1 together with a robot shard;
//   imgenv_reset_worlds (and through it imgenv_reset_world, imgenv_reset_worlds_spawn, imgenv_step_autoreset) forwards a handle of
//     one world to imgenv_reset, which has no list, and range-checks every entry of a longer handle's list;
//   imgenv_step_autoreset_device, whose list k_finished_dev writes (entries < n_worlds), refuses a handle that does not hold all
//     robots of every world -- this is the one listed chain a handle of ONE world can run, and that handle is whole as well.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TAIL_HD __host__ __device__ __forceinline__
#else
#define TAIL_HD inline
#endif

struct TailRows {
    int32_t RL, Rw;    // local robots, robots per world
    const int* list;   // the worlds of a reset chain (nullptr = every local robot) ...
    const int* n_dev;  // ... and their count in device memory (nullptr = n_worlds)
    int32_t n_worlds;
};

// `listed` is the caller's compile-time-known `RESTART && rows.list != nullptr`: a step's instantiation pays nothing for the list
TAIL_HD size_t tail_rows_count(const TailRows& r, bool listed) {
    return listed ? (size_t)(r.n_dev ? *r.n_dev : r.n_worlds) * (size_t)r.Rw : (size_t)r.RL;
}
// the local row of the m-th covered robot, m < tail_rows_count
TAIL_HD size_t tail_rows_row(const TailRows& r, bool listed, size_t m) {
    if (!listed) return m;
    const size_t q = m / (size_t)r.Rw;
    return (size_t)r.list[q] * (size_t)r.Rw + (m - q * (size_t)r.Rw);
}
