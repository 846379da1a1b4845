// track_bank.h -- recorded crowds in one handle (include/imgenv.h: imgenv_tracks_add): the bank of pedestrian track sets a
// dataset world's episode starts from, which of them each world's current episode replays (cur), which its next bank-fed reset
// takes (next) and how many bank-fed resets it has had (count, for IMGENV_TRACKS_CYCLE).
//
// A set is what ONE world's reset batch carries for a dataset scene (ped_pose, ped_traj, ped_traj_v, ped_traj_len), converted ONCE
// on the host into exactly what stage_world (imgenv_hip.hip) stages for such a batch: the start pose with the yaw of the
// quaternion, the positions, the velocities with atan2(vy, vx) of the host's libm as third column, records behind a
// pedestrian's length zero.  k_tracks_install copies a set into the world's rows of the per-handle tables, so a bank-fed reset
// leaves the device state an explicit batch of the same tracks leaves, bit for bit, and every step kernel reads what it read.
//
// All three [W] arrays live in device memory: the device-side reset chain (csrc/spawn_device.h) resolves a world's set inside
// k_tracks_install, behind k_respawn -- the host never knows it.  A handle without a bank launches nothing of this.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "map_bank.h"
#include "tfm.h"

// The 64-bit salt of imgenv_tracks_for_placement: the fractional bits of sqrt(3) (0.7320508...).  The track set of a placement
// is map_for_placement over seed + salt, so a handle with both banks does not tie map m to set m.
#define TRACKS_PLACEMENT_SALT 0xBB67AE8584CAA73Bull

MAP_BANK_HD static inline int32_t tracks_for_placement(uint64_t seed, int32_t n_sets) {
    return map_for_placement(seed + TRACKS_PLACEMENT_SALT, n_sets);
}

// The e-th bank-fed reset of a world under IMGENV_TRACKS_CYCLE: PedTrajectoryDatasetWrapper's order (cur_world moves on after
// repeated_time_per_env episodes, PedTrajectoryDatasetWrapper.py:225-291) -- wrapping where the reference exits.
MAP_BANK_HD static inline int32_t tracks_for_cycle(uint32_t e, int32_t repeat, int32_t n_sets) {
    return (int32_t)((e / (uint32_t)repeat) % (uint32_t)n_sets);
}

// ---------------------------------------------------------------------------------------- host: one set -> what a reset stages
// `stride` records per pedestrian in the outputs (>= cap): pose3 [Pw][3] = (x, y, yaw), traj and traj_v [Pw][stride][3], len [Pw].
// Returns 0, or 1 + the first pedestrian with a bad length, or -(1 + pedestrian) for a value that is not finite.  Plain C++:
// tests/host/track_bank_check.cpp runs it under the sanitizers without a device.
static inline int tracks_convert_set(int Pw, int cap, int stride, const double* ped_pose, const double* ped_traj, const double* ped_traj_v,
                                     const int32_t* ped_traj_len, double* pose3, double* traj, double* traj_v, int32_t* len) {
    for (size_t e = 0; e < (size_t)Pw * stride * 3; e++) traj[e] = traj_v[e] = 0.0;
    for (int j = 0; j < Pw; j++) {
        const int n = ped_traj_len[j];
        if (n < 1 || n > cap) return 1 + j;
        const double* p = ped_pose + 4 * (size_t)j;
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]) || !std::isfinite(p[3])) return -(1 + j);
        pose3[3 * j] = p[0];
        pose3[3 * j + 1] = p[1];
        pose3[3 * j + 2] = tf_yaw_from_quaternion_zw(p[2], p[3]);
        if (!std::isfinite(pose3[3 * j + 2])) return -(1 + j);  // (a zero quaternion)
        len[j] = n;
        for (int q = 0; q < n; q++) {
            const double* tp = ped_traj + ((size_t)j * cap + q) * 3;
            const double* tv = ped_traj_v + ((size_t)j * cap + q) * 2;
            if (!std::isfinite(tp[0]) || !std::isfinite(tp[1]) || !std::isfinite(tp[2]) || !std::isfinite(tv[0]) || !std::isfinite(tv[1])) return -(1 + j);
            double* o = traj + ((size_t)j * stride + q) * 3;
            double* v = traj_v + ((size_t)j * stride + q) * 3;
            o[0] = tp[0];
            o[1] = tp[1];
            o[2] = tp[2];
            v[0] = tv[0];
            v[1] = tv[1];
            v[2] = atan2(tv[1], tv[0]);  // the yaw _step_ped_dataset derives from the velocity, with the host's libm
        }
    }
    return 0;
}

// ---------------------------------------------------------------------------------------- device
struct TrackSel {
    // the bank: [n_sets] blocks of Pw * cap * 3 doubles (8-byte words: a world's rows of the handle's tables start at
    // world * Pw * stride * 24 bytes, which is only 8-byte aligned for odd Pw * stride -- nothing here assumes more)
    const double* traj;
    const double* traj_v;
    const double* pose3;  // [n_sets][Pw][3]
    const int* len;       // [n_sets][Pw]
    int* cur;             // [W] set of each world's current episode, -1: its last reset brought its own tracks
    int* next;            // [W] set each world's next bank-fed reset takes under IMGENV_TRACKS_KEEP
    uint32_t* count;      // [W] bank-fed resets since imgenv_tracks_policy
    int n_sets, cap;      // cap: records per pedestrian in the bank (the handle's stride when the bank was made)
    int policy, repeat;   // IMGENV_TRACKS_*
};

#if defined(__HIPCC__)
// The worlds of a reset chain take their recorded crowds.  One workgroup per listed world, striding over the list:
//   host chains: `list` / `ids` in page-locked memory, n of them; ids[q] >= 0 is the host's draw for the placement's seed
//   the device chain: list = fin_list, *n_dev of them (the grid is sized for a guess), serial / consumed from k_respawn
// Per world: the set is resolved by every lane from the same words (uniform loads), a barrier, then lane 0 stores cur / next /
// count; the set's traj and traj_v blocks go into the world's rows as 8-byte words; one lane per pedestrian writes what
// reset_ped writes for a dataset world (imgenv_hip.hip: pose, ptraj_idx, the RVO agent's position, ped_state[0..1]; velocities,
// last pose and the leg gait persist across resets, as in Agent::init_pose).  The yaw is the host's, not cr_atan2's.
__global__ __launch_bounds__(256) void k_tracks_install(DevWorld w, TrackSel t, const int* __restrict__ list, const int* __restrict__ n_dev, int n_host,
                                                        const int* __restrict__ ids, const unsigned long long* __restrict__ serial,
                                                        const unsigned long long* __restrict__ consumed, unsigned long long seed0,
                                                        double* __restrict__ d_traj, double* __restrict__ d_traj_v, int* __restrict__ d_len, int stride) {
    // (the pointers of DevWorld this kernel stores through, fetched in front of any branch: DESIGN.md section 4)
    double *ppx = w.ppx, *ppy = w.ppy, *pyaw = w.pyaw, *ped_state = w.ped_state;
    const double *pvx = w.pvx, *pvy = w.pvy;
    float *apx = w.apx, *apy = w.apy;
    int* ptraj_idx = w.ptraj_idx;
    const int Pw = w.Pw, NA = w.NA, tid = (int)threadIdx.x;
    const int n = n_dev ? *n_dev : n_host;
    const unsigned long long first = consumed ? consumed[1] : 0ull;
    for (int q = (int)blockIdx.x; q < n; q += (int)gridDim.x) {
        const int world = list[q];
        if (serial && serial[world] != first + (unsigned long long)q) continue;  // k_respawn could not place it: the old episode stays
        int set;
        if (ids && ids[q] >= 0) set = ids[q];
        else if (t.policy == IMGENV_TRACKS_CYCLE) set = tracks_for_cycle(t.count[world], t.repeat, t.n_sets);
        else if (t.policy == IMGENV_TRACKS_BY_PLACEMENT && serial) set = tracks_for_placement(seed0 + serial[world], t.n_sets);
        else set = t.next[world];
        const uint32_t count = t.count[world];
        __syncthreads();  // every lane has read the world's words before lane 0 replaces them
        if (tid == 0) {
            t.cur[world] = set;
            t.next[world] = set;
            t.count[world] = count + 1u;
        }
        const size_t row = (size_t)t.cap * 3, words = (size_t)Pw * row;
        const double* __restrict__ st = t.traj + (size_t)set * words;
        const double* __restrict__ sv = t.traj_v + (size_t)set * words;
        for (size_t e = (size_t)tid; e < words; e += blockDim.x) {
            const size_t j = e / row, r = e - j * row;
            const size_t at = ((size_t)world * Pw + j) * (size_t)stride * 3 + r;
            d_traj[at] = st[e];
            d_traj_v[at] = sv[e];
        }
        for (int a = tid; a < Pw; a += (int)blockDim.x) {
            const int j = world * Pw + a;
            const double* p = t.pose3 + ((size_t)set * Pw + a) * 3;
            const double x = p[0], y = p[1];
            d_len[j] = t.len[(size_t)set * Pw + a];
            ptraj_idx[j] = 0;
            ppx[j] = x;
            ppy[j] = y;
            pyaw[j] = p[2];
            if (NA > 0) {
                apx[j] = (float)x;
                apy[j] = (float)y;
            }
            ped_state[4 * j] = x;
            ped_state[4 * j + 1] = y;
            ped_state[4 * j + 2] = pvx[j];
            ped_state[4 * j + 3] = pvy[j];
        }
    }
}
#endif
