// obs_post.h -- the two small output wrappers of the reference that the fused tail does not cover, for every robot of a handle:
//   StatePedVectorWrapper (envs/wrapper/base.py:19-34)   ped_vector_norm: the robot's ped_vector row with the 7 values of each of
//                                                         its first n = min(int(row[0]), max_ped) pedestrians shifted and scaled,
//                                                         float32((double(x) - avg[c]) / std[c]) -- numpy's float32 slice minus
//                                                         and divided by float64 constants, stored back into the float32 row;
//                                                         row[0] and the padding behind the n pedestrians are copied
//   InfoLogWrapper's bool_get_close_to_human (base.py:250-252)   close_to_human = ped_min_dists < close_dist (the reference's 1)
// The results go to arrays of their own: imgenv_out.ped_vector_states stays the raw vector that k_obs and the output guards own.
//
// One kernel, two instantiations, launched at the end of every chain (launch_views) behind k_stack / k_episodes and in front of
// the seal, on the caller's stream:
//   <false> (a step)          every local robot
//   <true>  (a reset chain)   the robots of the worlds the chain covers (tail_rows.h: k_stack<true>'s cases)
// One lane per element of a row (1 + 7 max_ped of them; one per robot where only close_to_human is kept): neighbouring lanes read
// and write neighbouring floats, row[0] is one broadcast read per row.  The lane of element 0 also writes close_to_human.
// Only - /, conversions and compares, without contraction: IEEE-exact, tests/action_model.py gives the same bits.
// Bytes per robot and chain: 4 (1 + 7 max_ped) read and written, + 8 read and 1 written for close_to_human.
#pragma once
#include <stdint.h>

#include "launch_plan.h"  // OBS_POST_BLOCK, OBS_POST_MAX_BLOCKS
#include "tail_rows.h"

#define OBS_POST_DIM 7  // values per pedestrian (imgenv_cfg.ped_vec_dim of every shipped YAML; the wrapper's avg / std have 7)

struct ObsPostDev {
    const float* ped_vector_states;  // [RL][PV]  imgenv_out's, in the working arena
    const double* ped_min_dists;     // [RL]
    float* norm;                     // [RL][PV]  (PED_NORM)
    uint8_t* close;                  // [RL]      (CLOSE)
    double avg[OBS_POST_DIM], std[OBS_POST_DIM], close_dist;
    int32_t flags, PV, max_ped, per_row;  // per_row: PV with PED_NORM, else 1
    TailRows rows;                   // the robots of this launch (<true>: those of the reset chain's worlds)
};

// a[c] for a kernel argument: selects on scalar registers, no indexed copy of the struct
__device__ __forceinline__ double obs_post_at(const double (&a)[OBS_POST_DIM], int c) {
    double x = a[0];
#pragma unroll
    for (int k = 1; k < OBS_POST_DIM; k++) x = c == k ? a[k] : x;
    return x;
}

template <bool RESTART>
__global__ __launch_bounds__(OBS_POST_BLOCK) void k_obs_post(const ObsPostDev p) {
    const bool listed = RESTART && p.rows.list != nullptr;
    const size_t per_row = (size_t)p.per_row, total = tail_rows_count(p.rows, listed) * per_row, stride = (size_t)gridDim.x * OBS_POST_BLOCK;
    for (size_t t = (size_t)blockIdx.x * OBS_POST_BLOCK + threadIdx.x; t < total; t += stride) {
        const size_t m = t / per_row;
        const int e = (int)(t - m * per_row);
        const size_t row = tail_rows_row(p.rows, listed, m);
        if (e == 0 && (p.flags & IMGENV_OBS_CLOSE)) p.close[row] = p.ped_min_dists[row] < p.close_dist ? 1 : 0;
        if (!(p.flags & IMGENV_OBS_PED_NORM)) continue;
        const float* src = p.ped_vector_states + row * (size_t)p.PV;
        float x = src[e];
        if (e > 0) {
            const float count = src[0];
            // int(row[0]), at most max_ped (a count that is not a number normalises nothing)
            const int n = count >= 1.0f ? (count < (float)p.max_ped ? (int)count : p.max_ped) : 0;
            const int j = (e - 1) / OBS_POST_DIM, c = (e - 1) - j * OBS_POST_DIM;
            if (j < n) x = (float)(((double)x - obs_post_at(p.avg, c)) / obs_post_at(p.std, c));
        }
        p.norm[row * (size_t)p.PV + e] = x;
    }
}
