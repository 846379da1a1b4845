// normalise.h -- running normalisation of the observation vector and of the reward on the device (imgenv_normalise_enable):
// Stable-Baselines3's VecNormalize / RunningMeanStd for the rows of a multi-env handle.  Only the library knows which rows count
// -- frozen robots (is_clean == 0) count for nothing, a device-side reset restarts rows without telling the host -- and the arrays
// of imgenv_out are the kernels' working copies, so the normalised rows go to arrays of their own.
//
// State, all library-owned, float64 (D = state_dim, R = local robots):
//   stats   [2][4 + 2 D]   obs_count | ret_count | ret_mean | ret_var | obs_mean[D] | obs_var[D]; a launch reads word `turn & 1`
//                          and writes word `(turn + 1) & 1`.  Initial values: counts 1e-4, means 0, variances 1
//   returns [2][R]         the running discounted return of each robot's open episode; a step reads word `ret_turn & 1` and writes
//                          the other, a reset chain only writes zeros into word `ret_turn & 1`
//   part [tiles][cols][2], part_n [tiles]   the partial (mean, M2) of every column, and the rows, of every tile of the batch
// Both turn counters are the host's, passed by value: the word a launch reads is never the word it writes.
//
// Columns: the D elements of vector_states (IMGENV_NORM_OBS), then, on a step chain, the return (IMGENV_NORM_REWARD).  A wavefront
// holds rpw = 64 / cols whole rows, lane l = r * cols + col is column `col` of the wavefront's row r (lanes from rpw * cols on
// idle): neighbouring lanes read neighbouring floats, and a column's lanes are a stride of `cols` apart.
//
// A chain with update on, two launches; the launch boundary is the only synchronisation, no workgroup waits for another:
//   k_norm_part<RESTART>   a workgroup per tile of 4 x rpw x NORM_PER_LANE covered rows (tail_rows.h; striding).  The batch: a
//       step's rows with is_clean != 0, every row a reset chain covers.  Lane (wavefront w, r, col) holds the samples of rows
//       tile + i (4 rpw) + w rpw + r, i = 0 .. NORM_PER_LANE - 1 -- float32 promoted, or returns * gamma + reward -- and adds them
//       in that order; the lanes of a column fold over r by halves (r += r + half, half = the power of two below rpw .. 1:
//       shuffles), the four wavefronts' sums are added 0, 1, 2, 3 (LDS); mean = sum / rows; the squares (x - mean)^2 take the
//       same way: part[tile][col] = (mean, M2), part_n[tile] = rows.
//   k_norm_apply<RESTART>  every lane folds its column's partials, tile 0, 1, 2, ... (Chan's formula; tiles of no rows are
//       skipped), and merges the batch (c, bm, M2) into the running triple:
//           delta = bm - mean; tot = count + c; mean += delta * c / tot; var = (var * count + M2 + delta * delta * count * c / tot) / tot
//       (c == 0: every word is copied bit for bit); workgroup 0 stores the result into the other word.  Then the apply, a lane
//       per (covered row, column), with the new statistics:
//           norm_vector_states[row][d] = (float)clamp((x - mean[d]) / sqrt(var[d] + eps), +-clip_obs), every frame of the raw
//           state stack likewise (zero padding included) into norm_state_stack;
//           a step: norm_rewards[row] = clamp(reward / sqrt(ret_var + eps), +-clip_reward), and the return's lane stores
//           returns' other word: the new return (the old one for a frozen row), 0 where the step's dones is set;
//           a reset chain: column 0's lane zeroes returns[row].
// With update off k_norm_apply runs alone, reads the statistics of word `turn & 1` and writes no statistic and no return.
//
// Algorithmic bytes per covered row and chain, update on: the row's 4 D bytes of vector_states read twice (+ 8 + 8 + 1 for the
// return, + 1 dones), 4 D + 4 K D written (+ 4 K D of the stack read), + 8 + 8 for norm_rewards and returns; the partials are
// 16 cols + 4 bytes per tile, read by every workgroup of the apply (out of L2).
//
// All arithmetic is float64 without contraction in the order written here.  The per-lane functions are host / device functions:
// tests/host/normalise_check.cpp runs them over a simulated grid against tests/normalise_model.py; what crosses lanes -- the fold
// over r and over the wavefronts -- is norm_fold's fixed order, mirrored there lane by lane.
#pragma once
#include <math.h>
#include <stdint.h>

#include "launch_plan.h"  // NORM_*, NORM_STATS_WORDS
#include "rollout.h"      // ROLLOUT_UNROLL
#include "tail_rows.h"

#define NORM_WAVES (NORM_BLOCK / WAVE)

struct NormDev {
    // what a chain has just written (the working arena's imgenv_out rows, imgenv_stack_out's state stack)
    const float* vector_states;  // [RL][D]
    const float* state_stack;    // [RL][K][D] or nullptr
    const double* rewards;       // [RL]  step_rewards
    const uint8_t* is_clean;     // [RL]  step_is_clean
    const uint8_t* dones;        // [RL]  step_dones
    double* stats;               // [2][NORM_STATS_WORDS(D)]
    double* returns;             // [2][RL] or nullptr
    double* part;                // [tiles][cols][2]
    uint32_t* part_n;            // [tiles]
    float* norm_vector_states;   // [RL][D]
    float* norm_state_stack;     // [RL][K][D] or nullptr
    double* norm_rewards;        // [RL]
    double gamma, clip_obs, clip_reward, eps;
    int32_t D, K;
    int32_t n_obs, n_ret, cols;  // the launch's columns: n_obs = D or 0, n_ret = 1 on a step with IMGENV_NORM_REWARD, cols >= 1
    int32_t update;              // training: the statistics and the returns move
    uint32_t turn, ret_turn;
    TailRows rows;
};

struct NormLane {
    int w, r, col;  // wavefront of the workgroup, row of the wavefront, column
};
TAIL_HD NormLane norm_lane(int cols, uint32_t thread) {
    const int l = (int)(thread & (WAVE - 1)), r = l / cols;
    return {(int)(thread / WAVE), r, l - r * cols};
}
// the first half of the fold over a wavefront's rpw rows: the largest power of two below rpw (0: one row, nothing to fold)
TAIL_HD int norm_half0(int rpw) {
    int half = 1;
    while (half * 2 < rpw) half *= 2;
    return rpw > 1 ? half : 0;
}
TAIL_HD const double* norm_stats_cur(const NormDev& n) { return n.stats + (size_t)(n.turn & 1) * NORM_STATS_WORDS(n.D); }
TAIL_HD double* norm_stats_next(const NormDev& n) { return n.stats + (size_t)((n.turn + 1) & 1) * NORM_STATS_WORDS(n.D); }
TAIL_HD size_t norm_tiles(const NormDev& n, size_t covered) { return plan_norm_tiles(covered, n.cols); }

// the return of `row` with this step's reward in it
TAIL_HD double norm_return(const NormDev& n, size_t row) {
    const double g = n.returns[(size_t)(n.ret_turn & 1) * (size_t)n.rows.RL + row] * n.gamma;
    return g + n.rewards[row];
}

// lane `id` of tile `tile`: its samples into x, bit i of the answer = sample i exists
template <bool RESTART>
TAIL_HD uint32_t norm_part_load(const NormDev& n, bool listed, size_t covered, size_t tile, const NormLane& id, double* x) {
    const int rpw = plan_norm_rows_per_wave(n.cols);
    uint32_t have = 0;
    ROLLOUT_UNROLL
    for (int i = 0; i < NORM_PER_LANE; i++) {
        const size_t m = tile * plan_norm_tile_rows(n.cols) + (size_t)i * (size_t)(NORM_WAVES * rpw) + (size_t)(id.w * rpw + id.r);
        double v = 0.0;
        if (id.r < rpw && m < covered) {
            const size_t row = tail_rows_row(n.rows, listed, m);
            if (RESTART || n.is_clean[row] != 0) {
                v = id.col < n.n_obs ? (double)n.vector_states[row * (size_t)n.D + id.col] : norm_return(n, row);
                have |= 1u << i;
            }
        }
        x[i] = v;
    }
    return have;
}
TAIL_HD double norm_lane_sum(const double* x, uint32_t have) {
    double acc = 0.0;
    ROLLOUT_UNROLL
    for (int i = 0; i < NORM_PER_LANE; i++)
        if (have >> i & 1) acc = acc + x[i];
    return acc;
}
TAIL_HD double norm_lane_squares(const double* x, uint32_t have, double mean) {
    double acc = 0.0;
    ROLLOUT_UNROLL
    for (int i = 0; i < NORM_PER_LANE; i++)
        if (have >> i & 1) {
            const double d = x[i] - mean;
            acc = acc + d * d;
        }
    return acc;
}
// the fold of a workgroup's lane values a[thread] for column `col`, as the workgroup does it: in every wavefront
// a[r] += a[r + half] over the rows, half = norm_half0 .. 1, then the wavefronts' row 0 added in order
template <typename T>
TAIL_HD T norm_fold(T* a, int cols, int col) {
    const int rpw = plan_norm_rows_per_wave(cols);
    for (int w = 0; w < NORM_WAVES; w++)
        for (int half = norm_half0(rpw); half > 0; half >>= 1)
            for (int r = 0; r < half && r + half < rpw; r++) a[w * WAVE + r * cols + col] = a[w * WAVE + r * cols + col] + a[w * WAVE + (r + half) * cols + col];
    T t = a[col];
    for (int w = 1; w < NORM_WAVES; w++) t = t + a[w * WAVE + col];
    return t;
}
TAIL_HD double norm_part_mean(double sum, uint32_t c) { return c ? sum / (double)c : 0.0; }
TAIL_HD void norm_part_store(const NormDev& n, size_t tile, int col, uint32_t c, double mean, double m2) {
    double* p = n.part + (tile * (size_t)n.cols + (size_t)col) * 2;
    p[0] = mean;
    p[1] = c ? m2 : 0.0;
    if (col == 0) n.part_n[tile] = c;
}

struct NormTriple {
    double count, mean, var;  // (the batch's: rows, mean, M2)
};
// the batch of column `col`: the tiles' partials merged in order
TAIL_HD NormTriple norm_batch(const NormDev& n, size_t tiles, int col) {
    NormTriple b = {0.0, 0.0, 0.0};
    for (size_t q = 0; q < tiles; q++) {
        const uint32_t cq = n.part_n[q];
        if (cq == 0) continue;
        const double* p = n.part + (q * (size_t)n.cols + (size_t)col) * 2;
        const double cb = (double)cq, mb = p[0], m2b = p[1];
        if (b.count == 0.0) {
            b = {cb, mb, m2b};
            continue;
        }
        const double delta = mb - b.mean, tot = b.count + cb;
        b.mean = b.mean + delta * cb / tot;
        b.var = b.var + m2b + delta * delta * b.count * cb / tot;
        b.count = tot;
    }
    return b;
}
// Chan's merge of the batch into the running triple; an empty batch leaves every bit
TAIL_HD NormTriple norm_merge(const NormTriple& run, const NormTriple& b) {
    if (b.count == 0.0) return run;
    const double delta = b.mean - run.mean, tot = run.count + b.count;
    NormTriple o;
    o.mean = run.mean + delta * b.count / tot;
    o.var = (run.var * run.count + b.var + delta * delta * run.count * b.count / tot) / tot;
    o.count = tot;
    return o;
}
// the running triple of the launch's column `col` in a statistics word
TAIL_HD NormTriple norm_stats_load(const NormDev& n, const double* s, int col) {
    if (col < n.n_obs) return {s[0], s[4 + col], s[4 + n.D + col]};
    return {s[1], s[2], s[3]};
}
// what the lane of column `col` (one per workgroup 0) stores of the new word; the columns the launch does not have are copied
TAIL_HD void norm_stats_store(const NormDev& n, int col, const NormTriple& t) {
    const double* cur = norm_stats_cur(n);
    double* nx = norm_stats_next(n);
    if (col < n.n_obs) {
        if (col == 0) nx[0] = t.count;
        nx[4 + col] = t.mean;
        nx[4 + n.D + col] = t.var;
    } else if (n.n_ret && col == n.n_obs) {
        nx[1] = t.count;
        nx[2] = t.mean;
        nx[3] = t.var;
    }
    if (col == 0) {
        if (!n.n_ret)
            for (int k = 1; k < 4; k++) nx[k] = cur[k];
        if (!n.n_obs) {
            nx[0] = cur[0];
            for (int k = 0; k < 2 * n.D; k++) nx[4 + k] = cur[4 + k];
        }
    }
}
TAIL_HD double norm_clamp(double v, double clip) { return v < -clip ? -clip : (v > clip ? clip : v); }
// column `col` of the m-th covered row, with the column's statistics: mean and den = sqrt(var + eps)
template <bool RESTART>
TAIL_HD void norm_apply_item(const NormDev& n, bool listed, size_t m, int col, double mean, double den) {
    const size_t row = tail_rows_row(n.rows, listed, m), RL = (size_t)n.rows.RL, D = (size_t)n.D;
    if (col < n.n_obs) {
        const double x = (double)n.vector_states[row * D + col];
        n.norm_vector_states[row * D + col] = (float)norm_clamp((x - mean) / den, n.clip_obs);
        if (n.norm_state_stack)
            for (size_t k = 0; k < (size_t)n.K; k++) {
                const double f = (double)n.state_stack[(row * (size_t)n.K + k) * D + col];
                n.norm_state_stack[(row * (size_t)n.K + k) * D + col] = (float)norm_clamp((f - mean) / den, n.clip_obs);
            }
    } else if (!RESTART && n.n_ret && col == n.n_obs) {
        const double reward = n.rewards[row];
        n.norm_rewards[row] = norm_clamp(reward / den, n.clip_reward);
        if (n.update) {
            const double old = n.returns[(size_t)(n.ret_turn & 1) * RL + row];
            const double now = n.is_clean[row] != 0 ? norm_return(n, row) : old;
            n.returns[(size_t)((n.ret_turn + 1) & 1) * RL + row] = n.dones[row] != 0 ? 0.0 : now;
        }
    }
    if (RESTART && col == 0 && n.update && n.returns) n.returns[(size_t)(n.ret_turn & 1) * RL + row] = 0.0;
}

#if defined(__HIPCC__)
// norm_fold on the device: the rows of a wavefront by shuffles, the wavefronts through `lds`; every lane of the workgroup calls
// it and gets its column's total
template <typename T>
__device__ __forceinline__ T norm_block_fold(T v, const NormLane& id, int rpw, int cols, T (*lds)[NORM_MAX_COLS]) {
    for (int half = norm_half0(rpw); half > 0; half >>= 1) {
        const T up = __shfl_down(v, (unsigned)(half * cols));
        if (id.r < half && id.r + half < rpw) v = v + up;
    }
    if (id.r == 0) lds[id.w][id.col] = v;
    __syncthreads();
    T t = lds[0][id.col];
    ROLLOUT_UNROLL
    for (int w = 1; w < NORM_WAVES; w++) t = t + lds[w][id.col];
    __syncthreads();  // (lds is written again by the next fold)
    return t;
}

template <bool RESTART>
__global__ __launch_bounds__(NORM_BLOCK) void k_norm_part(const NormDev n) {
    __shared__ double sum_w[NORM_WAVES][NORM_MAX_COLS];
    __shared__ uint32_t cnt_w[NORM_WAVES][NORM_MAX_COLS];
    const bool listed = RESTART && n.rows.list != nullptr;
    const size_t covered = tail_rows_count(n.rows, listed), tiles = norm_tiles(n, covered);
    const int rpw = plan_norm_rows_per_wave(n.cols);
    const NormLane id = norm_lane(n.cols, threadIdx.x);
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        double x[NORM_PER_LANE];
        const uint32_t have = norm_part_load<RESTART>(n, listed, covered, tile, id, x);
        const uint32_t c = norm_block_fold<uint32_t>((uint32_t)__builtin_popcount(have), id, rpw, n.cols, cnt_w);
        const double mean = norm_part_mean(norm_block_fold<double>(norm_lane_sum(x, have), id, rpw, n.cols, sum_w), c);
        const double m2 = norm_block_fold<double>(norm_lane_squares(x, have, mean), id, rpw, n.cols, sum_w);
        if ((int)threadIdx.x < n.cols) norm_part_store(n, tile, id.col, c, mean, m2);
    }
}

template <bool RESTART>
__global__ __launch_bounds__(NORM_BLOCK) void k_norm_apply(const NormDev n) {
    const bool listed = RESTART && n.rows.list != nullptr;
    const size_t covered = tail_rows_count(n.rows, listed);
    const int rpw = plan_norm_rows_per_wave(n.cols);
    const NormLane id = norm_lane(n.cols, threadIdx.x);
    NormTriple t = norm_stats_load(n, norm_stats_cur(n), id.col);
    if (n.update && (!RESTART || n.n_obs)) {
        t = norm_merge(t, norm_batch(n, norm_tiles(n, covered), id.col));
        if (blockIdx.x == 0 && (int)threadIdx.x < n.cols) norm_stats_store(n, id.col, t);
    }
    if (id.r >= rpw) return;
    const double den = sqrt(t.var + n.eps);
    const size_t pass = (size_t)gridDim.x * (size_t)(NORM_WAVES * rpw);
    for (size_t m = ((size_t)blockIdx.x * NORM_WAVES + (size_t)id.w) * (size_t)rpw + (size_t)id.r; m < covered; m += pass)
        norm_apply_item<RESTART>(n, listed, m, id.col, t.mean, den);
}
#endif
