// episodes.h -- TestEpisodeWrapper (envs/wrapper/evaluation_wrapper/TestEpisodeWrapper.py:8-119) and its TrajectoryPathHelper
// (evaluation_wrapper/utils.py:5-133) for every robot of a handle: how episodes end, how long they take, what they return and
// the path figures of the commands (variance and sign changes of w, mean |acceleration| and |jerk|, mean v and |w|), kept as
// running sums -- the rule of img_env_amd/envs.py's EpisodeStats / TestEpisodeWrapper, operation for operation, in float64.
//
// One kernel, two instantiations, launched at the end of every chain (launch_views) on the caller's stream:
//   accumulate (a step)         every local robot takes the step's command, reward and is_clean into its open episode
//   fold       (a reset chain)  the robots of the worlds the chain covers (tail_rows.h) close their episode by the LAST STEP's dones_info
//                               (imgenv_out.step_dones_info: a reset never touches it) and open the next one
// An auto-reset call runs a step chain and a reset chain, so a finished world's last step is accumulated and then folded.
//
// One lane per robot, state as structure of arrays ([field][RL]: a wavefront reads 64 neighbouring values of one field), no
// atomics, no LDS: a robot folds into its own row of totals, so every sum has one fixed order.  Only + - * / |x| rint and
// compares (the extension is compiled with -ffp-contract=off): every operation is IEEE-exact, the numpy model of
// tests/episode_model.py gives the same bits.
//
// State per robot: 27 float64 + 18 int32 = 288 bytes.  A step reads and writes the 15 + 2 rows of the open episode and the two
// running totals (152 bytes each way, + 17 bytes of inputs), a fold of a counted episode nearly all of it.
//
// The per-robot rules below compile as plain C++ as well (EP_HD), for tests/host/episode_log_check.cpp; the kernel is HIP only.
#pragma once
#include <math.h>
#include <stdint.h>

#include "launch_plan.h"  // EP_BLOCK, EP_MAX_BLOCKS
#include "tail_rows.h"

#if defined(__HIPCC__)
#define EP_HD __host__ __device__ __forceinline__
#else
#define EP_HD inline
#endif

// float64 rows: the open episode first (EpisodeStats' members, envs.py:388-396, then the running return) ...
enum {
    EPF_N = 0, EPF_SUM_V, EPF_SUM_W, EPF_SUM_WW, EPF_SUM_ABSW, EPF_ACC_V, EPF_ACC_W, EPF_JERK_V, EPF_JERK_W,
    EPF_PREV_V, EPF_PREV_W, EPF_PREV2_V, EPF_PREV2_W, EPF_W_ZERO,
    EPF_PATH_ROWS,                  // (the rows above restart with a COUNTED episode only)
    EPF_RETURN = EPF_PATH_ROWS,     // restarts with every reset
    EPF_OPEN_ROWS,
    // ... then the totals: running v and |w| (TestEpisodeWrapper.py v_sum / w_sum), the eight figures of finish() summed over the
    // counted episodes, their returns, and the last counted episode's return
    EPF_V_SUM = EPF_OPEN_ROWS, EPF_W_SUM,
    EPF_FIG0,                       // w_variance, w_zero, v_acc, w_acc, v_jerk, w_jerk, v_avg, w_avg
    EPF_RETURN_SUM = EPF_FIG0 + 8,
    EPF_LAST_RETURN,
    EPF_ROWS
};
// int32 rows
enum {
    EPI_TMP_STEPS = 0, EPI_LEN,     // the open episode: steps since its reset, of which clean
    EPI_OPEN_ROWS,
    EPI_ENDS0 = EPI_OPEN_ROWS,      // counted episodes by end: arrive, time-out, collision 1 / 2 / 3, aborted
    EPI_EPISODES = EPI_ENDS0 + 6, EPI_SHORT, EPI_SPEED_STEPS, EPI_ARRIVE_STEPS, EPI_LEN_SUM,
    EPI_LAST_CODE, EPI_LAST_STEPS, EPI_LAST_LEN, EPI_LAST_EPISODE,
    EPI_CLEARED_ROWS,               // (imgenv_episodes_clear zeroes the rows above)
    EPI_OPEN = EPI_CLEARED_ROWS,    // 1 once a reset has opened an episode
    EPI_ROWS
};

struct EpisodesDev {
    double* f;                   // [EPF_ROWS][RL]
    int32_t* i;                  // [EPI_ROWS][RL]
    const float* actions;        // [RL][3] (v, w, beep): the step's, valid until the chain's end (imgenv_step_begin)
    const double* step_rewards;  // [RL]  the working arena's imgenv_out.step_* rows
    const uint8_t* step_is_clean;
    const int32_t* step_dones_info;
    double dt;                   // control_hz: the divisor of the acceleration / jerk terms
    int32_t min_steps;
    TailRows rows;               // the robots of this launch (fold: those of the reset chain's worlds)
};

EP_HD double ep_round4(double x) { return rint(x * 1e4) / 1e4; }  // torch.round(x * 1e4) / 1e4

// EpisodeStats.add (envs.py:398-415) and TestEpisodeWrapper.step (envs.py:466-475) for robot row `r`
EP_HD void ep_accumulate(const EpisodesDev& e, size_t r) {
    const size_t RL = (size_t)e.rows.RL;
    double* f = e.f + r;
    int32_t* q = e.i + r;
    if (q[EPI_OPEN * RL] == 0) return;  // enabled in mid-episode: nothing is kept until a reset has opened one
    const bool clean = e.step_is_clean[r] != 0;
    const double v = clean ? (double)e.actions[r * 3] : 0.0, w = clean ? (double)e.actions[r * 3 + 1] : 0.0;
    const double dt = e.dt, n = f[EPF_N * RL];
    const bool has1 = n >= 1.0, has2 = n >= 2.0;
    q[EPI_TMP_STEPS * RL] += 1;
    f[EPF_V_SUM * RL] += v;
    f[EPF_W_SUM * RL] += fabs(w);
    const double pv = f[EPF_PREV_V * RL], pw = f[EPF_PREV_W * RL], p2v = f[EPF_PREV2_V * RL], p2w = f[EPF_PREV2_W * RL];
    {
        const double acc = (v - pv) / dt, acc_prev = (pv - p2v) / dt;
        f[EPF_ACC_V * RL] += has1 ? fabs(acc) : 0.0;
        f[EPF_JERK_V * RL] += has2 ? fabs((acc - acc_prev) / dt) : 0.0;
    }
    {
        const double acc = (w - pw) / dt, acc_prev = (pw - p2w) / dt;
        f[EPF_ACC_W * RL] += has1 ? fabs(acc) : 0.0;
        f[EPF_JERK_W * RL] += has2 ? fabs((acc - acc_prev) / dt) : 0.0;
    }
    const bool turn = (w == 0.0 && pw != 0.0) || (w > 0.0 && pw < 0.0) || (w < 0.0 && pw > 0.0);
    f[EPF_W_ZERO * RL] += turn ? 1.0 : 0.0;
    f[EPF_PREV2_V * RL] = pv;
    f[EPF_PREV2_W * RL] = pw;
    f[EPF_PREV_V * RL] = v;
    f[EPF_PREV_W * RL] = w;
    f[EPF_N * RL] = n + 1.0;
    f[EPF_SUM_V * RL] += v;
    f[EPF_SUM_W * RL] += w;
    f[EPF_SUM_WW * RL] += w * w;
    f[EPF_SUM_ABSW * RL] += fabs(w);
    f[EPF_RETURN * RL] += e.step_rewards[r];
    q[EPI_LEN * RL] += clean ? 1 : 0;
}

// EpisodeStats.finish (envs.py:417-431): the eight figures of the open episode of the robot whose float64 rows start at `f` (stride
// RL) -- what a fold adds to the robot's figure_sums and what the episode log (episode_log.h) records, from this one function
EP_HD void ep_figures(const double* f, size_t RL, double fig[8]) {
    const double n = f[EPF_N * RL];
    const double n0 = n < 1.0 ? 1.0 : n, n1 = n - 1.0 < 1.0 ? 1.0 : n - 1.0, n2 = n - 2.0 < 1.0 ? 1.0 : n - 2.0;  // clamp(min=1)
    const double mean_w = f[EPF_SUM_W * RL] / n0;
    fig[0] = ep_round4(f[EPF_SUM_WW * RL] / n0 - mean_w * mean_w);
    fig[1] = f[EPF_W_ZERO * RL];
    fig[2] = ep_round4(f[EPF_ACC_V * RL] / n1);
    fig[3] = ep_round4(f[EPF_ACC_W * RL] / n1);
    fig[4] = ep_round4(f[EPF_JERK_V * RL] / n2);
    fig[5] = ep_round4(f[EPF_JERK_W * RL] / n2);
    fig[6] = ep_round4(f[EPF_SUM_V * RL] / n0);
    fig[7] = ep_round4(f[EPF_SUM_ABSW * RL] / n0);
}

// TestEpisodeWrapper.reset / _count (envs.py:477-500) for robot row `r`
EP_HD void ep_fold(const EpisodesDev& e, size_t r) {
    const size_t RL = (size_t)e.rows.RL;
    double* f = e.f + r;
    int32_t* q = e.i + r;
    const int steps = q[EPI_TMP_STEPS * RL];
    if (q[EPI_OPEN * RL] != 0 && steps > e.min_steps) {
        const int code = e.step_dones_info[r];
        const int bin = code == 5 ? 0 : code == 10 ? 1 : (code >= 1 && code <= 3) ? 1 + code : 5;
        q[(EPI_ENDS0 + bin) * RL] += 1;
        const int episode = q[EPI_EPISODES * RL] + 1;
        q[EPI_EPISODES * RL] = episode;
        q[EPI_SPEED_STEPS * RL] += steps;
        q[EPI_ARRIVE_STEPS * RL] += code == 5 ? steps : 0;
        double fig[8];
        ep_figures(f, RL, fig);
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int k = 0; k < 8; k++) f[(EPF_FIG0 + k) * RL] += fig[k];
        const double ret = f[EPF_RETURN * RL];
        const int len = q[EPI_LEN * RL];
        f[EPF_RETURN_SUM * RL] += ret;
        q[EPI_LEN_SUM * RL] += len;
        f[EPF_LAST_RETURN * RL] = ret;
        q[EPI_LAST_CODE * RL] = code;
        q[EPI_LAST_STEPS * RL] = steps;
        q[EPI_LAST_LEN * RL] = len;
        q[EPI_LAST_EPISODE * RL] = episode;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int k = 0; k < EPF_PATH_ROWS; k++) f[k * RL] = 0.0;
    } else if (q[EPI_OPEN * RL] != 0) {
        // too short to count (TestEpisodeWrapper.py: `if self.tmp_steps > 3`): its commands ride into the next counted episode
        q[EPI_SHORT * RL] += 1;
    }
    q[EPI_TMP_STEPS * RL] = 0;
    q[EPI_LEN * RL] = 0;
    f[EPF_RETURN * RL] = 0.0;
    q[EPI_OPEN * RL] = 1;
}

#if defined(__HIPCC__)
template <bool FOLD>
__global__ __launch_bounds__(EP_BLOCK) void k_episodes(const EpisodesDev e) {
    // robots of this launch (tail_rows.h; blocks stride over whatever the count turns out to be)
    const bool listed = FOLD && e.rows.list != nullptr;
    const size_t total = tail_rows_count(e.rows, listed), stride = (size_t)gridDim.x * EP_BLOCK;
    for (size_t t = (size_t)blockIdx.x * EP_BLOCK + threadIdx.x; t < total; t += stride) {
        const size_t row = tail_rows_row(e.rows, listed, t);
        if (FOLD) ep_fold(e, row);
        else ep_accumulate(e, row);
    }
}
#endif  // __HIPCC__
