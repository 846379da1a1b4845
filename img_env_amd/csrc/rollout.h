// rollout.h -- a trainer's rollout storage on the device: what imgenv_out shows after every chain, kept per time slot, and the
// advantage pass (GAE) over it.  The arrays of imgenv_out are the kernels' working copies -- the next step rewrites them, the
// stacks shift in place -- so a trainer has to copy every observation field, reward, done, mask and action away after every step;
// and only the library knows which rows a reset chain has just overwritten and which transitions count.
//
// The ring (all library-owned; R = local robots, T = horizon, F = final capacity; include/imgenv.h has the full table):
//   obs_<field>  [T+1][R][row bytes]   slot s = the observation transition s starts from
//   actions, rewards, dones, is_clean, dones_info   [T][R]   transition s
//   final_idx    [T+1][R]              -1, or the final-list entry that holds what slot s showed before a reset chain overwrote it
//   final_<field> [F][row bytes], final_slot / final_row [F], final_n [2]
// The cursor n (transitions stored) and the count of reset chains since imgenv_rollout_begin are the host's, passed by value.
//
// One kernel, k_rollout<RESTART>, the last launch of every chain (launch_views: behind k_obs_post, in front of the seal):
//   a step chain (RESTART = false), for every local row: the transition scalars into slot n, the observation rows into slot n + 1;
//   a reset chain (RESTART = true), for the m-th row it covers (tail_rows.h): entry e = final_n[turn & 1] + m; where e < F the
//     row's chunks of slot n move into final_<field>[e]; the new live chunks go into slot n; the lane of chunk 0 writes
//     final_idx[n][row] = e and, where e < F, final_slot[e] / final_row[e]; one thread stores final_n[(turn + 1) & 1] =
//     final_n[turn & 1] + covered rows.  The word a launch reads is never the word it writes, so no lane waits for another.
//     e >= F is overflow: the entry is dropped, final_idx and final_n still tell the caller.
// imgenv_rollout_begin runs the step instantiation once more with the scalars off (rewards == nullptr), n = -1 and the sources
// pointing at slot n: the copy of slot n into slot 0.
//
// A row of a field is cut into chunks of 16 / 8 / 4 / 2 / 1 bytes (launch_plan.h: plan_final_field), one lane per chunk, a flat
// grid-stride loop over rows x chunks per row, the field table by value in the arguments and selected with constant indices
// (field_rows.h).  No LDS, no scratch.
//
// Algorithmic bytes per row: a step reads and writes the selected rows once, + 12 + 8 + 1 + 1 + 4 read and 12 + 4 + 1 + 1 + 4 written;
// a reset chain reads the live rows and (e < F) slot n's, writes both, + 4 (+ 8) for the index.
//
// k_rollout_gae: one lane per local row walks t = n - 1 .. 0 over [t][R] arrays (a wavefront reads consecutive words); the loads of
// GAE_BATCH steps are issued before their dependent chain is walked, since only `gae` carries from step to step.  Float32
// throughout, in the order written in rollout_gae_row (the build has -ffp-contract=off).
//
// rollout_item, rollout_count and rollout_gae_row are host / device functions: tests/host/rollout_check.cpp runs them over a
// simulated grid against tests/rollout_model.py.
#pragma once
#include <stdint.h>

#include "field_rows.h"
#include "launch_plan.h"  // ROLLOUT_BLOCK, ROLLOUT_MAX_BLOCKS, ROLLOUT_TABLE_FIELDS, GAE_BLOCK, GAE_BATCH
#include "tail_rows.h"

#if defined(__HIPCC__)
#define ROLLOUT_UNROLL _Pragma("unroll")
#else
#define ROLLOUT_UNROLL
#endif

struct RolloutField {
    unsigned char* ring;       // [T+1][RL][row bytes]
    unsigned char* fin;        // [F][row bytes]
    const unsigned char* src;  // [RL][row bytes]: the field's live array (imgenv_rollout_begin: slot n of the ring)
    uint32_t unit;             // 16 | 8 | 4 | 2 | 1 (every base is 256-byte aligned)
    uint32_t chunks;           // row bytes / unit
};

struct RolloutDev {
    RolloutField f[ROLLOUT_TABLE_FIELDS];
    int32_t n_fields;
    uint32_t chunks_per_row;  // sum of f[].chunks
    // the transition of a step: the sources ([RL], the working arena's imgenv_out.step_* rows and the step's actions) ...
    const float* act_src;     // [RL][3]
    const double* rew_src;
    const uint8_t* done_src;
    const uint8_t* clean_src;
    const int32_t* info_src;
    // ... and the ring's [T][RL] arrays (rewards == nullptr: no scalars, imgenv_rollout_begin's copy)
    float* actions;           // [T][RL][3]
    float* rewards;
    uint8_t* dones;
    uint8_t* is_clean;
    int32_t* dones_info;
    int32_t* final_idx;       // [T+1][RL]
    int32_t* final_slot;      // [F]
    int32_t* final_row;       // [F]
    uint32_t* final_n;        // [2]
    int32_t n;                // a step: the transition it stores (scalars of slot n, rows of slot n + 1); a reset chain: the slot it rewrites
    uint32_t turn;            // reset chains since imgenv_rollout_begin: which word of final_n is read
    int32_t F;
    TailRows rows;            // the robots of the chain in hand
};

// chunk c of `row`: a step stores the live chunk in `slot`; a reset chain first moves what the slot holds into final entry e (`keep`)
template <typename T, bool RESTART>
TAIL_HD void rollout_chunk(unsigned char* ring, unsigned char* fin, const unsigned char* src, uint32_t chunks, size_t at_ring, size_t row,
                           size_t e, bool keep, uint32_t c) {
    const T live = ((const T*)src)[row * (size_t)chunks + c];
    T* at = (T*)ring + at_ring * (size_t)chunks + c;
    if (RESTART && keep) {
        const T old = *at;
        ((T*)fin)[e * (size_t)chunks + c] = old;
    }
    *at = live;
}

// item t of a launch: chunk t % chunks_per_row of the (t / chunks_per_row)-th covered row.  `base`: final_n[turn & 1] (RESTART)
template <bool RESTART>
TAIL_HD void rollout_item(const RolloutDev& ro, bool listed, uint32_t base, size_t t) {
    const size_t m = t / ro.chunks_per_row;
    uint32_t c = (uint32_t)(t - m * ro.chunks_per_row);
    const size_t row = tail_rows_row(ro.rows, listed, m), RL = (size_t)ro.rows.RL;
    const size_t slot = (size_t)(RESTART ? ro.n : ro.n + 1), at_ring = slot * RL + row;
    const size_t e = RESTART ? (size_t)base + m : 0;
    const bool keep = RESTART && e < (size_t)ro.F;
    if (c == 0) {  // (one lane per row and launch)
        if (RESTART) {
            ro.final_idx[at_ring] = (int32_t)(e < 0x7fffffffu ? e : 0x7fffffffu);
            if (keep) {
                ro.final_slot[e] = (int32_t)slot;
                ro.final_row[e] = (int32_t)row;
            }
        } else if (ro.rewards) {
            const size_t at = (size_t)ro.n * RL + row;
            const float v = ro.act_src[row * 3], w = ro.act_src[row * 3 + 1], beep = ro.act_src[row * 3 + 2];
            const double reward = ro.rew_src[row];
            const uint8_t done = ro.done_src[row], clean = ro.clean_src[row];
            const int32_t info = ro.info_src[row];
            ro.actions[at * 3] = v;
            ro.actions[at * 3 + 1] = w;
            ro.actions[at * 3 + 2] = beep;
            ro.rewards[at] = (float)reward;  // (rounded once, to nearest)
            ro.dones[at] = done;
            ro.is_clean[at] = clean;
            ro.dones_info[at] = info;
        }
    }
    const RolloutField f = field_walk(ro.f, ro.n_fields, c);
    field_dispatch(f.unit, [&](auto chunk) {
        rollout_chunk<typename decltype(chunk)::type, RESTART>(f.ring, f.fin, f.src, f.chunks, at_ring, row, e, keep, c);
    });
}

// one thread of a reset chain's launch: the entries so far, into the word the NEXT reset chain reads
TAIL_HD void rollout_count(const RolloutDev& ro, uint32_t base, size_t covered) { ro.final_n[(ro.turn + 1) & 1] = base + (uint32_t)covered; }

// ---- the advantage pass
struct RolloutGaeDev {
    const float* rewards;      // [T][RL]
    const uint8_t* dones;
    const uint8_t* is_clean;
    const int32_t* dones_info;
    const int32_t* final_idx;  // [T+1][RL]
    const float* values;       // [T+1][RL], the caller's
    const float* final_values; // [F] or nullptr, the caller's
    float* adv;                // [T][RL], the caller's
    float* ret;
    float gamma, lam;
    int32_t n, F, RL;
};

// GAE for one row, t = n - 1 .. 0:
//   a real end (dones, dones_info != 10) bootstraps from nothing; a row whose next slot a reset chain overwrote (final_idx >= 0: a
//   time-out, or a caller's reset in mid-episode) from the value of what the reset overwrote, 0 where the entry was dropped or no
//   final_values are given; anything else -- a time-out nobody has reset yet included -- from the next slot.  The trace stops at a
//   done and at a restart.  A row that was not clean (a frozen robot of MultiRobotCleanWrapper) gets 0 and cuts the trace.
TAIL_HD void rollout_gae_row(const RolloutGaeDev& g, size_t row) {
    const size_t RL = (size_t)g.RL;
    const float gl = g.gamma * g.lam;
    float gae = 0.0f;
    for (int t0 = g.n - 1; t0 >= 0; t0 -= GAE_BATCH) {
        float reward[GAE_BATCH] = {}, v[GAE_BATCH] = {}, nv[GAE_BATCH] = {};
        bool clean[GAE_BATCH] = {}, cont[GAE_BATCH] = {};
        ROLLOUT_UNROLL
        for (int i = 0; i < GAE_BATCH; i++) {
            const int t = t0 - i;
            if (t < 0) continue;
            const size_t at = (size_t)t * RL + row;
            const int32_t e = g.final_idx[at + RL];
            const bool done = g.dones[at] != 0;
            const bool terminal = done && g.dones_info[at] != 10;
            float next = g.values[at + RL];
            if (e >= 0) next = (e < g.F && g.final_values) ? g.final_values[e] : 0.0f;
            reward[i] = g.rewards[at];
            v[i] = g.values[at];
            nv[i] = terminal ? 0.0f : next;
            clean[i] = g.is_clean[at] != 0;
            cont[i] = !(done || e >= 0);
        }
        ROLLOUT_UNROLL
        for (int i = 0; i < GAE_BATCH; i++) {
            const int t = t0 - i;
            if (t < 0) continue;
            const size_t at = (size_t)t * RL + row;
            float a = 0.0f, r = 0.0f;
            if (!clean[i]) {
                gae = 0.0f;
            } else {
                const float m = g.gamma * nv[i];
                const float s = reward[i] + m;
                const float delta = s - v[i];
                float c = gl * gae;
                c = cont[i] ? c : 0.0f;
                gae = delta + c;
                a = gae;
                r = gae + v[i];
            }
            g.adv[at] = a;
            g.ret[at] = r;
        }
    }
}

#if defined(__HIPCC__)
template <bool RESTART>
__global__ __launch_bounds__(ROLLOUT_BLOCK) void k_rollout(const RolloutDev ro) {
    // (blocks stride over whatever the count turns out to be: behind a device-side reset the grid is sized for a guess)
    const bool listed = RESTART && ro.rows.list != nullptr;
    const size_t covered = tail_rows_count(ro.rows, listed);
    const uint32_t base = RESTART ? ro.final_n[ro.turn & 1] : 0u;
    const size_t total = covered * ro.chunks_per_row, stride = (size_t)gridDim.x * ROLLOUT_BLOCK;
    for (size_t t = (size_t)blockIdx.x * ROLLOUT_BLOCK + threadIdx.x; t < total; t += stride) rollout_item<RESTART>(ro, listed, base, t);
    if (RESTART && blockIdx.x == 0 && threadIdx.x == 0) rollout_count(ro, base, covered);
}

__global__ __launch_bounds__(GAE_BLOCK) void k_rollout_gae(const RolloutGaeDev g) {
    const size_t stride = (size_t)gridDim.x * GAE_BLOCK;
    for (size_t row = (size_t)blockIdx.x * GAE_BLOCK + threadIdx.x; row < (size_t)g.RL; row += stride) rollout_gae_row(g, row);
}
#endif
