// sequences.h -- sequence minibatches out of the rollout storage (rollout.h), for recurrent policies: the window cut into chunks
// of L steps per row, which of them count, a fresh random order over them, and the gather of Bs of them into TIME-MAJOR rows.
// R local rows, horizon T, cursor n, k = t R + row as in rollout.h and minibatch.h; C = ceil(n / L) chunks per row, C_max =
// ceil(T / L).  Sequence q = c R + row, 0 <= q < C R, covers row `row`'s transitions t = c L .. min(c L + L, n) - 1.  Chunks are
// aligned to the window, not to episodes: an episode boundary inside a chunk is marked (mb_first), not split.
//
// Everything is the library's (imgenv_rollout_seq_enable; include/imgenv.h has the table):
//   seq_flag [C_max R] u8   1 iff any covered transition has is_clean != 0
//   seq_valid [C_max R]     the q with the flag set, ascending;  seq_valid_n  their count Vs
//   seq_order [C_max R]     seq_order[p] = seq_valid[pi(p)] for p < Vs, -1 behind
//   tile_count / tile_base [tiles]   the compaction's scratch, the feature's own
//   mb_* per buffer         the gathered minibatch, [L][Bs]...
//
// The index, four launches; the launch boundaries are the only synchronisation -- no workgroup ever waits for another, no atomics:
//   k_seq_flag    a lane per q; consecutive lanes take consecutive rows of one chunk, so each of the up to L byte loads of a lane
//                 is part of a coalesced wavefront read, R apart; one byte stored per lane
//   k_mb_count, k_mb_scan, k_mb_scatter (minibatch.h) on an MbIndexDev whose `clean` is seq_flag and whose `total` is C R
// The shuffle, one launch: k_mb_shuffle (minibatch.h) on an MbShuffleDev of the sequence arrays; Vs is read on the device.
// The gather, one launch, k_rollout_seq_gather: k_rollout_gather's walk -- chunks of 16 / 8 / 4 / 2 / 1 bytes (plan_final_field), a
//   lane per chunk, a flat grid-stride loop, the field table by value and selected with constant indices.  Field item t is chunk
//   t % chunks_per_row of destination row t / chunks_per_row = l Bs + i: a wavefront's chunks are consecutive in one destination
//   row (and in one source row).  Slot i takes q = seq_order[j Bs + i] (-1 from C_max R on); step l is t = c L + l, k = t R + row
//   where q >= 0 and t < n, else k = -1: k >= 0 copies, k < 0 writes zeros.  The chunk-0 lane of (l, i) writes that step's
//   scalars, the one of (0, i) also the slot's mb_seq and mb_seq_len.  Behind the field items, in the same launch, the state items:
//   chunk u % state_chunks of slot u / state_chunks, the caller's row at the sequence's first step k0 = c L R + row.
//   No LDS, no scratch.
//
// mb_first is final_idx[t][row] >= 0: a reset chain rewrote slot t's observation, so the row's episode starts at this step (the
// device-side reset, the host-side ones, a caller's reset in mid-episode or at n = 0).  It does NOT say whether slot 0 continues
// the previous window: imgenv_rollout_begin clears final_idx, and the caller's stored initial state carries that.
//
// Algorithmic bytes: flags n R read + C R written; compaction C R read twice + 4 Vs written; shuffle 4 Vs read + 4 C_max R
// written; a minibatch L Bs x (the selected rows + 12 + 4 + 1 + 4 + 1 + 4 + 4 S) read and the same + 4 written, + Bs x the state rows.
//
// The per-item functions are host / device functions: tests/host/seq_check.cpp runs them over a simulated grid against
// tests/seq_model.py.  They are timed nowhere in imgenv_timing.
#pragma once
#include <stdint.h>

#include "field_rows.h"
#include "launch_plan.h"  // SEQ_*, ROLLOUT_BLOCK, ROLLOUT_MAX_BLOCKS, ROLLOUT_TABLE_FIELDS
#include "minibatch.h"    // MbIndexDev, MbShuffleDev, MbGatherField, MB_MAX_SCALARS

// ---- the flags
struct SeqFlagDev {
    const uint8_t* clean;  // [n][R]
    uint8_t* flag;         // [C R]
    uint32_t R, L, n;
    uint32_t total;        // C R
};
TAIL_HD void seq_flag_item(const SeqFlagDev& d, uint32_t q) {
    const uint32_t c = q / d.R, row = q - c * d.R;
    const uint32_t t0 = c * d.L, t1 = t0 + d.L < d.n ? t0 + d.L : d.n;
    uint32_t any = 0;
    for (uint32_t t = t0; t < t1; t++) any |= d.clean[(size_t)t * d.R + row];
    d.flag[q] = any ? 1 : 0;
}

// ---- the gather
struct SeqState {
    const unsigned char* src;  // the caller's [T or T+1][R][row bytes]
    unsigned char* dst;        // mb_seq_state[a] [Bs][row bytes] of the buffer in hand
    uint32_t unit, chunks;     // (chunks 0: no such array)
};
struct SeqGatherDev {
    MbGatherField f[ROLLOUT_TABLE_FIELDS];  // dst: mb_<field> [L][Bs][row bytes]
    int32_t n_fields;
    uint32_t chunks_per_row;
    SeqState st[SEQ_MAX_STATES];
    uint32_t state_chunks;    // st[0].chunks + st[1].chunks
    const int32_t* order;     // seq_order [S]
    size_t first;             // j Bs
    uint32_t Bs, L, R, S;     // S = C_max R
    int32_t n;                // the cursor
    // the ring's [T][R] arrays
    const float* actions;     // [.][3]
    const float* rewards;
    const uint8_t* dones;
    const uint8_t* is_clean;
    const int32_t* dones_info;
    const int32_t* final_idx; // [T+1][R]
    // the buffer's [L][Bs] arrays
    float* mb_actions;
    float* mb_rewards;
    uint8_t* mb_dones;
    int32_t* mb_dones_info;
    int32_t* mb_index;
    float* mb_weight;
    uint8_t* mb_first;
    float* mb_scalars;        // [MB_MAX_SCALARS][L][Bs]
    int32_t* mb_seq;          // [Bs]
    int32_t* mb_seq_len;
    const float* scalars[MB_MAX_SCALARS];  // the caller's, indexed by k
    int32_t n_scalars, normalise;          // normalise: an index into scalars or -1
    const float* norm;        // [2]
};

// the sequence of slot i, -1 for none
TAIL_HD int32_t seq_of_slot(const SeqGatherDev& g, size_t i) {
    const size_t pos = g.first + i;
    const int32_t q = pos < (size_t)g.S ? g.order[pos] : -1;
    return q >= 0 ? q : -1;
}
// transition k of step l of sequence q, -1 where the step does not exist
TAIL_HD int32_t seq_step(const SeqGatherDev& g, int32_t q, uint32_t l) {
    if (q < 0) return -1;
    const uint32_t c = (uint32_t)q / g.R, row = (uint32_t)q - c * g.R, t = c * g.L + l;
    return t < (uint32_t)g.n ? (int32_t)(t * g.R + row) : -1;
}
template <int S>
TAIL_HD void seq_gather_scalars(const SeqGatherDev& g, int32_t k, size_t d, size_t N) {
    if constexpr (S < MB_MAX_SCALARS) {
        if (S < g.n_scalars) {
            float v = 0.0f;
            if (k >= 0) {
                v = g.scalars[S][k];
                if (S == g.normalise) {
                    const float e = v - g.norm[0];  // (two roundings: the build has -ffp-contract=off)
                    v = e * g.norm[1];
                }
            }
            g.mb_scalars[(size_t)S * N + d] = v;
            seq_gather_scalars<S + 1>(g, k, d, N);
        }
    }
}
template <typename T>
TAIL_HD void seq_state_chunk(const SeqState& s, int32_t k0, size_t i, uint32_t c) {
    T v = T{};
    if (k0 >= 0) v = ((const T*)s.src)[(size_t)k0 * s.chunks + c];
    ((T*)s.dst)[i * (size_t)s.chunks + c] = v;
}
// item t of a launch.  t < L Bs chunks_per_row: chunk t % chunks_per_row of destination row d = t / chunks_per_row = l Bs + i;
// behind them: state chunk u % state_chunks of slot u / state_chunks
TAIL_HD void seq_gather_item(const SeqGatherDev& g, size_t t) {
    const size_t N = (size_t)g.L * g.Bs, field_items = N * g.chunks_per_row;
    if (t >= field_items) {
        const size_t u = t - field_items, i = u / g.state_chunks;
        uint32_t c = (uint32_t)(u - i * g.state_chunks);
        const int32_t k0 = seq_step(g, seq_of_slot(g, i), 0);
        SeqState s = g.st[0];
        if (c >= s.chunks) {
            c -= s.chunks;
            s = g.st[1];
        }
        field_dispatch<4>(s.unit, [&](auto chunk) { seq_state_chunk<typename decltype(chunk)::type>(s, k0, i, c); });
        return;
    }
    const size_t d = t / g.chunks_per_row;
    uint32_t c = (uint32_t)(t - d * g.chunks_per_row);
    const uint32_t l = (uint32_t)(d / g.Bs);
    const size_t i = d - (size_t)l * g.Bs;
    const int32_t q = seq_of_slot(g, i), k = seq_step(g, q, l);
    if (c == 0) {  // (one lane per step of a slot)
        float v = 0.0f, w = 0.0f, beep = 0.0f, reward = 0.0f, weight = 0.0f;
        uint8_t done = 0, first = 0;
        int32_t info = 0;
        if (k >= 0) {
            v = g.actions[(size_t)k * 3]; w = g.actions[(size_t)k * 3 + 1]; beep = g.actions[(size_t)k * 3 + 2];
            reward = g.rewards[k];
            done = g.dones[k];
            info = g.dones_info[k];
            weight = g.is_clean[k] != 0 ? 1.0f : 0.0f;
            first = g.final_idx[k] >= 0 ? 1 : 0;
        }
        g.mb_actions[d * 3] = v;
        g.mb_actions[d * 3 + 1] = w;
        g.mb_actions[d * 3 + 2] = beep;
        g.mb_rewards[d] = reward;
        g.mb_dones[d] = done;
        g.mb_dones_info[d] = info;
        g.mb_index[d] = k;
        g.mb_weight[d] = weight;
        g.mb_first[d] = first;
        seq_gather_scalars<0>(g, k, d, N);
        if (l == 0) {  // (one lane per slot)
            int32_t len = 0;
            if (q >= 0) {
                const int32_t t0 = (int32_t)(((uint32_t)q / g.R) * g.L), left = g.n - t0;
                len = left < 0 ? 0 : left < (int32_t)g.L ? left : (int32_t)g.L;
            }
            g.mb_seq[i] = q;
            g.mb_seq_len[i] = len;
        }
    }
    if (g.n_fields == 0) return;  // (every selected field is drawn, ped_draw.h: chunks_per_row is 1, the scalars' lane)
    const MbGatherField f = field_walk(g.f, g.n_fields, c);
    field_dispatch(f.unit, [&](auto chunk) { mb_gather_chunk<typename decltype(chunk)::type>(f.ring, f.dst, f.chunks, k, d, c); });
}
TAIL_HD size_t seq_gather_items(const SeqGatherDev& g) { return (size_t)g.L * g.Bs * g.chunks_per_row + (size_t)g.Bs * g.state_chunks; }

#if defined(__HIPCC__)
__global__ __launch_bounds__(SEQ_FLAG_BLOCK) void k_seq_flag(const SeqFlagDev d) {
    const size_t q = (size_t)blockIdx.x * SEQ_FLAG_BLOCK + threadIdx.x;
    if (q < (size_t)d.total) seq_flag_item(d, (uint32_t)q);
}

__global__ __launch_bounds__(ROLLOUT_BLOCK) void k_rollout_seq_gather(const SeqGatherDev g) {
    const size_t total = seq_gather_items(g), stride = (size_t)gridDim.x * ROLLOUT_BLOCK;
    for (size_t t = (size_t)blockIdx.x * ROLLOUT_BLOCK + threadIdx.x; t < total; t += stride) seq_gather_item(g, t);
}
#endif
