// episode_log.h -- one record per finished episode, in a ring in device memory (include/imgenv.h: imgenv_episode_log_enable).
// The reference writes one line per episode of a fixed test set (PedTrajectoryDatasetWrapper.out2logfile, BarnDataSetWrapper.
// out2logfile: which world, how it ended, v_avg ... w_zero, path_time, steps) and TestEpisodeWrapper keeps per-episode lists
// (w_variance_array, ...); episodes.h keeps running totals only.  Here every reset chain appends, in front of its fold
// (k_episodes<true>), one record per episode it closes, tagged with what the episode ran on.
//
// One launch per reset chain, in front of k_episodes<true> on the caller's stream, so it reads the state the fold is about to
// consume.  The chain covers robot rows in tail_rows.h order; each covered row with an open episode appends one record, in that
// order: the log is deterministic -- chains in stream order, rows in tail order.  Record q (counted since enabling) lives in slot
// q % capacity; of a chain that closes more episodes than the ring holds only the last `capacity` are written, so no two lanes
// ever store to one slot.  Every covered row, open or not, then takes the tags of the episode that starts, from the device words
// the chain has already written (the map bank's cur[], the track bank's cur[], k_scenario_mark's words, k_respawn's place_serial).
//
// Everything that changes per chain is read from device memory: the counter, the tags, the list and its length.
//
// The per-row rules compile as plain C++ (tests/host/episode_log_check.cpp walks them in chunks as the kernel does); the kernel is
// HIP only: one workgroup of EPLOG_BLOCK lanes, k_finished_dev's pattern -- a uniform-trip-count loop over the covered rows in
// chunks of EPLOG_BLOCK, a wave64 ballot and its popcount per wavefront, the 16 wave counts in LDS, a running base; lane 0
// advances n_written once, at the end.  No atomics, plain vector stores.
#pragma once
#include <stdint.h>

#include "episodes.h"

// rows of EpisodeLogDev::i32 (IMGENV_EPLOG_I32 of them) ...
enum { EPL_ROBOT = 0, EPL_WORLD, EPL_CODE, EPL_STEPS, EPL_LEN, EPL_COUNTED, EPL_EPISODE, EPL_MAP, EPL_TRACKS, EPL_SCENARIO, EPL_I32_ROWS };
// ... of f64 (IMGENV_EPLOG_F64): the return, then the eight figures ...
enum { EPL_RETURN = 0, EPL_FIG0, EPL_F64_ROWS = EPL_FIG0 + 8 };
// ... and of the per-robot tags of the open episode
enum { EPT_MAP = 0, EPT_TRACKS, EPT_SCENARIO, EPT_ROWS };
#define EPLOG_SCN_DEVICE (-2)  // IMGENV_EPLOG_SCN_DEVICE

struct EpisodeLogDev {
    unsigned long long* n_written;  // [1] records appended since enabling
    int32_t* i32;                   // [EPL_I32_ROWS][capacity]
    double* f64;                    // [EPL_F64_ROWS][capacity]
    unsigned long long* placement;  // [capacity]
    int32_t capacity;
    int32_t W;                      // worlds of the handle (1 on a robot shard)
    int32_t* tags;                  // [EPT_ROWS][RL] what each robot's open episode runs on (-1: it was open before the log was)
    unsigned long long* tag_place;  // [RL] its world's placement number when it opened (~0: none)
    // where a chain's tags come from (each nullptr without that bank / before the first device-side reset)
    const int* map_cur;                      // [W]
    const int* trk_cur;                      // [W]
    const int* scn_world;                    // [W]
    const unsigned long long* scn_mark;      // [W]
    const unsigned long long* place_serial;  // [W]
};

// the world of local row `row`: row / Rw on a whole handle, 0 on a robot shard (which holds one world)
EP_HD int32_t eplog_world(const EpisodesDev& e, const EpisodeLogDev& g, size_t row) {
    const size_t w = row / (size_t)e.rows.Rw;
    return w < (size_t)g.W ? (int32_t)w : g.W - 1;
}
EP_HD bool eplog_open(const EpisodesDev& e, size_t row) { return e.i[EPI_OPEN * (size_t)e.rows.RL + row] != 0; }
// of the records seq .. n_end - 1 a chain appends, the ring keeps the last `capacity`
EP_HD bool eplog_kept(unsigned long long seq, unsigned long long n_end, int32_t capacity) { return n_end - seq <= (unsigned long long)capacity; }

// the record of the open episode of row `row`, as the fold behind this launch will count it, into the slot of number `seq`
EP_HD void eplog_record(const EpisodesDev& e, const EpisodeLogDev& g, size_t row, unsigned long long seq) {
    const size_t RL = (size_t)e.rows.RL, C = (size_t)g.capacity, s = (size_t)(seq % (unsigned long long)g.capacity);
    const double* f = e.f + row;
    const int32_t* q = e.i + row;
    const int steps = q[EPI_TMP_STEPS * RL];
    const bool counted = steps > e.min_steps;
    double fig[8];
    ep_figures(f, RL, fig);
    g.i32[EPL_ROBOT * C + s] = (int32_t)row;
    g.i32[EPL_WORLD * C + s] = eplog_world(e, g, row);
    g.i32[EPL_CODE * C + s] = e.step_dones_info[row];
    g.i32[EPL_STEPS * C + s] = steps;
    g.i32[EPL_LEN * C + s] = q[EPI_LEN * RL];
    g.i32[EPL_COUNTED * C + s] = counted ? 1 : 0;
    g.i32[EPL_EPISODE * C + s] = counted ? q[EPI_EPISODES * RL] + 1 : 0;
    g.i32[EPL_MAP * C + s] = g.tags[EPT_MAP * RL + row];
    g.i32[EPL_TRACKS * C + s] = g.tags[EPT_TRACKS * RL + row];
    g.i32[EPL_SCENARIO * C + s] = g.tags[EPT_SCENARIO * RL + row];
    g.f64[EPL_RETURN * C + s] = f[EPF_RETURN * RL];
    for (int k = 0; k < 8; k++) g.f64[(EPL_FIG0 + k) * C + s] = counted ? fig[k] : 0.0;
    g.placement[s] = g.tag_place[row];
}

// the tags of the episode that starts on row `row`
EP_HD void eplog_retag(const EpisodesDev& e, const EpisodeLogDev& g, size_t row) {
    const size_t RL = (size_t)e.rows.RL;
    const int32_t w = eplog_world(e, g, row);
    const unsigned long long serial = g.place_serial ? g.place_serial[w] : ~0ull;
    g.tags[EPT_MAP * RL + row] = g.map_cur ? g.map_cur[w] : 0;
    g.tags[EPT_TRACKS * RL + row] = g.trk_cur ? g.trk_cur[w] : -1;
    g.tags[EPT_SCENARIO * RL + row] = !g.scn_world ? -1 : g.scn_mark[w] == serial ? g.scn_world[w] : EPLOG_SCN_DEVICE;
    g.tag_place[row] = serial;
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(EPLOG_BLOCK) void k_episode_log(const EpisodesDev e, const EpisodeLogDev g) {
    __shared__ int wave_n[EPLOG_BLOCK / WAVE];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid >> 6;
    const bool listed = e.rows.list != nullptr;
    const size_t total = tail_rows_count(e.rows, listed);  // (uniform: the host's count or the device's)
    const unsigned long long n0 = *g.n_written;
    // how many records the chain appends: decides which of them the ring keeps.  This second walk of the list, every open flag read
    // twice on the one serial workgroup, is paid by every reset chain for the sake of rings smaller than a chain: only there could
    // two lanes otherwise meet in one slot.
    int mine = 0;
    for (size_t k0 = 0; k0 < total; k0 += EPLOG_BLOCK) {  // uniform trip count
        const size_t m = k0 + tid;
        const bool open = m < total && eplog_open(e, tail_rows_row(e.rows, listed, m));
        mine += __popcll(__ballot(open));
    }
    if (lane == 0) wave_n[wv] = mine;
    __syncthreads();
    unsigned long long n_end = n0;
    for (int q = 0; q < EPLOG_BLOCK / WAVE; q++) n_end += (unsigned long long)wave_n[q];
    __syncthreads();
    unsigned long long base = n0;  // the number of the chunk's first record
    for (size_t k0 = 0; k0 < total; k0 += EPLOG_BLOCK) {
        const size_t m = k0 + tid;
        const bool covered = m < total;
        const size_t row = covered ? tail_rows_row(e.rows, listed, m) : 0;
        const bool open = covered && eplog_open(e, row);
        const unsigned long long mask = __ballot(open);
        if (lane == 0) wave_n[wv] = __popcll(mask);
        __syncthreads();
        unsigned long long before = base, chunk = 0;
        for (int q = 0; q < EPLOG_BLOCK / WAVE; q++) {
            before += q < wv ? (unsigned long long)wave_n[q] : 0ull;
            chunk += (unsigned long long)wave_n[q];
        }
        if (open) {
            const unsigned long long seq = before + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
            if (eplog_kept(seq, n_end, g.capacity)) eplog_record(e, g, row, seq);
        }
        if (covered) eplog_retag(e, g, row);
        base += chunk;
        __syncthreads();  // (wave_n is rewritten by the next chunk)
    }
    if (tid == 0) *g.n_written = n_end;
}
#endif  // __HIPCC__
