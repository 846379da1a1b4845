// final_obs.h -- the observation an episode ended on (Gym's final_observation / terminal_observation), for every robot row a reset
// chain covers: the chain's views and k_obs write the new episode's first observation over those rows of imgenv_out in place, and
// behind a device-side reset the host never learns which rows they were.  k_final_obs copies the rows of the selected fields into
// library-owned "final" arrays of the same shape and row numbering first.
//
// One kernel, launched at the head of a reset chain (launch_views(is_reset = 1), in front of the chain's first launch that writes
// a captured field), on the caller's stream; a step chain launches nothing.  The rows are tail_rows.h's: every local robot, or Rw
// per listed world in list order, the count the host's or the device's.  The sources are the fields of imgenv_out (always the
// kernels' working arena, as k_stack reads it), the whole [K][frame] rows of the observation stacks of depth >= 2 as the step's
// push left them, and imgenv_obs_post_out.ped_vector_norm.
//
// A row of a field is cut into chunks of `unit` bytes (launch_plan.h: plan_final_field; 16 for 4608-byte sensor maps, 2880-byte
// scans and 27648-byte ped_maps, 8 for 181 beams, 4 for 12- and 20-byte vector states, 1 for the one-byte flags); one lane copies
// one chunk, a flat grid-stride loop over rows x chunks per row.  The lane of a row's chunk 0 also bumps final_count[row]: a caller
// tells a fresh capture from an old one by the count, nothing is cleared per step.
//
// Algorithmic bytes per captured row: the selected fields' row sizes read and written once, + 4 + 4 for the count.
//
// final_obs_item, the loop body, is a host / device function: tests/host/final_obs_check.cpp runs it over a simulated grid.
#pragma once
#include <stdint.h>

#include "field_rows.h"
#include "launch_plan.h"  // FINAL_BLOCK, FINAL_MAX_BLOCKS, FINAL_MAX_FIELDS
#include "tail_rows.h"

struct FinalField {
    unsigned char* dst;        // [RL][row bytes]: the final array
    const unsigned char* src;  // [RL][row bytes]: the field's live array
    uint32_t unit;             // 16 | 8 | 4 | 2 | 1 (both bases are 256-byte aligned)
    uint32_t chunks;           // row bytes / unit
};

struct FinalObsDev {
    FinalField f[FINAL_MAX_FIELDS];
    int32_t n_fields;
    uint32_t chunks_per_row;  // sum of f[].chunks
    uint32_t* count;          // [RL] final_count
    TailRows rows;            // the robots of the reset chain in hand
};

template <typename T>
TAIL_HD void final_obs_copy(unsigned char* dst, const unsigned char* src, uint32_t chunks, size_t row, uint32_t c) {
    const size_t at = row * (size_t)chunks + c;
    ((T*)dst)[at] = ((const T*)src)[at];
}

// item t of the launch:chunk t % chunks_per_row of the (t / chunks_per_row)-th covered row
TAIL_HD void final_obs_item(const FinalObsDev& fo, bool listed, size_t t) {
    const size_t m = t / fo.chunks_per_row;
    uint32_t c = (uint32_t)(t - m * fo.chunks_per_row);
    const size_t row = tail_rows_row(fo.rows, listed, m);
    if (c == 0) fo.count[row] += 1;  // (one lane per row and launch: no atomic)
    const FinalField f = field_walk(fo.f, fo.n_fields, c);
    field_dispatch(f.unit, [&](auto chunk) { final_obs_copy<typename decltype(chunk)::type>(f.dst, f.src, f.chunks, row, c); });
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(FINAL_BLOCK) void k_final_obs(const FinalObsDev fo) {
    // (blocks stride over whatever the count turns out to be: behind a device-side reset the grid is sized for a guess)
    const bool listed = fo.rows.list != nullptr;
    const size_t total = tail_rows_count(fo.rows, listed) * fo.chunks_per_row, stride = (size_t)gridDim.x * FINAL_BLOCK;
    for (size_t t = (size_t)blockIdx.x * FINAL_BLOCK + threadIdx.x; t < total; t += stride) final_obs_item(fo, listed, t);
}
#endif
