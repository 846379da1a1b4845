// stack.h -- StateBatchWrapper (envs/wrapper/base.py:97-150) for every robot of a handle: the last K frames of a field, oldest
// first, newest last, contiguous per robot ([R][K][frame]), zero-padded at the start of an episode.
//
// One kernel, two instantiations, launched at the end of every chain (launch_views) on the caller's stream:
//   push    (a step)          stack = [old[1], ..., old[K-1], F]   for every local robot
//   restart (a reset chain)   stack = [0, ..., 0, F]               for the robots of the worlds the chain covers (tail_rows.h)
// where F is the field's row of imgenv_out (always the kernels' working arena) after that chain.  An auto-reset call runs a step
// chain and a reset chain, so its finished worlds are pushed and then restarted: the reference's result by composition.
//
// The shift is done in place and needs no barrier: a frame is cut into chunks of `unit` bytes (16 where the frame size allows it:
// 4608-byte sensor maps, 2880-byte scans of 360 beams; 8 / 4 / 2 for what does not: 181 beams, 12- and 20-byte vector states) and
// one lane owns chunk c of EVERY slot of its robot.  It loads slots j+1 .. j+8 (and the new frame) before it stores slots j .. j+7,
// so a depth of up to 9 is one memory round trip, the cap of 16 two.  Nothing depends on the step number: no ring head.
//
// Algorithmic bytes per robot and push: K * F read and K * F written per field of depth K >= 2.  Fields of depth 1 alias the
// imgenv_out array and never reach this kernel.
#pragma once
#include <stdint.h>

#include "field_rows.h"
#include "launch_plan.h"  // STACK_BLOCK, STACK_MAX_BLOCKS
#include "tail_rows.h"

#define STACK_MAX_DEPTH 16   // documented cap (include/imgenv.h: IMGENV_STACK_MAX_DEPTH)
#define STACK_BATCH 8        // slots a lane keeps in registers at once

struct StackField {
    unsigned char* stack;        // [RL][depth][frame_bytes]
    const unsigned char* frame;  // [RL][frame_bytes]: the field's imgenv_out array in the working arena
    uint32_t frame_bytes;
    uint32_t unit;               // 16 | 8 | 4 | 2: plan_final_field's, never 1 (both bases are 256-byte aligned)
    uint32_t chunks;             // frame_bytes / unit
    int32_t depth;               // >= 2
};

struct StackDev {
    StackField f[3];
    int32_t n_fields;            // fields of depth >= 2
    uint32_t chunks_per_robot;   // sum of f[].chunks
    TailRows rows;               // the robots of this launch (restart: those of the reset chain's worlds)
};

// chunk `c` of robot row `row` of one field (the field's members by value: they stay in scalar registers)
template <typename T, bool RESTART>
__device__ __forceinline__ void stack_chunk(unsigned char* stack, const unsigned char* frame, uint32_t chunks, int K, size_t row, uint32_t c) {
    const size_t per_slot = chunks;
    T* s = (T*)stack + row * (size_t)K * per_slot + c;
    const T fresh = ((const T*)frame)[row * per_slot + c];
    if (RESTART) {
        const T z = T();  // all-zero bytes
        for (int j = 0; j < K - 1; j++) s[(size_t)j * per_slot] = z;
        s[(size_t)(K - 1) * per_slot] = fresh;
        return;
    }
    for (int j0 = 0; j0 < K - 1; j0 += STACK_BATCH) {
        T v[STACK_BATCH];
#pragma unroll
        for (int i = 0; i < STACK_BATCH; i++) {
            v[i] = T();
            if (j0 + i + 1 < K) v[i] = s[(size_t)(j0 + i + 1) * per_slot];
        }
#pragma unroll
        for (int i = 0; i < STACK_BATCH; i++)
            if (j0 + i + 1 < K) s[(size_t)(j0 + i) * per_slot] = v[i];
    }
    s[(size_t)(K - 1) * per_slot] = fresh;
}

template <bool RESTART>
__global__ __launch_bounds__(STACK_BLOCK) void k_stack(const StackDev sd) {
    // robots of this launch (tail_rows.h; blocks stride over whatever the count turns out to be)
    const bool listed = RESTART && sd.rows.list != nullptr;
    const size_t total = tail_rows_count(sd.rows, listed) * sd.chunks_per_robot, stride = (size_t)gridDim.x * STACK_BLOCK;
    for (size_t t = (size_t)blockIdx.x * STACK_BLOCK + threadIdx.x; t < total; t += stride) {
        const size_t m = t / sd.chunks_per_robot;
        uint32_t c = (uint32_t)(t - m * sd.chunks_per_robot);
        const size_t row = tail_rows_row(sd.rows, listed, m);
        const StackField f = field_walk(sd.f, sd.n_fields, c);
        field_dispatch<2>(f.unit, [&](auto chunk) {
            stack_chunk<typename decltype(chunk)::type, RESTART>(f.stack, f.frame, f.chunks, f.depth, row, c);
        });
    }
}
