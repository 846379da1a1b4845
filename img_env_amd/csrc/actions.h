// actions.h -- VelActionWrapper.action (envs/wrapper/base.py:37-66, envs/action/action.py:8-38) and the `speeds` that
// MultiRobotCleanWrapper masks (base.py:58, 81-83) for every local robot of a handle: what a policy emits -- one index into the
// YAML's discrete_actions per robot, or a row of raw floats -- becomes the float32 (v, w, beep) row that the step entry points take.
//
// One kernel, k_actions<DTYPE, MODE>, one launch per imgenv_actions_decode on the caller's stream, in front of the step that
// consumes the handle-owned `actions` (the move is the next launch on that stream, and every later reader is ordered behind it):
//   TABLE, integer raw [R]           actions[r] = table[raw[r]] (a two-column row of the YAML has beep 0: action.py:29-30);
//                                    an index outside [0, n_table) gives (0, 0, 0) and is counted, never read
//   TABLE, float raw [R][n_cols]     ContinuousAction(*x) (base.py:43): rounded to float32, not clipped, beep 0 with two columns
//   CLIP,  float raw [R][n_cols]     column i: x = float32(raw); x = x >= lo_i ? x : lo_i; x = x <= hi_i ? x : hi_i
//                                    (np.clip per component, base.py:47-51; rounding to float32 is monotone, so clipping the rounded
//                                    value by the rounded bounds is the reference's clip in double put on the float32 wire)
//   a row with a component that is not finite, as it came or once it is float32: (0, 0, 0), counted -- the reference would carry
//                                    it into the node; here cell indices are rounded poses, so it must not arrive
//   speeds[r] = (v, w) of the decoded row where clean_state[r] is set, (0, 0) where not: clean_state (world.h) is
//                                    MultiRobotCleanWrapper.is_clean as the last chain's tail_group left it, 1 after a reset --
//                                    the is_clean of BEFORE the step, which is what base.py:81-83 masks with
//   n_bad                            += the bad rows: one atomicAdd per wavefront that saw any (ballot + popcount)
//
// One lane per robot, blocks of ACT_BLOCK, no LDS: the table (at most 4096 rows of 12 bytes) is read from device memory, where a
// wavefront's 64 lookups hit a handful of cache lines.  The launch is latency, not bytes: per robot 4-24 bytes in, 20 out.
// Only compares, conversions and selects: every result is exact, tests/action_model.py gives the same bits.
#pragma once
#include <stdint.h>

#include "launch_plan.h"  // ACT_BLOCK

struct ActionsDev {
    const void* raw;             // [RL] indices or [RL][n_cols] floats, the caller's
    const float* table;          // [n_table][3] (TABLE mode)
    float* actions;              // [RL][3]
    float* speeds;               // [RL][2]
    int32_t* n_bad;              // [1]
    const uint8_t* clean_state;  // [RL] (world.h)
    float lo[3], hi[3];          // CLIP mode: the bounds of the first n_cols columns
    int32_t n_table, n_cols, RL;
};

template <int DTYPE>
struct ActRaw;
template <>
struct ActRaw<IMGENV_RAW_I32> { typedef int32_t type; };
template <>
struct ActRaw<IMGENV_RAW_I64> { typedef int64_t type; };
template <>
struct ActRaw<IMGENV_RAW_F32> { typedef float type; };
template <>
struct ActRaw<IMGENV_RAW_F64> { typedef double type; };

template <int DTYPE, int MODE>
__global__ __launch_bounds__(ACT_BLOCK) void k_actions(const ActionsDev a) {
    typedef typename ActRaw<DTYPE>::type T;
    constexpr bool integer = DTYPE == IMGENV_RAW_I32 || DTYPE == IMGENV_RAW_I64;
    static_assert(!(integer && MODE == IMGENV_ACTIONS_CLIP), "indices are not clipped");
    const int r = (int)(blockIdx.x * ACT_BLOCK + threadIdx.x);
    const bool live = r < a.RL;
    bool bad = false;
    if (live) {
        float v = 0.0f, w = 0.0f, beep = 0.0f;
        if constexpr (integer) {
            const long long k = (long long)((const T*)a.raw)[r];
            bad = k < 0 || k >= (long long)a.n_table;
            if (!bad) {
                const float* row = a.table + (size_t)k * 3;
                v = row[0]; w = row[1]; beep = row[2];
            }
        } else {
            const T* x = (const T*)a.raw + (size_t)r * a.n_cols;
            float y[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int i = 0; i < 3; i++) {
                if (i < a.n_cols) {
                    const T xi = x[i];
                    float f = (float)xi;  // (float64: round to nearest even, the float32 wire)
                    bad = bad || !isfinite(xi);
                    if (MODE == IMGENV_ACTIONS_CLIP) {
                        f = f >= a.lo[i] ? f : a.lo[i];
                        f = f <= a.hi[i] ? f : a.hi[i];
                    }
                    bad = bad || !isfinite(f);  // (a finite double beyond float32 that nothing clipped)
                    y[i] = f;
                }
            }
            v = y[0]; w = y[1]; beep = y[2];
        }
        if (bad) v = w = beep = 0.0f;
        float* out = a.actions + (size_t)r * 3;
        out[0] = v; out[1] = w; out[2] = beep;
        const bool clean = a.clean_state[r] != 0;
        a.speeds[(size_t)r * 2] = clean ? v : 0.0f;
        a.speeds[(size_t)r * 2 + 1] = clean ? w : 0.0f;
    }
    // (every lane of the wavefront is here: nothing above returns)
    const unsigned long long seen = __ballot(bad);
    if (seen != 0 && (threadIdx.x & (WAVE - 1)) == 0) atomicAdd(a.n_bad, (int)__popcll(seen));
}
