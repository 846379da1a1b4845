// field_rows.h -- what the row-copy kernels share (k_stack, k_final_obs, k_rollout, k_rollout_gather), for the kernels and, as plain
// C++, for tests/host/field_rows_check.cpp.
//
// Each of them copies rows of several fields in one launch.  A row of a field is cut into chunks of `unit` bytes (launch_plan.h:
// plan_final_field is the one rule: the largest of 16 / 8 / 4 / 2 / 1 that divides the row's size); one lane owns one chunk, and a
// lane's chunk number c runs over the chunks of all fields of a row, field after field.  The kernel's argument holds a table
// F f[N] of the fields -- any struct with a `chunks` member -- of which the first n_fields are in use.
//
//   field_walk      from c to the field it falls into and the chunk number within that field
//   field_dispatch  from the field's unit to the caller's per-chunk operation, instantiated for the chunk type
#pragma once
#include <stdint.h>

#include "tail_rows.h"  // TAIL_HD

#if defined(__HIPCC__)
// (vector types: a struct of four words held across the second load was given a private array, which the compiler put into LDS)
typedef uint4 FieldChunk16;
typedef uint2 FieldChunk8;
#else
struct alignas(16) FieldChunk16 {
    uint32_t v[4];
};
struct alignas(8) FieldChunk8 {
    uint32_t v[2];
};
#endif

// while chunk `c` lies behind the field in hand, step to the next one, from field K on.  Every index into the table is a
// compile-time constant and `cur` is a local the compiler takes apart: the copy is a select per member on scalar kernel arguments,
// no per-lane indexed copy of the struct and no scratch.
template <int K, typename F, int N>
TAIL_HD void field_walk_from(const F (&f)[N], int n_fields, uint32_t& c, F& cur) {
    if constexpr (K < N) {
        if (K < n_fields && c >= cur.chunks) {
            c -= cur.chunks;
            cur = f[K];
            field_walk_from<K + 1>(f, n_fields, c, cur);
        }
    }
}
// the field chunk `c` of a row falls into, by value; `c` becomes the chunk number within it.  (A c past the row's last chunk stays
// in the last field in use.)
template <typename F, int N>
TAIL_HD F field_walk(const F (&f)[N], int n_fields, uint32_t& c) {
    F cur = f[0];
    field_walk_from<1>(f, n_fields, c, cur);
    return cur;
}

template <typename T>
struct FieldChunkType {
    typedef T type;
};
// op(FieldChunkType<T>()) for the chunk type T of `unit` bytes.  MIN_UNIT is the smallest unit the caller's tables can hold: 2
// (k_stack: a frame is never odd) leaves the one-byte instantiation out.
template <int MIN_UNIT = 1, typename Op>
TAIL_HD void field_dispatch(uint32_t unit, Op&& op) {
    switch (unit) {
        case 16: op(FieldChunkType<FieldChunk16>()); break;
        case 8: op(FieldChunkType<FieldChunk8>()); break;
        case 4: op(FieldChunkType<uint32_t>()); break;
        default:
            if (MIN_UNIT >= 2 || unit == 2)
                op(FieldChunkType<uint16_t>());
            else if constexpr (MIN_UNIT < 2)
                op(FieldChunkType<uint8_t>());
            break;
    }
}
