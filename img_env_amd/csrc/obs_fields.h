// obs_fields.h -- the observation fields a feature can copy rows of (final observations, rollout storage, rollout minibatches):
// which they are, where a handle keeps each one and how long its row is.  Host code, nothing of HIP: plain C++17, compiled by g++
// for tests/host/field_rows_check.cpp.
//
// A feature keeps only its own ordered list of (bit of its cfg, field, where its out struct keeps the copy's pointer); the order
// decides the layout of its block.  obs_fields fills the catalogue from plain facts about the handle, obs_fields_select picks a
// list's fields.
#pragma once
#include <stddef.h>

#include "../../include/imgenv.h"

enum ObsFieldId {
    // the fields of imgenv_out
    OBSF_VECTOR_STATES, OBSF_SENSOR_MAPS, OBSF_LASERS, OBSF_PED_VECTOR_STATES, OBSF_PED_MAPS, OBSF_IS_COLLISIONS, OBSF_IS_ARRIVES,
    OBSF_STEP_DS, OBSF_PED_MIN_DISTS, OBSF_VIEW_MAPS, OBSF_LASERS_RAW,
    // what a handle has only once a feature is on (obs_fields_select: skipped where it is not)
    OBSF_STACK_SENSOR_MAPS, OBSF_STACK_VECTOR_STATES, OBSF_STACK_LASERS,  // imgenv_stack_enable
    OBSF_PED_VECTOR_NORM,                                                 // imgenv_obs_post_enable
    OBSF_NORM_VECTOR_STATES, OBSF_NORM_STATE_STACK,                       // imgenv_normalise_enable
    OBSF_COUNT,
    OBSF_FIRST_OPTIONAL = OBSF_STACK_SENSOR_MAPS
};

struct ObsFacts {
    imgenv_out out;                        // the working arena's: the dimensions and the eleven arrays
    int ped_image_size[2];                 // imgenv_cfg's
    imgenv_stack_out stack;                // all zero before imgenv_stack_enable
    const void* ped_vector_norm;           // obs_post.h's, or null
    const void* norm_vector_states;        // normalise.h's, or null ...
    const void* norm_state_stack;
    int norm_K;                            // ... and the depth of its stack
};

struct ObsField {
    const void* src;   // [RL][row_bytes], null where the handle has no such array
    size_t row_bytes;
};

inline void obs_fields(const ObsFacts& a, ObsField (&f)[OBSF_COUNT]) {
    const imgenv_out& w = a.out;
    const imgenv_stack_out& so = a.stack;
    const size_t NC = (size_t)w.view_h * w.view_w, NI = (size_t)w.image_h * w.image_w, B = (size_t)(w.n_beams > 0 ? w.n_beams : 0);
    const size_t NP = (size_t)a.ped_image_size[0] * a.ped_image_size[1], D = (size_t)w.state_dim, PV = (size_t)w.ped_vec_len;
    // (a stack of depth >= 2 is the library's or the caller's arena, never an alias of imgenv_out; one of depth 1 is the field itself)
    const auto deep = [](int depth, const void* p) { return depth >= 2 ? p : nullptr; };
    const auto depth = [](int d) { return (size_t)(d > 0 ? d : 0); };
    f[OBSF_VECTOR_STATES] = {w.vector_states, D * 4};
    f[OBSF_SENSOR_MAPS] = {w.sensor_maps, NI * 2};
    f[OBSF_LASERS] = {w.lasers, B * 8};
    f[OBSF_PED_VECTOR_STATES] = {w.ped_vector_states, PV * 4};
    f[OBSF_PED_MAPS] = {w.ped_maps, 3 * NP * 4};
    f[OBSF_IS_COLLISIONS] = {w.is_collisions, 1};
    f[OBSF_IS_ARRIVES] = {w.is_arrives, 1};
    f[OBSF_STEP_DS] = {w.step_ds, 8};
    f[OBSF_PED_MIN_DISTS] = {w.ped_min_dists, 8};
    f[OBSF_VIEW_MAPS] = {w.view_maps, NC};
    f[OBSF_LASERS_RAW] = {w.lasers_raw, B * 4};
    f[OBSF_STACK_SENSOR_MAPS] = {deep(so.image_depth, so.sensor_maps), depth(so.image_depth) * NI * 2};
    f[OBSF_STACK_VECTOR_STATES] = {deep(so.state_depth, so.vector_states), depth(so.state_depth) * D * 4};
    f[OBSF_STACK_LASERS] = {deep(so.laser_depth, so.lasers), depth(so.laser_depth) * B * 8};
    f[OBSF_PED_VECTOR_NORM] = {a.ped_vector_norm, PV * 4};
    f[OBSF_NORM_VECTOR_STATES] = {a.norm_vector_states, D * 4};
    f[OBSF_NORM_STATE_STACK] = {a.norm_state_stack, depth(a.norm_K) * D * 4};
}

// the entries of `list` (any struct with `bit` and `id`) whose bit is in `want`, in the list's order, into sel[]; their count.
// An optional field the handle lacks is skipped silently; any other field without an array or of no bytes is refused: -1, and
// *bad_bit is the bit that named it.
template <typename L, int N>
inline int obs_fields_select(const ObsField (&f)[OBSF_COUNT], const L (&list)[N], int want, const L* (&sel)[N], int* bad_bit) {
    int n = 0;
    for (const L& s : list) {
        const ObsField& of = f[s.id];
        if (!(want & s.bit) || (s.id >= OBSF_FIRST_OPTIONAL && !of.src)) continue;
        if (!of.src || of.row_bytes == 0) {
            *bad_bit = s.bit;
            return -1;
        }
        sel[n++] = &s;
    }
    return n;
}
