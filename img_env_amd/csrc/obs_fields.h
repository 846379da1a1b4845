// obs_fields.h -- the observation fields a feature can copy rows of (final observations, rollout storage, rollout minibatches):
// which they are, where a handle keeps each one and how long its row is.  Host code, nothing of HIP: plain C++17, compiled by g++
// for tests/host/field_rows_check.cpp and tests/host/feature_plan_check.cpp.
//
// The slot catalogue (OBS_SLOTS) says, per field, which bit of a feature's cfg names it and where the feature's out struct keeps
// the copy's pointer; a feature keeps only the order of its block.  obs_fields fills a handle's catalogue of arrays from plain
// facts about it, obs_fields_select picks a list's fields (feature_plan.h: select_feature_fields).
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
    OBSF_FIRST_OPTIONAL = OBSF_STACK_SENSOR_MAPS,
    // behind the fields a handle has arrays of (an ObsField catalogue has OBSF_COUNT entries), the slots no array stands behind:
    // ped_maps drawn from the ring's ped_vector_states (ped_draw.h) -- a minibatch field only
    OBSF_PED_MAPS_DRAWN = OBSF_COUNT,
    OBSF_SLOT_COUNT
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

// ---------------------------------------------------------------------------------------- the slot catalogue
// One row per field: the bit that names it in imgenv_final_obs_cfg and in imgenv_rollout_cfg / imgenv_minibatch_cfg (0: the feature
// has no such field), and where each feature hands the copy's pointer out, as a byte offset into imgenv_final_obs_out,
// imgenv_rollout_out (ring and final list) and imgenv_minibatch_buffer.  `norm`: the field is normalise.h's, and every one of its
// slots is a member of imgenv_normalise_out instead (those structs keep their layout); its minibatch slot is entry 0 of an array
// with one entry per buffer.  A drawn field (the ids from OBSF_COUNT on) has a minibatch slot alone: no feature stores it, the
// minibatches draw it from the ring of field `from` into the buffer member of the field it stands for; how long its row is the
// caller says (obs_fields_with_drawn).
#define OBS_NO_SLOT ((size_t)-1)
struct ObsSlot {
    int final_bit, rollout_bit;
    size_t final_out, ring_out, fin_out, mb_out;
    bool norm;
    int from;  // a drawn field's source field; -1 for every other
    size_t seq_out;  // imgenv_seq_buffer's member (sequences.h), the normalised fields' too: that struct holds them itself
};
#define OBS_SLOT_FINAL_ONLY(bit, member) {bit, 0, offsetof(imgenv_final_obs_out, member), OBS_NO_SLOT, OBS_NO_SLOT, OBS_NO_SLOT, false, -1, OBS_NO_SLOT}
#define OBS_SLOT_DRAWN(rbit, member, from_id) \
    {0, rbit, OBS_NO_SLOT, OBS_NO_SLOT, OBS_NO_SLOT, offsetof(imgenv_minibatch_buffer, mb_##member), false, from_id, \
     offsetof(imgenv_seq_buffer, mb_##member)}
#define OBS_SLOT_ALL(fbit, rbit, member)                                                                                       \
    {fbit, rbit, offsetof(imgenv_final_obs_out, member), offsetof(imgenv_rollout_out, obs_##member),                           \
     offsetof(imgenv_rollout_out, final_##member), offsetof(imgenv_minibatch_buffer, mb_##member), false, -1,                  \
     offsetof(imgenv_seq_buffer, mb_##member)}
#define OBS_SLOT_NORM(member)                                                                                                  \
    {IMGENV_FINAL_NORM_STATES, IMGENV_ROLLOUT_NORM_STATES, offsetof(imgenv_normalise_out, final_##member),                     \
     offsetof(imgenv_normalise_out, rollout_obs_##member), offsetof(imgenv_normalise_out, rollout_final_##member),             \
     offsetof(imgenv_normalise_out, mb_##member), true, -1, offsetof(imgenv_seq_buffer, mb_##member)}
static const ObsSlot OBS_SLOTS[OBSF_SLOT_COUNT] = {
    OBS_SLOT_ALL(IMGENV_FINAL_VECTOR_STATES, IMGENV_ROLLOUT_VECTOR_STATES, vector_states),
    OBS_SLOT_ALL(IMGENV_FINAL_SENSOR_MAPS, IMGENV_ROLLOUT_SENSOR_MAPS, sensor_maps),
    OBS_SLOT_ALL(IMGENV_FINAL_LASERS, IMGENV_ROLLOUT_LASERS, lasers),
    OBS_SLOT_ALL(IMGENV_FINAL_PED_VECTOR_STATES, IMGENV_ROLLOUT_PED_VECTOR_STATES, ped_vector_states),
    OBS_SLOT_ALL(IMGENV_FINAL_PED_MAPS, IMGENV_ROLLOUT_PED_MAPS, ped_maps),
    OBS_SLOT_FINAL_ONLY(IMGENV_FINAL_IS_COLLISIONS, is_collisions),
    OBS_SLOT_FINAL_ONLY(IMGENV_FINAL_IS_ARRIVES, is_arrives),
    OBS_SLOT_FINAL_ONLY(IMGENV_FINAL_STEP_DS, step_ds),
    OBS_SLOT_FINAL_ONLY(IMGENV_FINAL_PED_MIN_DISTS, ped_min_dists),
    OBS_SLOT_FINAL_ONLY(IMGENV_FINAL_VIEW_MAPS, view_maps),
    OBS_SLOT_FINAL_ONLY(IMGENV_FINAL_LASERS_RAW, lasers_raw),
    OBS_SLOT_ALL(IMGENV_FINAL_STACKS, IMGENV_ROLLOUT_STACKS, stack_sensor_maps),
    OBS_SLOT_ALL(IMGENV_FINAL_STACKS, IMGENV_ROLLOUT_STACKS, stack_vector_states),
    OBS_SLOT_ALL(IMGENV_FINAL_STACKS, IMGENV_ROLLOUT_STACKS, stack_lasers),
    OBS_SLOT_ALL(IMGENV_FINAL_PED_NORM, IMGENV_ROLLOUT_PED_NORM, ped_vector_norm),
    OBS_SLOT_NORM(norm_vector_states),
    OBS_SLOT_NORM(norm_state_stack),
    OBS_SLOT_DRAWN(IMGENV_ROLLOUT_PED_MAPS_DRAWN, ped_maps, OBSF_PED_VECTOR_STATES),
};
// A feature keeps only the order of its block.  The final observations: the enum's.  The rollout and the minibatches: sensor_maps
// in front of vector_states, ped_vector_norm in front of the stacks (the order of the blocks already handed out: it must not change).
// The minibatches: the rollout's, with the drawn ped_maps where the stored ones stand (the rollout excludes one of the two, so a
// selection still has ROLLOUT_TABLE_FIELDS entries at most).
static const int FINAL_FIELD_ORDER[] = {
    OBSF_VECTOR_STATES, OBSF_SENSOR_MAPS, OBSF_LASERS, OBSF_PED_VECTOR_STATES, OBSF_PED_MAPS, OBSF_IS_COLLISIONS, OBSF_IS_ARRIVES,
    OBSF_STEP_DS, OBSF_PED_MIN_DISTS, OBSF_VIEW_MAPS, OBSF_LASERS_RAW, OBSF_STACK_SENSOR_MAPS, OBSF_STACK_VECTOR_STATES,
    OBSF_STACK_LASERS, OBSF_PED_VECTOR_NORM, OBSF_NORM_VECTOR_STATES, OBSF_NORM_STATE_STACK};
static const int ROLLOUT_FIELD_ORDER[] = {
    OBSF_SENSOR_MAPS, OBSF_VECTOR_STATES, OBSF_LASERS, OBSF_PED_VECTOR_STATES, OBSF_PED_MAPS, OBSF_PED_VECTOR_NORM,
    OBSF_STACK_SENSOR_MAPS, OBSF_STACK_VECTOR_STATES, OBSF_STACK_LASERS, OBSF_NORM_VECTOR_STATES, OBSF_NORM_STATE_STACK};
static const int MINIBATCH_FIELD_ORDER[] = {
    OBSF_SENSOR_MAPS, OBSF_VECTOR_STATES, OBSF_LASERS, OBSF_PED_VECTOR_STATES, OBSF_PED_MAPS, OBSF_PED_MAPS_DRAWN, OBSF_PED_VECTOR_NORM,
    OBSF_STACK_SENSOR_MAPS, OBSF_STACK_VECTOR_STATES, OBSF_STACK_LASERS, OBSF_NORM_VECTOR_STATES, OBSF_NORM_STATE_STACK};
// the pointer a slot receives: member `off` (the slot's final_out, ring_out or fin_out) of `own`, the feature's out struct -- of
// `norm_out` for a normalised field
inline void obs_slot_put(const ObsSlot& s, size_t off, void* own, imgenv_normalise_out* norm_out, void* p) {
    *(void**)((unsigned char*)(s.norm ? (void*)norm_out : own) + off) = p;
}
// likewise for minibatch buffer `b`: the slot's mb_out member of `buf` (that buffer's struct), or entry b of norm_out's array
inline void obs_slot_put_mb(const ObsSlot& s, imgenv_minibatch_buffer* buf, imgenv_normalise_out* norm_out, int b, void* p) {
    obs_slot_put(s, s.mb_out + (s.norm ? (size_t)b * sizeof(void*) : 0), buf, norm_out, p);
}

// likewise for a sequence buffer (sequences.h): always a member of `buf` itself
inline void obs_slot_put_seq(const ObsSlot& s, imgenv_seq_buffer* buf, void* p) { *(void**)((unsigned char*)buf + s.seq_out) = p; }

// a catalogue with the drawn fields behind it: a drawn field is there where its source is, with a row of `drawn_row_bytes` (the one
// drawn field there is: a pedestrian map, feature_plan.h's ped_maps_row_bytes)
inline void obs_fields_with_drawn(const ObsField (&f)[OBSF_COUNT], size_t drawn_row_bytes, ObsField (&ext)[OBSF_SLOT_COUNT]) {
    for (int k = 0; k < OBSF_COUNT; k++) ext[k] = f[k];
    for (int k = OBSF_COUNT; k < OBSF_SLOT_COUNT; k++) {
        const ObsSlot& s = OBS_SLOTS[k];
        ext[k] = f[s.from].src ? ObsField{f[s.from].src, drawn_row_bytes} : ObsField{nullptr, 0};
    }
}

// the entries of `list` (any struct with `bit` and `id`) whose bit is in `want`, in the list's order, into sel[]; their count.
// An optional field the handle lacks is skipped silently; any other field without an array or of no bytes is refused: -1, and
// *bad_bit is the bit that named it.
template <typename L, int NF>
inline int obs_fields_select_n(const ObsField (&f)[NF], const L* list, int n_list, int want, const L** sel, int* bad_bit) {
    int n = 0;
    for (int q = 0; q < n_list; q++) {
        const L& s = list[q];
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
template <typename L, int N>
inline int obs_fields_select(const ObsField (&f)[OBSF_COUNT], const L (&list)[N], int want, const L* (&sel)[N], int* bad_bit) {
    return obs_fields_select_n(f, list, N, want, sel, bad_bit);
}
