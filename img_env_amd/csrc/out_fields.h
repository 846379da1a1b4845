// out_fields.h -- the arrays of the output arena: which they are, in what order they lie, how long each one is and where imgenv_out
// keeps its pointer.  Host code, nothing of HIP: plain C++17, compiled by g++ for tests/host/create_plan_check.cpp.
//
// ONE list, in the arena's order (which is not imgenv_out's: paper_rewards came late).  The layout (plan_arena), the pointers of
// imgenv_out, their mirror in DevWorld, FULL_REWRITE's shifted copy, the guarded spans with their names and imgenv_arena_bytes all
// expand it: an array added here is added everywhere.
#pragma once
#include <stddef.h>

#include "../../include/imgenv.h"
#include "launch_plan.h"  // Carve

// what the sizes read of a handle
struct OutFacts {
    size_t R;        // local robots
    size_t SD;       // state_dim
    size_t NC;       // view cells
    size_t NI;       // sensor_map pixels
    size_t B;        // beams, at least 1
    size_t PV;       // 1 + ped_vec_dim * max_ped
    size_t NP;       // ped image cells
    size_t P;        // pedestrians, at least 1
    size_t NR;       // robots of every rank (the records are all-gathered in place)
    bool extras;     // IMGENV_FLAG_AGENT_STATE_EXTRAS: the sizes of hits_x, hits_y, angular_map ...
    bool has_beams;  // ... which exist only where there are beams as well
};
inline OutFacts out_facts(const imgenv_cfg& c, int view_h, int view_w, int beams, int RL) {
    OutFacts s;
    s.R = (size_t)RL;
    s.SD = (size_t)c.state_dim;
    s.NC = (size_t)view_h * view_w;
    s.NI = (size_t)c.image_size[0] * (size_t)c.image_size[1];
    s.B = (size_t)(beams > 0 ? beams : 1);
    s.PV = 1 + (size_t)c.ped_vec_dim * c.max_ped;
    s.NP = (size_t)c.ped_image_size[0] * c.ped_image_size[1];
    s.P = (size_t)(c.n_peds > 0 ? c.n_peds : 1);
    s.NR = (size_t)c.n_robots;
    s.extras = (c.flags & IMGENV_FLAG_AGENT_STATE_EXTRAS) != 0;
    s.has_beams = beams > 0;
    return s;
}

// OUT(name, bytes): an array imgenv_out has a pointer to, always.  OUT_EXTRA(name, bytes): one that exists only with
// IMGENV_FLAG_AGENT_STATE_EXTRAS and beams > 0 (null otherwise; its slot stays).  OUT_HIDDEN(name, bytes): no pointer in
// imgenv_out and no guard -- the records, which a shard's caller all-gathers in place (imgenv_records).  `s` is an OutFacts.
#define OUT_FIELDS(OUT, OUT_EXTRA, OUT_HIDDEN)                  \
    OUT(vector_states, s.R * s.SD * 4)                          \
    OUT(view_maps, s.R * s.NC)                                  \
    OUT(sensor_maps, s.R * s.NI * 2) /* [image_h][image_w] f16 */ \
    OUT(lasers_raw, s.R * s.B * 4)                              \
    OUT(lasers, s.R * s.B * 8)                                  \
    OUT(ped_vector_states, s.R * s.PV * 4)                      \
    OUT(ped_maps, s.R * 3 * s.NP * 4)                           \
    OUT(is_collisions, s.R)                                     \
    OUT(is_arrives, s.R)                                        \
    OUT(step_ds, s.R * 8)                                       \
    OUT(ped_min_dists, s.R * 8)                                 \
    OUT(base_rewards, s.R * 4)                                  \
    OUT(base_dones, s.R)                                        \
    OUT(rewards, s.R * 8)                                       \
    OUT(dones, s.R)                                             \
    OUT(dones_info, s.R * 4)                                    \
    OUT(is_clean, s.R)                                          \
    OUT(robot_pose, s.R * 24)                                   \
    OUT(ped_state, s.P * 32)                                    \
    OUT(counters, 16)                                           \
    OUT_HIDDEN(records, s.NR * IMGENV_RECORD_DOUBLES * 8)       \
    OUT(paper_rewards, s.R * 8)                                 \
    OUT(step_rewards, s.R * 8)                                  \
    OUT(step_dones, s.R)                                        \
    OUT(step_dones_info, s.R * 4)                               \
    OUT(step_is_clean, s.R)                                     \
    OUT(step_is_arrives, s.R)                                   \
    OUT(step_is_collisions, s.R)                                \
    OUT(step_all_down, s.R)                                     \
    OUT_EXTRA(hits_x, s.extras ? s.R * s.B * 4 : 0)             \
    OUT_EXTRA(hits_y, s.extras ? s.R * s.B * 4 : 0)             \
    OUT_EXTRA(angular_map, s.extras ? s.R * IMGENV_ANGULAR_BINS * 4 : 0)

#define OUT_FIELD_ID_(name, bytes) OUTF_##name,
enum OutFieldId { OUT_FIELDS(OUT_FIELD_ID_, OUT_FIELD_ID_, OUT_FIELD_ID_) OUTF_COUNT };
#undef OUT_FIELD_ID_

struct OutFieldRow {
    const char* name;
    size_t bytes;
    bool guarded;  // IMGENV_FLAG_CHECK_OUTPUTS watches it (where it exists)
    bool extra;    // exists only with IMGENV_FLAG_AGENT_STATE_EXTRAS and beams > 0
};
inline void out_field_rows(const OutFacts& s, OutFieldRow (&f)[OUTF_COUNT]) {
#define OUT_ROW_(name, bytes) f[OUTF_##name] = {#name, (size_t)(bytes), true, false};
#define OUT_ROW_EXTRA_(name, bytes) f[OUTF_##name] = {#name, (size_t)(bytes), true, true};
#define OUT_ROW_HIDDEN_(name, bytes) f[OUTF_##name] = {#name, (size_t)(bytes), false, false};
    OUT_FIELDS(OUT_ROW_, OUT_ROW_EXTRA_, OUT_ROW_HIDDEN_)
#undef OUT_ROW_
#undef OUT_ROW_EXTRA_
#undef OUT_ROW_HIDDEN_
}
inline bool out_field_exists(const OutFacts& s, const OutFieldRow& f) { return !f.extra || (s.extras && s.has_beams); }

// the arena: every array on a 256-byte boundary, an empty one still takes one slot (so no two arrays share an address)
struct ArenaLayout {
    size_t off[OUTF_COUNT], total;
    size_t slot(int q) const { return (q + 1 < OUTF_COUNT ? off[q + 1] : total) - off[q]; }  // the array and its padding
};
inline ArenaLayout plan_arena(const OutFacts& s) {
    OutFieldRow f[OUTF_COUNT];
    out_field_rows(s, f);
    ArenaLayout l;
    Carve c;
    for (int q = 0; q < OUTF_COUNT; q++) l.off[q] = c.take(f[q].bytes ? f[q].bytes : 1);
    l.total = c.total;
    return l;
}
