// feature_plan.h -- what an enable call of an optional feature (imgenv_*_enable, include/imgenv.h) decides before it touches a
// device: the refusals of its cfg, the answer to a repeated call, the refusals that depend on what else the handle has enabled,
// and, for the row-copy features, which fields it selects (the slot catalogue is obs_fields.h's).  Host code, nothing of HIP:
// plain C++17, compiled by g++ for tests/host/feature_plan_check.cpp.  Nothing here writes the handle.
//
// One function per feature, X_enable_plan, makes the decisions in the one order every enable follows:
//     the cfg and out structs' sizes -> the cfg's own refusals -> the null handle -> the repeated call -> the facts' refusals
// `f` is what feature_facts(h) of imgenv_hip.hip read of the handle, nullptr for a null handle; `stored` is the cfg of the first
// call, looked at only where the feature is on.  A refusal returns its IMGENV_E* code and leaves its text in `msg`; the caller
// hands both on (imgenv_last_error).  ENABLE_REPEAT: the same cfg again, the caller answers with the stored out struct.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <cmath>

#include "../../include/imgenv.h"
#include "launch_plan.h"  // NORM_MAX_COLS, plan_stack
#include "obs_fields.h"

typedef char FeatureMsg[512];
#define FEATURE_REFUSE(code, ...) return snprintf(msg, sizeof(FeatureMsg), __VA_ARGS__), (code)
#define FEATURE_TRY(expr)             \
    do {                              \
        if (int rc_ = (expr)) return rc_; \
    } while (0)
enum { ENABLE_REPEAT = 1 };  // (no IMGENV_E* code is positive)
#define OBS_POST_PLAN_DIM 7  // avg / std entries of imgenv_obs_post_cfg (obs_post.h: OBS_POST_DIM)

// ---------------------------------------------------------------------------------------- what the rules read of a handle
struct FeatureFacts {
    int RL = 0, P = 0, state_dim = 0, ped_vec_dim = 0, n_beams = 0;
    bool keep_view_maps = false;
    bool any_reset = false;      // a world has been reset (imgenv_stack_enable must come before)
    // per feature: whether it is on, and what other features depend on.  No rule here reads act_n_table, act_n_cols, pol_kind,
    // pol_flags, pol_A, pol_C or roll_horizon: they are what a dependent enable of imgenv_hip.hip sizes its block by AFTER its plan
    // has passed (the policy head from the actions and the rollout, the loss from the policy head) -- nothing checks them.
    bool stack_on = false;
    int stack_state_depth = 0;   // imgenv_stack_out.state_depth
    int stack_n_fields = 0;      // stacks deeper than 1
    bool ep_on = false;
    bool eplog_on = false;
    int eplog_capacity = 0;
    bool act_on = false;
    int act_mode = 0, act_n_table = 0, act_n_cols = 0;
    bool pol_on = false;
    int pol_kind = 0, pol_flags = 0, pol_A = 0, pol_C = 0;
    bool ploss_on = false;
    bool post_on = false, post_norm = false;  // obs_post keeps ped_vector_norm (IMGENV_OBS_PED_NORM)
    bool final_on = false;
    bool roll_on = false;
    int roll_horizon = 0, roll_fields = 0;
    bool mb_on = false;
    bool norm_on = false, norm_obs = false, norm_rew = false;  // the arrays of IMGENV_NORM_OBS / IMGENV_NORM_REWARD exist
    int ped_h = 0, ped_w = 0;    // imgenv_cfg.ped_image_size (IMGENV_ROLLOUT_PED_MAPS_DRAWN: the map must fit k_ped_draw's rank plane)
    bool seq_on = false;         // sequences.h
};

// the cfg and the caller's out struct of an enable call, before the handle is looked at.  An out struct says 0 or this library's size.
template <typename Cfg, typename Out>
inline int enable_args(const Cfg* c, const char* cfg_name, const Out* out, const char* out_name, FeatureMsg msg) {
    if (!c) FEATURE_REFUSE(IMGENV_EINVAL, "null argument");
    if (c->struct_size != (int32_t)sizeof(Cfg)) FEATURE_REFUSE(IMGENV_EINVAL, "%s.struct_size %d (this library's is %d)", cfg_name, c->struct_size, (int)sizeof(Cfg));
    if (out && out->struct_size != 0 && out->struct_size != (int32_t)sizeof(Out)) FEATURE_REFUSE(IMGENV_EINVAL, "%s.struct_size", out_name);
    return IMGENV_OK;
}
inline int enable_null_handle(const FeatureFacts* f, FeatureMsg msg) {
    if (!f) FEATURE_REFUSE(IMGENV_EINVAL, "null argument");
    return IMGENV_OK;
}
// an entry point that needs a feature: "<its enable> was not called"
inline int feature_needed(bool on, const char* enable_name, FeatureMsg msg) {
    if (!on) FEATURE_REFUSE(IMGENV_ESTATE, "%s was not called", enable_name);
    return IMGENV_OK;
}

// ---------------------------------------------------------------------------------------- observation stacks
// (unlike the others: the handle in front of the cfg, a second call is refused, and so is one after the first reset; the caller
// may bring the arena)
inline int stack_cfg_refusals(const imgenv_stack_cfg& s, FeatureMsg msg) {
    if (s.image_batch < 0 || s.state_batch < 0) FEATURE_REFUSE(IMGENV_EINVAL, "image_batch / state_batch must be >= 0");
    if (s.image_batch > IMGENV_STACK_MAX_DEPTH || s.state_batch > IMGENV_STACK_MAX_DEPTH || s.laser_batch > IMGENV_STACK_MAX_DEPTH)
        FEATURE_REFUSE(IMGENV_EINVAL, "a stack depth above IMGENV_STACK_MAX_DEPTH (%d)", IMGENV_STACK_MAX_DEPTH);
    return IMGENV_OK;
}
inline int stack_enable_plan(const imgenv_stack_cfg* s, const imgenv_stack_out* out, const FeatureFacts* f, FeatureMsg msg) {
    FEATURE_TRY(enable_null_handle(f, msg));
    FEATURE_TRY(enable_args(s, "imgenv_stack_cfg", out, "imgenv_stack_out", msg));
    if (f->stack_on) FEATURE_REFUSE(IMGENV_ESTATE, "imgenv_stack_enable has already been called on this handle");
    if (f->any_reset) FEATURE_REFUSE(IMGENV_ESTATE, "imgenv_stack_enable after the first reset");
    return stack_cfg_refusals(*s, msg);
}
inline int stack_arena_refusals(const imgenv_stack_cfg& s, size_t total, FeatureMsg msg) {
    if (s.arena_bytes < (int64_t)total) FEATURE_REFUSE(IMGENV_EINVAL, "stack arena too small: %lld < %zu", (long long)s.arena_bytes, total);
    if ((uintptr_t)s.arena & 255) FEATURE_REFUSE(IMGENV_EINVAL, "stack arena must be 256-byte aligned");
    return IMGENV_OK;
}

// ---------------------------------------------------------------------------------------- episode statistics
inline bool episodes_cfg_same(const imgenv_episodes_cfg& c, const imgenv_episodes_cfg& o) { return c.min_steps == o.min_steps && c.dt == o.dt; }
inline int episodes_enable_plan(const imgenv_episodes_cfg* c, const imgenv_episodes_out* out, const FeatureFacts* f, const imgenv_episodes_cfg* stored,
                                FeatureMsg msg) {
    FEATURE_TRY(enable_args(c, "imgenv_episodes_cfg", out, "imgenv_episodes_out", msg));
    if (!(c->dt > 0.0) || !std::isfinite(c->dt)) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_episodes_cfg.dt must be > 0 (the YAML's control_hz)");
    if (c->min_steps < 0) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_episodes_cfg.min_steps must be >= 0");
    FEATURE_TRY(enable_null_handle(f, msg));
    if (!f->ep_on) return IMGENV_OK;
    if (!episodes_cfg_same(*c, *stored))
        FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_episodes_enable: the handle already keeps statistics with min_steps %d, dt %g", stored->min_steps, stored->dt);
    return ENABLE_REPEAT;
}

// ---------------------------------------------------------------------------------------- episode log (needs the episodes)
inline int episode_log_enable_plan(const imgenv_episode_log_cfg* c, const imgenv_episode_log_out* out, const FeatureFacts* f, FeatureMsg msg) {
    FEATURE_TRY(enable_args(c, "imgenv_episode_log_cfg", out, "imgenv_episode_log_out", msg));
    if (c->capacity < 1 || c->capacity > IMGENV_EPLOG_MAX_CAPACITY)
        FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_episode_log_cfg.capacity %d: 1 .. %d", c->capacity, IMGENV_EPLOG_MAX_CAPACITY);
    FEATURE_TRY(enable_null_handle(f, msg));
    if (!f->ep_on) FEATURE_REFUSE(IMGENV_ESTATE, "imgenv_episode_log_enable before imgenv_episodes_enable");
    if (!f->eplog_on) return IMGENV_OK;
    if (c->capacity != f->eplog_capacity)
        FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_episode_log_enable: the handle already keeps a log of capacity %d", f->eplog_capacity);
    return ENABLE_REPEAT;
}

// ---------------------------------------------------------------------------------------- action decoding
// (`stored` keeps no table pointer: `table` is the handle's copy of the rows, and the rows are what is compared)
inline bool actions_cfg_same(const imgenv_actions_cfg& c, const imgenv_actions_cfg& o, const float* table) {
    if (c.mode != o.mode || c.n_cols != o.n_cols) return false;
    if (c.mode == IMGENV_ACTIONS_TABLE) return c.n_table == o.n_table && memcmp(c.table, table, sizeof(float) * 3 * (size_t)c.n_table) == 0;
    return memcmp(c.clip, o.clip, sizeof(float) * 2 * (size_t)c.n_cols) == 0;
}
inline int actions_enable_plan(const imgenv_actions_cfg* c, const imgenv_actions_out* out, const FeatureFacts* f, const imgenv_actions_cfg* stored,
                               const float* stored_table, FeatureMsg msg) {
    FEATURE_TRY(enable_args(c, "imgenv_actions_cfg", out, "imgenv_actions_out", msg));
    if (c->mode != IMGENV_ACTIONS_TABLE && c->mode != IMGENV_ACTIONS_CLIP) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_actions_cfg.mode %d", c->mode);
    if (c->n_cols != 2 && c->n_cols != 3) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_actions_cfg.n_cols %d: 2 (v, w) or 3 (v, w, beep)", c->n_cols);
    if (c->mode == IMGENV_ACTIONS_TABLE) {
        if (!c->table || c->n_table < 1 || c->n_table > IMGENV_ACTIONS_MAX_TABLE)
            FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_actions_cfg.table: 1 .. %d rows (n_table %d)", IMGENV_ACTIONS_MAX_TABLE, c->n_table);
        for (int q = 0; q < 3 * c->n_table; q++)
            if (!std::isfinite(c->table[q])) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_actions_cfg.table row %d holds a value that is not finite", q / 3);
    } else {
        for (int i = 0; i < c->n_cols; i++)
            if (!std::isfinite(c->clip[i][0]) || !std::isfinite(c->clip[i][1]) || c->clip[i][0] > c->clip[i][1])
                FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_actions_cfg.clip[%d] = (%g, %g): finite bounds with lo <= hi", i, c->clip[i][0], c->clip[i][1]);
    }
    FEATURE_TRY(enable_null_handle(f, msg));
    if (!f->act_on) return IMGENV_OK;
    if (!actions_cfg_same(*c, *stored, stored_table)) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_actions_enable: the handle already decodes actions with another cfg");
    return ENABLE_REPEAT;
}

// ---------------------------------------------------------------------------------------- the policy head (needs the actions in
// the matching mode; IMGENV_POLICY_STORE needs the rollout)
inline bool policy_cfg_same(const imgenv_policy_cfg& c, const imgenv_policy_cfg& o) { return c.kind == o.kind && c.flags == o.flags && c.seed == o.seed; }
inline int policy_enable_plan(const imgenv_policy_cfg* c, const imgenv_policy_out* out, const FeatureFacts* f, const imgenv_policy_cfg* stored, FeatureMsg msg) {
    FEATURE_TRY(enable_args(c, "imgenv_policy_cfg", out, "imgenv_policy_out", msg));
    if (c->kind != IMGENV_POLICY_CATEGORICAL && c->kind != IMGENV_POLICY_GAUSSIAN) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_policy_cfg.kind %d", c->kind);
    if (c->flags & ~IMGENV_POLICY_STORE) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_policy_cfg.flags %d", c->flags);
    if (c->reserved != 0) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_policy_cfg.reserved %d", c->reserved);
    FEATURE_TRY(enable_null_handle(f, msg));
    if (f->pol_on) {
        if (!policy_cfg_same(*c, *stored)) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_policy_enable: the handle already has a policy head with another cfg");
        return ENABLE_REPEAT;
    }
    if (!f->act_on) FEATURE_REFUSE(IMGENV_ESTATE, "imgenv_policy_enable before imgenv_actions_enable");
    const bool cat = c->kind == IMGENV_POLICY_CATEGORICAL;
    if (f->act_mode != (cat ? IMGENV_ACTIONS_TABLE : IMGENV_ACTIONS_CLIP))
        FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_policy_enable: a %s head needs imgenv_actions_enable in %s mode", cat ? "categorical" : "Gaussian", cat ? "TABLE" : "CLIP");
    if ((c->flags & IMGENV_POLICY_STORE) && !f->roll_on) FEATURE_REFUSE(IMGENV_ESTATE, "imgenv_policy_enable: IMGENV_POLICY_STORE before imgenv_rollout_enable");
    return IMGENV_OK;
}

// ---------------------------------------------------------------------------------------- PPO's loss (needs the policy head)
inline bool policy_loss_cfg_same(const imgenv_policy_loss_cfg& c, const imgenv_policy_loss_cfg& o) { return c.max_rows == o.max_rows; }
inline int policy_loss_enable_plan(const imgenv_policy_loss_cfg* c, const imgenv_policy_loss_out* out, const FeatureFacts* f,
                                   const imgenv_policy_loss_cfg* stored, FeatureMsg msg) {
    FEATURE_TRY(enable_args(c, "imgenv_policy_loss_cfg", out, "imgenv_policy_loss_out", msg));
    if (c->max_rows < 1) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_policy_loss_cfg.max_rows %d (at least 1)", c->max_rows);
    if (c->reserved[0] != 0 || c->reserved[1] != 0) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_policy_loss_cfg.reserved");
    FEATURE_TRY(enable_null_handle(f, msg));
    if (f->ploss_on) {
        if (!policy_loss_cfg_same(*c, *stored)) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_policy_loss_enable: the handle already has a policy loss with another cfg");
        return ENABLE_REPEAT;
    }
    if (!f->pol_on) FEATURE_REFUSE(IMGENV_ESTATE, "imgenv_policy_loss_enable before imgenv_policy_enable");
    return IMGENV_OK;
}

// ---------------------------------------------------------------------------------------- observation post-processing
// (avg / std count only under IMGENV_OBS_PED_NORM, close_dist only under IMGENV_OBS_CLOSE)
inline bool obs_post_cfg_same(const imgenv_obs_post_cfg& c, const imgenv_obs_post_cfg& o) {
    bool same = c.flags == o.flags;
    if (same && (c.flags & IMGENV_OBS_PED_NORM)) same = memcmp(c.avg, o.avg, sizeof(o.avg)) == 0 && memcmp(c.std, o.std, sizeof(o.std)) == 0;
    if (same && (c.flags & IMGENV_OBS_CLOSE)) same = c.close_dist == o.close_dist;
    return same;
}
inline int obs_post_enable_plan(const imgenv_obs_post_cfg* c, const imgenv_obs_post_out* out, const FeatureFacts* f, const imgenv_obs_post_cfg* stored,
                                FeatureMsg msg) {
    FEATURE_TRY(enable_args(c, "imgenv_obs_post_cfg", out, "imgenv_obs_post_out", msg));
    if (c->flags == 0 || (c->flags & ~(IMGENV_OBS_PED_NORM | IMGENV_OBS_CLOSE))) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_obs_post_cfg.flags %d", c->flags);
    if (c->flags & IMGENV_OBS_PED_NORM)
        for (int k = 0; k < OBS_POST_PLAN_DIM; k++) {
            if (!std::isfinite(c->avg[k]) || !std::isfinite(c->std[k])) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_obs_post_cfg: avg[%d] / std[%d] is not finite", k, k);
            if (c->std[k] == 0.0) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_obs_post_cfg.std[%d] is 0", k);
        }
    if ((c->flags & IMGENV_OBS_CLOSE) && std::isnan(c->close_dist)) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_obs_post_cfg.close_dist is not a number");
    FEATURE_TRY(enable_null_handle(f, msg));
    if (f->post_on) {
        if (!obs_post_cfg_same(*c, *stored)) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_obs_post_enable: the handle already post-processes its observations with another cfg");
        return ENABLE_REPEAT;
    }
    if ((c->flags & IMGENV_OBS_PED_NORM) && f->ped_vec_dim != OBS_POST_PLAN_DIM)
        FEATURE_REFUSE(IMGENV_EINVAL, "IMGENV_OBS_PED_NORM: ped_vec_dim %d (the wrapper's constants are for %d)", f->ped_vec_dim, OBS_POST_PLAN_DIM);
    if ((c->flags & IMGENV_OBS_CLOSE) && f->P == 0) FEATURE_REFUSE(IMGENV_EINVAL, "IMGENV_OBS_CLOSE on a handle without pedestrians");
    return IMGENV_OK;
}

// ---------------------------------------------------------------------------------------- running normalisation
// (any second call is refused; reads the state stack's depth as it is at the enable)
inline int normalise_enable_plan(const imgenv_normalise_cfg* c, const imgenv_normalise_out* out, const FeatureFacts* f, FeatureMsg msg) {
    FEATURE_TRY(enable_args(c, "imgenv_normalise_cfg", out, "imgenv_normalise_out", msg));
    if (c->flags == 0 || (c->flags & ~(IMGENV_NORM_OBS | IMGENV_NORM_REWARD))) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_normalise_cfg.flags %d", c->flags);
    if (!std::isfinite(c->clip_obs) || c->clip_obs <= 0.0) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_normalise_cfg.clip_obs %g: finite and above 0", c->clip_obs);
    if (!std::isfinite(c->clip_reward) || c->clip_reward <= 0.0) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_normalise_cfg.clip_reward %g: finite and above 0", c->clip_reward);
    if (!std::isfinite(c->eps) || c->eps <= 0.0) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_normalise_cfg.eps %g: finite and above 0", c->eps);
    if (!(c->gamma >= 0.0 && c->gamma <= 1.0)) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_normalise_cfg.gamma %g: 0 .. 1", c->gamma);
    FEATURE_TRY(enable_null_handle(f, msg));
    if (f->norm_on) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_normalise_enable has already been called on this handle");
    if (f->state_dim < 1 || f->state_dim + 1 > NORM_MAX_COLS)
        FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_normalise_enable: state_dim %d (1 .. %d)", f->state_dim, NORM_MAX_COLS - 1);
    return IMGENV_OK;
}
// the depth of the normalised state stack: the handle's, where IMGENV_NORM_OBS meets a state stack deeper than 1
inline int normalise_stack_depth(const FeatureFacts& f, bool obs) { return obs && f.stack_on && f.stack_state_depth >= 2 ? f.stack_state_depth : 0; }

// ---------------------------------------------------------------------------------------- the row-copy features' fields
enum FieldFeature { FIELDS_FINAL, FIELDS_ROLLOUT, FIELDS_MINIBATCH, FIELDS_SEQ };  // (the sequences gather the minibatches' fields)
struct FieldFeatureNames {
    const char *cfg, *bits;  // "imgenv_X_cfg" and the prefix of its bits' names
    const int* order;        // the block's order (obs_fields.h)
    int n_order;
};
inline FieldFeatureNames field_feature(FieldFeature which) {
    static const int n_final = (int)(sizeof(FINAL_FIELD_ORDER) / sizeof(int)), n_roll = (int)(sizeof(ROLLOUT_FIELD_ORDER) / sizeof(int));
    static const int n_mb = (int)(sizeof(MINIBATCH_FIELD_ORDER) / sizeof(int));
    static_assert(sizeof(FINAL_FIELD_ORDER) / sizeof(int) <= FINAL_MAX_FIELDS && sizeof(ROLLOUT_FIELD_ORDER) / sizeof(int) <= ROLLOUT_TABLE_FIELDS, "field tables");
    // (the minibatches' order lists the stored and the drawn ped_maps: one more than a selection can hold, select_feature_fields checks)
    static_assert(sizeof(MINIBATCH_FIELD_ORDER) / sizeof(int) <= FINAL_MAX_FIELDS, "field tables");
    switch (which) {
        case FIELDS_FINAL: return {"imgenv_final_obs_cfg", "IMGENV_FINAL", FINAL_FIELD_ORDER, n_final};
        case FIELDS_ROLLOUT: return {"imgenv_rollout_cfg", "IMGENV_ROLLOUT", ROLLOUT_FIELD_ORDER, n_roll};
        case FIELDS_SEQ: return {"imgenv_seq_cfg", "IMGENV_ROLLOUT", MINIBATCH_FIELD_ORDER, n_mb};
        default: return {"imgenv_minibatch_cfg", "IMGENV_ROLLOUT", MINIBATCH_FIELD_ORDER, n_mb};
    }
}
inline int field_bit(FieldFeature which, int id) { return which == FIELDS_FINAL ? OBS_SLOTS[id].final_bit : OBS_SLOTS[id].rollout_bit; }

// the field bits that name another feature's arrays, for the final observations and the rollout alike (the minibatches gather
// what the rollout already stores): the feature must be on, and must keep the array
inline int field_bits_refusals(FieldFeature which, const FeatureFacts& f, int want, FeatureMsg msg) {
    const FieldFeatureNames n = field_feature(which);
    const int lasers = field_bit(which, OBSF_LASERS) | field_bit(which, OBSF_LASERS_RAW), stacks = field_bit(which, OBSF_STACK_SENSOR_MAPS);
    if ((want & lasers) && f.n_beams <= 0) FEATURE_REFUSE(IMGENV_EINVAL, "%s.fields: lasers on a handle without use_laser", n.cfg);
    if ((want & field_bit(which, OBSF_VIEW_MAPS)) && !f.keep_view_maps) FEATURE_REFUSE(IMGENV_EINVAL, "%s.fields: view_maps under IMGENV_FLAG_NO_VIEW_MAPS", n.cfg);
    if ((want & stacks) && !f.stack_on) FEATURE_REFUSE(IMGENV_ESTATE, "%s_STACKS before imgenv_stack_enable", n.bits);
    if ((want & stacks) && f.stack_n_fields == 0) FEATURE_REFUSE(IMGENV_EINVAL, "%s_STACKS: no stack of this handle is deeper than 1", n.bits);
    if ((want & field_bit(which, OBSF_PED_VECTOR_NORM)) && !(f.post_on && f.post_norm))
        FEATURE_REFUSE(IMGENV_ESTATE, "%s_PED_NORM before imgenv_obs_post_enable with IMGENV_OBS_PED_NORM", n.bits);
    return IMGENV_OK;
}

// the fields a feature copies, in its block's order
struct FieldSelection {
    int n;
    int id[FINAL_MAX_FIELDS];
    size_t row_bytes[FINAL_MAX_FIELDS];
};
// The fields of `which`'s order whose bit is in `want`, out of the catalogue `cat` (the handle's arrays; for the minibatches what
// the ring keeps).  An optional field the catalogue lacks is skipped silently, any other without an array or of no bytes refused.
// `cfg_fields`: the cfg's own word, for the texts.  `drawn_row_bytes`: the row of a drawn field (the minibatches': ped_maps_row_bytes).
inline size_t ped_maps_row_bytes(const FeatureFacts& f) { return 3 * (size_t)(f.ped_h > 0 ? f.ped_h : 0) * (size_t)(f.ped_w > 0 ? f.ped_w : 0) * 4; }
inline int select_feature_fields(FieldFeature which, const ObsField (&cat)[OBSF_COUNT], int want, int cfg_fields, FieldSelection& s, FeatureMsg msg,
                                 size_t drawn_row_bytes = 0) {
    struct Pick { int bit, id; } list[FINAL_MAX_FIELDS];
    const Pick* sel[FINAL_MAX_FIELDS];
    const FieldFeatureNames n = field_feature(which);
    for (int k = 0; k < n.n_order; k++) list[k] = {field_bit(which, n.order[k]), n.order[k]};
    int bad_bit = 0;
    ObsField ext[OBSF_SLOT_COUNT];
    obs_fields_with_drawn(cat, drawn_row_bytes, ext);
    s.n = obs_fields_select_n(ext, list, n.n_order, want, sel, &bad_bit);
    if (s.n < 0) FEATURE_REFUSE(IMGENV_EINVAL, "%s.fields: bit %d names a field of no bytes on this handle", n.cfg, bad_bit);
    for (int k = 0; k < s.n; k++) {
        s.id[k] = sel[k]->id;
        s.row_bytes[k] = ext[s.id[k]].row_bytes;
    }
    if (which != FIELDS_FINAL && s.n > ROLLOUT_TABLE_FIELDS) FEATURE_REFUSE(IMGENV_EINVAL, "%s.fields %d: more fields than a table holds", n.cfg, cfg_fields);
    if (which == FIELDS_MINIBATCH && s.n == 0) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_minibatch_cfg.fields %d: no field of the rollout", cfg_fields);
    if (which == FIELDS_SEQ && s.n == 0) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_seq_cfg.fields %d: no field of the rollout", cfg_fields);
    return IMGENV_OK;
}

// ---------------------------------------------------------------------------------------- final observations
// (the IMGENV_*_NORM_* bits of the three cfgs are refused in FRONT of the null handle: a handle that is not there has no
// normalisation either)
inline int final_obs_enable_plan(const imgenv_final_obs_cfg* c, const imgenv_final_obs_out* out, const FeatureFacts* f, const imgenv_final_obs_cfg* stored,
                                 FeatureMsg msg) {
    FEATURE_TRY(enable_args(c, "imgenv_final_obs_cfg", out, "imgenv_final_obs_out", msg));
    if (c->fields == 0 || (c->fields & ~(IMGENV_FINAL_ALL | IMGENV_FINAL_NORM_STATES))) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_final_obs_cfg.fields %d", c->fields);
    if ((c->fields & IMGENV_FINAL_NORM_STATES) && !(f && f->norm_on && f->norm_obs))
        FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_final_obs_cfg.fields %d: IMGENV_FINAL_NORM_STATES before imgenv_normalise_enable with IMGENV_NORM_OBS", c->fields);
    FEATURE_TRY(enable_null_handle(f, msg));
    if (f->final_on) {
        if (c->fields != stored->fields)
            FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_final_obs_enable: the handle already keeps final observations of the fields %d", stored->fields);
        return ENABLE_REPEAT;
    }
    return field_bits_refusals(FIELDS_FINAL, *f, c->fields, msg);
}

// ---------------------------------------------------------------------------------------- rollout storage
inline bool rollout_cfg_same(const imgenv_rollout_cfg& c, const imgenv_rollout_cfg& o) {
    return c.horizon == o.horizon && c.final_capacity == o.final_capacity && c.fields == o.fields;
}
inline int rollout_enable_plan(const imgenv_rollout_cfg* c, const imgenv_rollout_out* out, const FeatureFacts* f, const imgenv_rollout_cfg* stored, FeatureMsg msg) {
    FEATURE_TRY(enable_args(c, "imgenv_rollout_cfg", out, "imgenv_rollout_out", msg));
    if (c->horizon < 1) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_rollout_cfg.horizon %d: at least 1", c->horizon);
    if (c->final_capacity < 1) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_rollout_cfg.final_capacity %d: at least 1", c->final_capacity);
    const int norm_bits = IMGENV_ROLLOUT_NORM_STATES | IMGENV_ROLLOUT_NORM_REWARDS, drawn = IMGENV_ROLLOUT_PED_MAPS_DRAWN;
    if (c->fields == 0 || (c->fields & ~(IMGENV_ROLLOUT_ALL | norm_bits | drawn))) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_rollout_cfg.fields %d", c->fields);
    // the drawn ped_maps: the ring keeps the vector they are drawn from, and not the maps themselves
    if (c->fields == drawn) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_rollout_cfg.fields %d", c->fields);  // (the bit alone stores nothing: the text of a word without a field)
    if ((c->fields & drawn) && !(c->fields & IMGENV_ROLLOUT_PED_VECTOR_STATES))
        FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_rollout_cfg.fields %d: IMGENV_ROLLOUT_PED_MAPS_DRAWN needs IMGENV_ROLLOUT_PED_VECTOR_STATES", c->fields);
    if ((c->fields & drawn) && (c->fields & IMGENV_ROLLOUT_PED_MAPS))
        FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_rollout_cfg.fields %d: IMGENV_ROLLOUT_PED_MAPS_DRAWN excludes IMGENV_ROLLOUT_PED_MAPS", c->fields);
    if (c->fields & norm_bits) {
        if (!(f && f->norm_on)) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_rollout_cfg.fields %d: IMGENV_ROLLOUT_NORM_* before imgenv_normalise_enable", c->fields);
        if ((c->fields & IMGENV_ROLLOUT_NORM_STATES) && !f->norm_obs)
            FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_rollout_cfg.fields %d: IMGENV_ROLLOUT_NORM_STATES without IMGENV_NORM_OBS", c->fields);
        if ((c->fields & IMGENV_ROLLOUT_NORM_REWARDS) && !f->norm_rew)
            FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_rollout_cfg.fields %d: IMGENV_ROLLOUT_NORM_REWARDS without IMGENV_NORM_REWARD", c->fields);
        if (!(c->fields & ~IMGENV_ROLLOUT_NORM_REWARDS)) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_rollout_cfg.fields %d: IMGENV_ROLLOUT_NORM_REWARDS selects no field", c->fields);
    }
    FEATURE_TRY(enable_null_handle(f, msg));
    if (f->roll_on) {
        if (!rollout_cfg_same(*c, *stored))
            FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_rollout_enable: the handle already keeps a rollout of horizon %d, final_capacity %d, fields %d", stored->horizon,
                           stored->final_capacity, stored->fields);
        return ENABLE_REPEAT;
    }
    if (((size_t)c->horizon + 1) * (size_t)f->RL > 0x7fffffffu)
        FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_rollout_cfg.horizon %d: (horizon + 1) x %d robots is beyond 2^31 - 1", c->horizon, f->RL);
    if ((c->fields & drawn) && !plan_ped_draw_fits(f->ped_h, f->ped_w))
        FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_rollout_cfg.fields %d: IMGENV_ROLLOUT_PED_MAPS_DRAWN with pedestrian maps of %d x %d cells (a plane of %d bytes at most)",
                       c->fields, f->ped_h, f->ped_w, PED_DRAW_LDS_BYTES);
    return field_bits_refusals(FIELDS_ROLLOUT, *f, c->fields, msg);
}

// ---------------------------------------------------------------------------------------- rollout minibatches (need the rollout)
inline bool minibatch_cfg_same(const imgenv_minibatch_cfg& c, const imgenv_minibatch_cfg& o) {
    return c.batch == o.batch && c.buffers == o.buffers && c.fields == o.fields;
}
// (*want: the bits in effect -- the cfg's, or with 0 every field the rollout stores)
inline int minibatch_enable_plan(const imgenv_minibatch_cfg* c, const imgenv_minibatch_out* out, const FeatureFacts* f, const imgenv_minibatch_cfg* stored,
                                 int* want, FeatureMsg msg) {
    FEATURE_TRY(enable_args(c, "imgenv_minibatch_cfg", out, "imgenv_minibatch_out", msg));
    if (c->batch < 1) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_minibatch_cfg.batch %d: at least 1", c->batch);
    if (c->buffers < 1 || c->buffers > IMGENV_MB_MAX_BUFFERS) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_minibatch_cfg.buffers %d: 1 .. %d", c->buffers, IMGENV_MB_MAX_BUFFERS);
    if (c->fields & ~(IMGENV_ROLLOUT_ALL | IMGENV_ROLLOUT_NORM_STATES | IMGENV_ROLLOUT_PED_MAPS_DRAWN)) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_minibatch_cfg.fields %d", c->fields);  // (NORM_REWARDS names no field)
    if ((c->fields & IMGENV_ROLLOUT_NORM_STATES) && !(f && f->norm_on))
        FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_minibatch_cfg.fields %d: IMGENV_ROLLOUT_NORM_* before imgenv_normalise_enable", c->fields);
    FEATURE_TRY(enable_null_handle(f, msg));
    if (!f->roll_on) FEATURE_REFUSE(IMGENV_ESTATE, "imgenv_rollout_minibatch_enable before imgenv_rollout_enable");
    if (f->mb_on) {
        if (!minibatch_cfg_same(*c, *stored))
            FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_rollout_minibatch_enable: the handle already gathers minibatches of batch %d, buffers %d, fields %d", stored->batch,
                           stored->buffers, stored->fields);
        return ENABLE_REPEAT;
    }
    *want = c->fields ? c->fields : (f->roll_fields & ~IMGENV_ROLLOUT_NORM_REWARDS);
    if (*want & ~f->roll_fields) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_minibatch_cfg.fields %d: the rollout stores %d", c->fields, f->roll_fields);
    return IMGENV_OK;
}

// ---------------------------------------------------------------------------------------- sequence minibatches (need the rollout,
// not the minibatches)
inline bool seq_cfg_same(const imgenv_seq_cfg& c, const imgenv_seq_cfg& o) {
    return c.length == o.length && c.batch == o.batch && c.buffers == o.buffers && c.fields == o.fields && c.state_bytes[0] == o.state_bytes[0] &&
           c.state_bytes[1] == o.state_bytes[1];
}
// (*want: the bits in effect, as minibatch_enable_plan's)
inline int seq_enable_plan(const imgenv_seq_cfg* c, const imgenv_seq_out* out, const FeatureFacts* f, const imgenv_seq_cfg* stored, int* want, FeatureMsg msg) {
    FEATURE_TRY(enable_args(c, "imgenv_seq_cfg", out, "imgenv_seq_out", msg));
    if (c->length < 1) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_seq_cfg.length %d: at least 1", c->length);
    if (c->batch < 1) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_seq_cfg.batch %d: at least 1", c->batch);
    if (c->buffers < 1 || c->buffers > IMGENV_MB_MAX_BUFFERS) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_seq_cfg.buffers %d: 1 .. %d", c->buffers, IMGENV_MB_MAX_BUFFERS);
    if (c->fields & ~(IMGENV_ROLLOUT_ALL | IMGENV_ROLLOUT_NORM_STATES | IMGENV_ROLLOUT_PED_MAPS_DRAWN)) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_seq_cfg.fields %d", c->fields);
    for (int a = 0; a < IMGENV_SEQ_MAX_STATES; a++)
        if (c->state_bytes[a] < 0 || c->state_bytes[a] % 4 != 0 || c->state_bytes[a] > SEQ_MAX_STATE_BYTES)
            FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_seq_cfg.state_bytes[%d] %d: a multiple of 4, 0 .. %d", a, c->state_bytes[a], SEQ_MAX_STATE_BYTES);
    if (c->reserved != 0) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_seq_cfg.reserved %d", c->reserved);
    if ((c->fields & IMGENV_ROLLOUT_NORM_STATES) && !(f && f->norm_on))
        FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_seq_cfg.fields %d: IMGENV_ROLLOUT_NORM_* before imgenv_normalise_enable", c->fields);
    FEATURE_TRY(enable_null_handle(f, msg));
    if (!f->roll_on) FEATURE_REFUSE(IMGENV_ESTATE, "imgenv_rollout_seq_enable before imgenv_rollout_enable");
    if (f->seq_on) {
        if (!seq_cfg_same(*c, *stored))
            FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_rollout_seq_enable: the handle already gathers sequences of length %d, batch %d, buffers %d, fields %d, state_bytes %d, %d",
                           stored->length, stored->batch, stored->buffers, stored->fields, stored->state_bytes[0], stored->state_bytes[1]);
        return ENABLE_REPEAT;
    }
    if (c->length > f->roll_horizon) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_seq_cfg.length %d: 1 .. the rollout's horizon %d", c->length, f->roll_horizon);
    if (plan_seq_chunks((size_t)f->roll_horizon, (size_t)c->length) * (size_t)f->RL > 0x7fffffffu)
        FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_seq_cfg.length %d: %zu chunks x %d robots is beyond 2^31 - 1", c->length,
                       plan_seq_chunks((size_t)f->roll_horizon, (size_t)c->length), f->RL);
    *want = c->fields ? c->fields : (f->roll_fields & ~IMGENV_ROLLOUT_NORM_REWARDS);
    if (*want & ~f->roll_fields) FEATURE_REFUSE(IMGENV_EINVAL, "imgenv_seq_cfg.fields %d: the rollout stores %d", c->fields, f->roll_fields);
    return IMGENV_OK;
}
