// feature_plan_check.cpp -- what an enable call of an optional feature decides before it touches a device
// (img_env_amd/csrc/feature_plan.h, the slot catalogue of obs_fields.h), on the CPU.
//   g++ -std=c++17 tests/host/feature_plan_check.cpp -o check && ./check
// (also built with -fsanitize=address,undefined by tests/test_feature_plan.py)
//
// Every literal here was written down by hand from the commit before feature_plan.h existed: the refusals' codes and texts from the
// FAIL lines the enable functions of imgenv_hip.hip then had, the selected fields and the members their pointers land in from the
// three local lists of imgenv_final_obs_enable, imgenv_rollout_enable and imgenv_rollout_minibatch_enable.  None is printed from the
// code under test.
#include <limits>
#include <string>
#include <vector>

#include "../../img_env_amd/csrc/feature_plan.h"

static int n_bad = 0, n_checks = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        n_checks++;                                                  \
        if (!(cond)) {                                               \
            n_bad++;                                                 \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                            \
    } while (0)
// a plan's verdict: its code and its full text (an accepted call leaves no text)
#define REFUSED(call, code, text)                                                \
    do {                                                                         \
        FeatureMsg msg = "";                                                     \
        const int rc_ = (call);                                                  \
        CHECK(rc_ == (code));                                                    \
        CHECK(std::string(msg) == (text));                                       \
        if (std::string(msg) != (text)) printf("  got %d: %s\n", rc_, msg);      \
    } while (0)
#define ACCEPTED(call, code) REFUSED(call, code, "")

static const double NaN = std::numeric_limits<double>::quiet_NaN(), Inf = std::numeric_limits<double>::infinity();

// a handle of 4 local robots with pedestrians, lasers and view maps, nothing enabled
static FeatureFacts bare() {
    FeatureFacts f;
    f.RL = 4; f.P = 3; f.state_dim = 3; f.ped_vec_dim = 7; f.n_beams = 181;
    f.keep_view_maps = true;
    return f;
}
// everything on: stacks of depth (3, 3, 2), TABLE actions of 11 rows, a categorical head with STORE, the loss, both obs_post
// flags, a rollout of horizon 3 over every field, minibatches, both halves of the normalisation
static FeatureFacts full() {
    FeatureFacts f = bare();
    f.stack_on = true; f.stack_state_depth = 3; f.stack_n_fields = 3;
    f.ep_on = f.eplog_on = true; f.eplog_capacity = 8;
    f.act_on = true; f.act_mode = IMGENV_ACTIONS_TABLE; f.act_n_table = 11; f.act_n_cols = 2;
    f.pol_on = true; f.pol_kind = IMGENV_POLICY_CATEGORICAL; f.pol_flags = IMGENV_POLICY_STORE; f.pol_A = 11;
    f.ploss_on = true;
    f.post_on = f.post_norm = true;
    f.final_on = true;
    f.roll_on = true; f.roll_horizon = 3; f.roll_fields = IMGENV_ROLLOUT_ALL | IMGENV_ROLLOUT_NORM_STATES | IMGENV_ROLLOUT_NORM_REWARDS;
    f.mb_on = true;
    f.norm_on = f.norm_obs = f.norm_rew = true;
    return f;
}
template <typename Cfg>
static Cfg sized() {
    Cfg c = {};
    c.struct_size = (int32_t)sizeof(Cfg);
    return c;
}

// ---------------------------------------------------------------------------------------- the shared front and the helper
static void check_args() {
    imgenv_episodes_cfg c = sized<imgenv_episodes_cfg>();
    imgenv_episodes_out o = {};
    REFUSED(enable_args((const imgenv_episodes_cfg*)nullptr, "imgenv_episodes_cfg", &o, "imgenv_episodes_out", msg), IMGENV_EINVAL, "null argument");
    c.struct_size = 8;
    REFUSED(enable_args(&c, "imgenv_episodes_cfg", &o, "imgenv_episodes_out", msg), IMGENV_EINVAL, "imgenv_episodes_cfg.struct_size 8 (this library's is 16)");
    c.struct_size = 16;
    o.struct_size = 4;
    REFUSED(enable_args(&c, "imgenv_episodes_cfg", &o, "imgenv_episodes_out", msg), IMGENV_EINVAL, "imgenv_episodes_out.struct_size");
    o.struct_size = (int32_t)sizeof(o);
    ACCEPTED(enable_args(&c, "imgenv_episodes_cfg", &o, "imgenv_episodes_out", msg), IMGENV_OK);
    o.struct_size = 0;
    ACCEPTED(enable_args(&c, "imgenv_episodes_cfg", &o, "imgenv_episodes_out", msg), IMGENV_OK);
    ACCEPTED(enable_args(&c, "imgenv_episodes_cfg", (const imgenv_episodes_out*)nullptr, "imgenv_episodes_out", msg), IMGENV_OK);
    REFUSED(feature_needed(false, "imgenv_rollout_enable", msg), IMGENV_ESTATE, "imgenv_rollout_enable was not called");
    ACCEPTED(feature_needed(true, "imgenv_rollout_enable", msg), IMGENV_OK);
}

// ---------------------------------------------------------------------------------------- stacks
static void check_stack() {
    FeatureFacts f = bare();
    imgenv_stack_cfg s = sized<imgenv_stack_cfg>();
    s.image_batch = s.state_batch = s.laser_batch = 2;
    ACCEPTED(stack_enable_plan(&s, nullptr, &f, msg), IMGENV_OK);
    // (unlike the others: the handle in front of the cfg)
    imgenv_stack_cfg bad = s;
    bad.struct_size = 4;
    REFUSED(stack_enable_plan(&bad, nullptr, nullptr, msg), IMGENV_EINVAL, "null argument");
    REFUSED(stack_enable_plan(&bad, nullptr, &f, msg), IMGENV_EINVAL, "imgenv_stack_cfg.struct_size 4 (this library's is 32)");
    f.stack_on = true;
    REFUSED(stack_enable_plan(&s, nullptr, &f, msg), IMGENV_ESTATE, "imgenv_stack_enable has already been called on this handle");
    f.stack_on = false;
    f.any_reset = true;
    REFUSED(stack_enable_plan(&s, nullptr, &f, msg), IMGENV_ESTATE, "imgenv_stack_enable after the first reset");
    f.any_reset = false;
    bad = s;
    bad.state_batch = -1;
    REFUSED(stack_enable_plan(&bad, nullptr, &f, msg), IMGENV_EINVAL, "image_batch / state_batch must be >= 0");
    bad = s;
    bad.laser_batch = 17;
    REFUSED(stack_enable_plan(&bad, nullptr, &f, msg), IMGENV_EINVAL, "a stack depth above IMGENV_STACK_MAX_DEPTH (16)");
    REFUSED(stack_cfg_refusals(bad, msg), IMGENV_EINVAL, "a stack depth above IMGENV_STACK_MAX_DEPTH (16)");
    s.arena = (void*)(uintptr_t)4096;
    s.arena_bytes = 1000;
    REFUSED(stack_arena_refusals(s, 1024, msg), IMGENV_EINVAL, "stack arena too small: 1000 < 1024");
    s.arena = (void*)(uintptr_t)(4096 + 128);
    s.arena_bytes = 1024;
    REFUSED(stack_arena_refusals(s, 1024, msg), IMGENV_EINVAL, "stack arena must be 256-byte aligned");
    s.arena = (void*)(uintptr_t)4096;
    ACCEPTED(stack_arena_refusals(s, 1024, msg), IMGENV_OK);
}

// ---------------------------------------------------------------------------------------- episodes and their log
static void check_episodes() {
    FeatureFacts f = bare();
    imgenv_episodes_cfg c = sized<imgenv_episodes_cfg>();
    c.min_steps = 3;
    c.dt = 0.4;
    ACCEPTED(episodes_enable_plan(&c, nullptr, &f, nullptr, msg), IMGENV_OK);
    REFUSED(episodes_enable_plan(&c, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, "null argument");  // a good cfg, no handle
    imgenv_episodes_cfg bad = c;
    bad.dt = 0.0;
    REFUSED(episodes_enable_plan(&bad, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, "imgenv_episodes_cfg.dt must be > 0 (the YAML's control_hz)");  // the cfg first
    bad.dt = Inf;
    REFUSED(episodes_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_episodes_cfg.dt must be > 0 (the YAML's control_hz)");
    bad = c;
    bad.min_steps = -1;
    REFUSED(episodes_enable_plan(&bad, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, "imgenv_episodes_cfg.min_steps must be >= 0");
    // the repeated call
    f.ep_on = true;
    const imgenv_episodes_cfg stored = c;
    imgenv_episodes_cfg again = c;
    ACCEPTED(episodes_enable_plan(&again, nullptr, &f, &stored, msg), ENABLE_REPEAT);
    CHECK(episodes_cfg_same(again, stored));
    again.min_steps = 4;
    CHECK(!episodes_cfg_same(again, stored));
    REFUSED(episodes_enable_plan(&again, nullptr, &f, &stored, msg), IMGENV_EINVAL,
            "imgenv_episodes_enable: the handle already keeps statistics with min_steps 3, dt 0.4");
    again = c;
    again.dt = 0.5;
    CHECK(!episodes_cfg_same(again, stored));

    // the log needs the episodes -- and says so in front of the repeated call
    imgenv_episode_log_cfg l = sized<imgenv_episode_log_cfg>();
    l.capacity = 8;
    f = bare();
    REFUSED(episode_log_enable_plan(&l, nullptr, &f, msg), IMGENV_ESTATE, "imgenv_episode_log_enable before imgenv_episodes_enable");
    REFUSED(episode_log_enable_plan(&l, nullptr, nullptr, msg), IMGENV_EINVAL, "null argument");
    f.ep_on = true;
    ACCEPTED(episode_log_enable_plan(&l, nullptr, &f, msg), IMGENV_OK);
    imgenv_episode_log_cfg lbad = l;
    lbad.capacity = 0;
    REFUSED(episode_log_enable_plan(&lbad, nullptr, nullptr, msg), IMGENV_EINVAL, "imgenv_episode_log_cfg.capacity 0: 1 .. 4194304");
    lbad.capacity = (1 << 22) + 1;
    REFUSED(episode_log_enable_plan(&lbad, nullptr, &f, msg), IMGENV_EINVAL, "imgenv_episode_log_cfg.capacity 4194305: 1 .. 4194304");
    f.eplog_on = true;
    f.eplog_capacity = 8;
    ACCEPTED(episode_log_enable_plan(&l, nullptr, &f, msg), ENABLE_REPEAT);
    l.capacity = 9;
    REFUSED(episode_log_enable_plan(&l, nullptr, &f, msg), IMGENV_EINVAL, "imgenv_episode_log_enable: the handle already keeps a log of capacity 8");
    f.ep_on = false;  // (cannot happen on a handle; the order is what is checked)
    REFUSED(episode_log_enable_plan(&l, nullptr, &f, msg), IMGENV_ESTATE, "imgenv_episode_log_enable before imgenv_episodes_enable");
}

// ---------------------------------------------------------------------------------------- actions
static void check_actions() {
    FeatureFacts f = bare();
    const float rows[6] = {0.0f, 0.5f, 0.0f, 1.0f, -0.5f, 1.0f};
    imgenv_actions_cfg t = sized<imgenv_actions_cfg>();
    t.mode = IMGENV_ACTIONS_TABLE;
    t.n_cols = 2;
    t.n_table = 2;
    t.table = rows;
    imgenv_actions_cfg k = sized<imgenv_actions_cfg>();
    k.mode = IMGENV_ACTIONS_CLIP;
    k.n_cols = 2;
    k.clip[0][0] = 0.0f; k.clip[0][1] = 1.0f; k.clip[1][0] = -1.0f; k.clip[1][1] = 1.0f;
    ACCEPTED(actions_enable_plan(&t, nullptr, &f, nullptr, nullptr, msg), IMGENV_OK);
    ACCEPTED(actions_enable_plan(&k, nullptr, &f, nullptr, nullptr, msg), IMGENV_OK);
    REFUSED(actions_enable_plan(&t, nullptr, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, "null argument");
    imgenv_actions_cfg bad = t;
    bad.mode = 2;
    REFUSED(actions_enable_plan(&bad, nullptr, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, "imgenv_actions_cfg.mode 2");
    bad = t;
    bad.n_cols = 4;
    REFUSED(actions_enable_plan(&bad, nullptr, &f, nullptr, nullptr, msg), IMGENV_EINVAL, "imgenv_actions_cfg.n_cols 4: 2 (v, w) or 3 (v, w, beep)");
    bad = t;
    bad.table = nullptr;
    REFUSED(actions_enable_plan(&bad, nullptr, &f, nullptr, nullptr, msg), IMGENV_EINVAL, "imgenv_actions_cfg.table: 1 .. 4096 rows (n_table 2)");
    bad = t;
    bad.n_table = 4097;
    REFUSED(actions_enable_plan(&bad, nullptr, &f, nullptr, nullptr, msg), IMGENV_EINVAL, "imgenv_actions_cfg.table: 1 .. 4096 rows (n_table 4097)");
    float nan_rows[6] = {0.0f, 0.5f, 0.0f, 1.0f, (float)NaN, 1.0f};
    bad = t;
    bad.table = nan_rows;
    REFUSED(actions_enable_plan(&bad, nullptr, &f, nullptr, nullptr, msg), IMGENV_EINVAL, "imgenv_actions_cfg.table row 1 holds a value that is not finite");
    bad = k;
    bad.clip[1][0] = 2.0f;
    REFUSED(actions_enable_plan(&bad, nullptr, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, "imgenv_actions_cfg.clip[1] = (2, 1): finite bounds with lo <= hi");
    // the repeated call: the table's rows are compared, not its pointer; CLIP compares the bounds of its n_cols columns
    f.act_on = true;
    imgenv_actions_cfg stored = t;
    stored.table = nullptr;  // (as the handle keeps it)
    const std::vector<float> kept(rows, rows + 6);
    float copy[6];
    memcpy(copy, rows, sizeof(copy));
    imgenv_actions_cfg again = t;
    again.table = copy;
    CHECK(actions_cfg_same(again, stored, kept.data()));
    ACCEPTED(actions_enable_plan(&again, nullptr, &f, &stored, kept.data(), msg), ENABLE_REPEAT);
    copy[4] = 0.25f;
    CHECK(!actions_cfg_same(again, stored, kept.data()));
    REFUSED(actions_enable_plan(&again, nullptr, &f, &stored, kept.data(), msg), IMGENV_EINVAL, "imgenv_actions_enable: the handle already decodes actions with another cfg");
    copy[4] = rows[4];
    again.n_table = 1;
    CHECK(!actions_cfg_same(again, stored, kept.data()));
    again = t; again.table = copy; again.n_cols = 3;
    CHECK(!actions_cfg_same(again, stored, kept.data()));
    again = t; again.table = copy; again.clip[0][0] = 9.0f;  // (the bounds do not count in TABLE mode)
    CHECK(actions_cfg_same(again, stored, kept.data()));
    CHECK(!actions_cfg_same(k, stored, kept.data()));  // another mode
    imgenv_actions_cfg kstored = k, kagain = k;
    CHECK(actions_cfg_same(kagain, kstored, nullptr));
    kagain.clip[1][1] = 2.0f;
    CHECK(!actions_cfg_same(kagain, kstored, nullptr));
    kagain = k; kagain.clip[2][0] = 5.0f;  // (column 2 of an n_cols = 2 cfg), n_table, the pointer: not compared in CLIP mode
    kagain.n_table = 7; kagain.table = rows;
    CHECK(actions_cfg_same(kagain, kstored, nullptr));
}

// ---------------------------------------------------------------------------------------- the policy head and the loss
static void check_policy() {
    FeatureFacts f = bare();
    imgenv_policy_cfg c = sized<imgenv_policy_cfg>();
    c.kind = IMGENV_POLICY_CATEGORICAL;
    c.seed = 7;
    REFUSED(policy_enable_plan(&c, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, "null argument");
    imgenv_policy_cfg bad = c;
    bad.kind = 2;
    REFUSED(policy_enable_plan(&bad, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, "imgenv_policy_cfg.kind 2");
    bad = c; bad.flags = 2;
    REFUSED(policy_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_policy_cfg.flags 2");
    bad = c; bad.reserved = 1;
    REFUSED(policy_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_policy_cfg.reserved 1");
    REFUSED(policy_enable_plan(&c, nullptr, &f, nullptr, msg), IMGENV_ESTATE, "imgenv_policy_enable before imgenv_actions_enable");
    f.act_on = true; f.act_mode = IMGENV_ACTIONS_CLIP; f.act_n_cols = 2;
    REFUSED(policy_enable_plan(&c, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_policy_enable: a categorical head needs imgenv_actions_enable in TABLE mode");
    imgenv_policy_cfg g = c;
    g.kind = IMGENV_POLICY_GAUSSIAN;
    ACCEPTED(policy_enable_plan(&g, nullptr, &f, nullptr, msg), IMGENV_OK);
    f.act_mode = IMGENV_ACTIONS_TABLE; f.act_n_table = 11;
    REFUSED(policy_enable_plan(&g, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_policy_enable: a Gaussian head needs imgenv_actions_enable in CLIP mode");
    ACCEPTED(policy_enable_plan(&c, nullptr, &f, nullptr, msg), IMGENV_OK);
    imgenv_policy_cfg st = c;
    st.flags = IMGENV_POLICY_STORE;
    REFUSED(policy_enable_plan(&st, nullptr, &f, nullptr, msg), IMGENV_ESTATE, "imgenv_policy_enable: IMGENV_POLICY_STORE before imgenv_rollout_enable");
    f.roll_on = true;
    ACCEPTED(policy_enable_plan(&st, nullptr, &f, nullptr, msg), IMGENV_OK);
    // the repeated call comes in FRONT of the prerequisites: the same cfg again succeeds whatever the actions' state says
    FeatureFacts odd = bare();
    odd.pol_on = true;
    const imgenv_policy_cfg stored = c;
    ACCEPTED(policy_enable_plan(&c, nullptr, &odd, &stored, msg), ENABLE_REPEAT);
    imgenv_policy_cfg again = c;
    CHECK(policy_cfg_same(again, stored));
    again.kind = IMGENV_POLICY_GAUSSIAN;
    CHECK(!policy_cfg_same(again, stored));
    REFUSED(policy_enable_plan(&again, nullptr, &odd, &stored, msg), IMGENV_EINVAL, "imgenv_policy_enable: the handle already has a policy head with another cfg");
    again = c; again.flags = IMGENV_POLICY_STORE;
    CHECK(!policy_cfg_same(again, stored));
    again = c; again.seed = 8;
    CHECK(!policy_cfg_same(again, stored));
    again = c; again.reserved = 5; again.struct_size = 0;  // not compared
    CHECK(policy_cfg_same(again, stored));

    // the loss needs the policy head, behind its own repeated call
    imgenv_policy_loss_cfg l = sized<imgenv_policy_loss_cfg>();
    l.max_rows = 5;
    f = bare();
    REFUSED(policy_loss_enable_plan(&l, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, "null argument");
    REFUSED(policy_loss_enable_plan(&l, nullptr, &f, nullptr, msg), IMGENV_ESTATE, "imgenv_policy_loss_enable before imgenv_policy_enable");
    imgenv_policy_loss_cfg lbad = l;
    lbad.max_rows = 0;
    REFUSED(policy_loss_enable_plan(&lbad, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, "imgenv_policy_loss_cfg.max_rows 0 (at least 1)");
    lbad = l; lbad.reserved[1] = 1;
    REFUSED(policy_loss_enable_plan(&lbad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_policy_loss_cfg.reserved");
    f.pol_on = true;
    ACCEPTED(policy_loss_enable_plan(&l, nullptr, &f, nullptr, msg), IMGENV_OK);
    f.pol_on = false;
    f.ploss_on = true;
    const imgenv_policy_loss_cfg lstored = l;
    ACCEPTED(policy_loss_enable_plan(&l, nullptr, &f, &lstored, msg), ENABLE_REPEAT);
    CHECK(policy_loss_cfg_same(l, lstored));
    l.max_rows = 6;
    CHECK(!policy_loss_cfg_same(l, lstored));
    REFUSED(policy_loss_enable_plan(&l, nullptr, &f, &lstored, msg), IMGENV_EINVAL, "imgenv_policy_loss_enable: the handle already has a policy loss with another cfg");
}

// ---------------------------------------------------------------------------------------- obs_post and normalise
static imgenv_obs_post_cfg post_cfg(int flags) {
    imgenv_obs_post_cfg c = sized<imgenv_obs_post_cfg>();
    const double avg[7] = {0, 0, 0, 0, 0.25, 0.25, 0}, sd[7] = {6, 6, 0.6, 0.9, 0.5, 0.5, 6};
    c.flags = flags;
    memcpy(c.avg, avg, sizeof(avg));
    memcpy(c.std, sd, sizeof(sd));
    c.close_dist = 1.5;
    return c;
}
static void check_obs_post() {
    FeatureFacts f = bare();
    const imgenv_obs_post_cfg both = post_cfg(IMGENV_OBS_PED_NORM | IMGENV_OBS_CLOSE);
    ACCEPTED(obs_post_enable_plan(&both, nullptr, &f, nullptr, msg), IMGENV_OK);
    REFUSED(obs_post_enable_plan(&both, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, "null argument");
    imgenv_obs_post_cfg bad = both;
    bad.flags = 0;
    REFUSED(obs_post_enable_plan(&bad, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, "imgenv_obs_post_cfg.flags 0");
    bad.flags = 4;
    REFUSED(obs_post_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_obs_post_cfg.flags 4");
    bad = both; bad.avg[2] = NaN;
    REFUSED(obs_post_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_obs_post_cfg: avg[2] / std[2] is not finite");
    bad = both; bad.std[5] = 0.0;
    REFUSED(obs_post_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_obs_post_cfg.std[5] is 0");
    bad = both; bad.close_dist = NaN;
    REFUSED(obs_post_enable_plan(&bad, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, "imgenv_obs_post_cfg.close_dist is not a number");
    bad = post_cfg(IMGENV_OBS_CLOSE); bad.std[0] = 0.0; bad.avg[1] = NaN;  // (not looked at without PED_NORM)
    ACCEPTED(obs_post_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_OK);
    f.ped_vec_dim = 5;
    REFUSED(obs_post_enable_plan(&both, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "IMGENV_OBS_PED_NORM: ped_vec_dim 5 (the wrapper's constants are for 7)");
    f = bare();
    f.P = 0;
    REFUSED(obs_post_enable_plan(&both, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "IMGENV_OBS_CLOSE on a handle without pedestrians");
    // the repeated call, in front of the facts' refusals; avg / std only under PED_NORM, close_dist only under CLOSE
    f.post_on = true;
    ACCEPTED(obs_post_enable_plan(&both, nullptr, &f, &both, msg), ENABLE_REPEAT);
    imgenv_obs_post_cfg again = both;
    CHECK(obs_post_cfg_same(again, both));
    again.avg[3] = 1.0;
    CHECK(!obs_post_cfg_same(again, both));
    REFUSED(obs_post_enable_plan(&again, nullptr, &f, &both, msg), IMGENV_EINVAL,
            "imgenv_obs_post_enable: the handle already post-processes its observations with another cfg");
    again = both; again.std[6] = 7.0;
    CHECK(!obs_post_cfg_same(again, both));
    again = both; again.close_dist = 2.0;
    CHECK(!obs_post_cfg_same(again, both));
    again = both; again.flags = IMGENV_OBS_CLOSE;
    CHECK(!obs_post_cfg_same(again, both));
    const imgenv_obs_post_cfg norm_only = post_cfg(IMGENV_OBS_PED_NORM), close_only = post_cfg(IMGENV_OBS_CLOSE);
    again = norm_only; again.close_dist = 9.0;
    CHECK(obs_post_cfg_same(again, norm_only));
    again = close_only; again.avg[0] = 9.0; again.std[0] = 9.0;
    CHECK(obs_post_cfg_same(again, close_only));
}

static void check_normalise() {
    FeatureFacts f = bare();
    imgenv_normalise_cfg c = sized<imgenv_normalise_cfg>();
    c.flags = IMGENV_NORM_OBS | IMGENV_NORM_REWARD;
    c.gamma = 0.99; c.clip_obs = 10.0; c.clip_reward = 10.0; c.eps = 1e-8;
    ACCEPTED(normalise_enable_plan(&c, nullptr, &f, msg), IMGENV_OK);
    REFUSED(normalise_enable_plan(&c, nullptr, nullptr, msg), IMGENV_EINVAL, "null argument");
    imgenv_normalise_cfg bad = c;
    bad.flags = 4;
    REFUSED(normalise_enable_plan(&bad, nullptr, nullptr, msg), IMGENV_EINVAL, "imgenv_normalise_cfg.flags 4");
    bad.flags = 0;
    REFUSED(normalise_enable_plan(&bad, nullptr, &f, msg), IMGENV_EINVAL, "imgenv_normalise_cfg.flags 0");
    bad = c; bad.clip_obs = 0.0;
    REFUSED(normalise_enable_plan(&bad, nullptr, &f, msg), IMGENV_EINVAL, "imgenv_normalise_cfg.clip_obs 0: finite and above 0");
    bad = c; bad.clip_reward = Inf;
    REFUSED(normalise_enable_plan(&bad, nullptr, &f, msg), IMGENV_EINVAL, "imgenv_normalise_cfg.clip_reward inf: finite and above 0");
    bad = c; bad.eps = -1.0;
    REFUSED(normalise_enable_plan(&bad, nullptr, &f, msg), IMGENV_EINVAL, "imgenv_normalise_cfg.eps -1: finite and above 0");
    bad = c; bad.gamma = 1.5;
    REFUSED(normalise_enable_plan(&bad, nullptr, nullptr, msg), IMGENV_EINVAL, "imgenv_normalise_cfg.gamma 1.5: 0 .. 1");
    f.norm_on = true;  // any second call is refused, the same cfg included
    REFUSED(normalise_enable_plan(&c, nullptr, &f, msg), IMGENV_EINVAL, "imgenv_normalise_enable has already been called on this handle");
    f = bare();
    f.state_dim = 64;
    REFUSED(normalise_enable_plan(&c, nullptr, &f, msg), IMGENV_EINVAL, "imgenv_normalise_enable: state_dim 64 (1 .. 63)");
    f.state_dim = 0;
    REFUSED(normalise_enable_plan(&c, nullptr, &f, msg), IMGENV_EINVAL, "imgenv_normalise_enable: state_dim 0 (1 .. 63)");
    // the state stack's depth as it is at the enable
    f = bare();
    CHECK(normalise_stack_depth(f, true) == 0);
    f.stack_on = true; f.stack_state_depth = 3;
    CHECK(normalise_stack_depth(f, true) == 3);
    CHECK(normalise_stack_depth(f, false) == 0);
    f.stack_state_depth = 1;
    CHECK(normalise_stack_depth(f, true) == 0);
}

// ---------------------------------------------------------------------------------------- the row-copy features' cfgs
static void check_final_obs() {
    FeatureFacts f = bare();
    imgenv_final_obs_cfg c = sized<imgenv_final_obs_cfg>();
    c.fields = IMGENV_FINAL_IMAGE_STATE;
    ACCEPTED(final_obs_enable_plan(&c, nullptr, &f, nullptr, msg), IMGENV_OK);
    REFUSED(final_obs_enable_plan(&c, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, "null argument");
    imgenv_final_obs_cfg bad = c;
    bad.fields = 0;
    REFUSED(final_obs_enable_plan(&bad, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, "imgenv_final_obs_cfg.fields 0");
    bad.fields = 16384;
    REFUSED(final_obs_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_final_obs_cfg.fields 16384");
    // the normalised states: refused in FRONT of the null handle
    bad.fields = IMGENV_FINAL_VECTOR_STATES | IMGENV_FINAL_NORM_STATES;
    const char* norm_text = "imgenv_final_obs_cfg.fields 8193: IMGENV_FINAL_NORM_STATES before imgenv_normalise_enable with IMGENV_NORM_OBS";
    REFUSED(final_obs_enable_plan(&bad, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, norm_text);
    REFUSED(final_obs_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, norm_text);
    f.norm_on = true; f.norm_rew = true;  // (reward only)
    REFUSED(final_obs_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, norm_text);
    f.norm_obs = true;
    ACCEPTED(final_obs_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_OK);
    // the bits that need the handle's arrays or another feature
    f = bare();
    f.n_beams = 0;
    bad.fields = IMGENV_FINAL_LASERS;
    REFUSED(final_obs_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_final_obs_cfg.fields: lasers on a handle without use_laser");
    bad.fields = IMGENV_FINAL_LASERS_RAW;
    REFUSED(final_obs_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_final_obs_cfg.fields: lasers on a handle without use_laser");
    f = bare();
    f.keep_view_maps = false;
    bad.fields = IMGENV_FINAL_VIEW_MAPS;
    REFUSED(final_obs_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_final_obs_cfg.fields: view_maps under IMGENV_FLAG_NO_VIEW_MAPS");
    f = bare();
    bad.fields = IMGENV_FINAL_STACKS;
    REFUSED(final_obs_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_ESTATE, "IMGENV_FINAL_STACKS before imgenv_stack_enable");
    f.stack_on = true;
    REFUSED(final_obs_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "IMGENV_FINAL_STACKS: no stack of this handle is deeper than 1");
    f.stack_n_fields = 1;
    ACCEPTED(final_obs_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_OK);
    bad.fields = IMGENV_FINAL_PED_NORM;
    REFUSED(final_obs_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_ESTATE, "IMGENV_FINAL_PED_NORM before imgenv_obs_post_enable with IMGENV_OBS_PED_NORM");
    f.post_on = true;  // (IMGENV_OBS_CLOSE alone)
    REFUSED(final_obs_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_ESTATE, "IMGENV_FINAL_PED_NORM before imgenv_obs_post_enable with IMGENV_OBS_PED_NORM");
    f.post_norm = true;
    ACCEPTED(final_obs_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_OK);
    // the repeated call in front of those
    f = bare();
    f.final_on = true;
    imgenv_final_obs_cfg stored = c;
    stored.fields = IMGENV_FINAL_STACKS;
    bad.fields = IMGENV_FINAL_STACKS;
    ACCEPTED(final_obs_enable_plan(&bad, nullptr, &f, &stored, msg), ENABLE_REPEAT);
    bad.fields = IMGENV_FINAL_LASERS;
    REFUSED(final_obs_enable_plan(&bad, nullptr, &f, &stored, msg), IMGENV_EINVAL, "imgenv_final_obs_enable: the handle already keeps final observations of the fields 2048");
}

static void check_rollout() {
    FeatureFacts f = bare();
    imgenv_rollout_cfg c = sized<imgenv_rollout_cfg>();
    c.horizon = 3; c.final_capacity = 4; c.fields = IMGENV_ROLLOUT_VECTOR_STATES | IMGENV_ROLLOUT_SENSOR_MAPS;
    ACCEPTED(rollout_enable_plan(&c, nullptr, &f, nullptr, msg), IMGENV_OK);
    REFUSED(rollout_enable_plan(&c, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, "null argument");
    imgenv_rollout_cfg bad = c;
    bad.horizon = 0;
    REFUSED(rollout_enable_plan(&bad, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, "imgenv_rollout_cfg.horizon 0: at least 1");
    bad = c; bad.final_capacity = 0;
    REFUSED(rollout_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_rollout_cfg.final_capacity 0: at least 1");
    bad = c; bad.fields = 0;
    REFUSED(rollout_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_rollout_cfg.fields 0");
    bad.fields = 512;
    REFUSED(rollout_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_rollout_cfg.fields 512");
    // the normalised bits: in FRONT of the null handle
    bad.fields = IMGENV_ROLLOUT_VECTOR_STATES | IMGENV_ROLLOUT_NORM_STATES;
    REFUSED(rollout_enable_plan(&bad, nullptr, nullptr, nullptr, msg), IMGENV_EINVAL, "imgenv_rollout_cfg.fields 130: IMGENV_ROLLOUT_NORM_* before imgenv_normalise_enable");
    REFUSED(rollout_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_rollout_cfg.fields 130: IMGENV_ROLLOUT_NORM_* before imgenv_normalise_enable");
    f.norm_on = true; f.norm_rew = true;
    REFUSED(rollout_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_rollout_cfg.fields 130: IMGENV_ROLLOUT_NORM_STATES without IMGENV_NORM_OBS");
    f.norm_rew = false; f.norm_obs = true;
    ACCEPTED(rollout_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_OK);
    bad.fields = IMGENV_ROLLOUT_VECTOR_STATES | IMGENV_ROLLOUT_NORM_REWARDS;
    REFUSED(rollout_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_rollout_cfg.fields 258: IMGENV_ROLLOUT_NORM_REWARDS without IMGENV_NORM_REWARD");
    f.norm_rew = true;
    ACCEPTED(rollout_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_OK);
    bad.fields = IMGENV_ROLLOUT_NORM_REWARDS;
    REFUSED(rollout_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_rollout_cfg.fields 256: IMGENV_ROLLOUT_NORM_REWARDS selects no field");
    // behind the repeated call: the size, then the bits that need the handle's arrays or another feature
    f = bare();
    f.RL = 1 << 20;
    bad = c; bad.horizon = 2047;
    REFUSED(rollout_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_rollout_cfg.horizon 2047: (horizon + 1) x 1048576 robots is beyond 2^31 - 1");
    bad.horizon = 2046;
    ACCEPTED(rollout_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_OK);
    f = bare();
    f.n_beams = 0;
    bad = c; bad.fields = IMGENV_ROLLOUT_LASERS;
    REFUSED(rollout_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "imgenv_rollout_cfg.fields: lasers on a handle without use_laser");
    f = bare();
    bad.fields = IMGENV_ROLLOUT_STACKS;
    REFUSED(rollout_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_ESTATE, "IMGENV_ROLLOUT_STACKS before imgenv_stack_enable");
    f.stack_on = true;
    REFUSED(rollout_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_EINVAL, "IMGENV_ROLLOUT_STACKS: no stack of this handle is deeper than 1");
    f.stack_n_fields = 2;
    ACCEPTED(rollout_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_OK);
    bad.fields = IMGENV_ROLLOUT_PED_NORM;
    REFUSED(rollout_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_ESTATE, "IMGENV_ROLLOUT_PED_NORM before imgenv_obs_post_enable with IMGENV_OBS_PED_NORM");
    f.keep_view_maps = false;  // (no bit of the rollout names the view maps: 512 is no field of it)
    f.post_on = f.post_norm = true;
    ACCEPTED(rollout_enable_plan(&bad, nullptr, &f, nullptr, msg), IMGENV_OK);
    // the repeated call
    f = bare();
    f.roll_on = true;
    const imgenv_rollout_cfg stored = c;
    imgenv_rollout_cfg again = c;
    CHECK(rollout_cfg_same(again, stored));
    ACCEPTED(rollout_enable_plan(&again, nullptr, &f, &stored, msg), ENABLE_REPEAT);
    again.horizon = 4;
    CHECK(!rollout_cfg_same(again, stored));
    REFUSED(rollout_enable_plan(&again, nullptr, &f, &stored, msg), IMGENV_EINVAL, "imgenv_rollout_enable: the handle already keeps a rollout of horizon 3, final_capacity 4, fields 3");
    again = c; again.final_capacity = 5;
    CHECK(!rollout_cfg_same(again, stored));
    again = c; again.fields = IMGENV_ROLLOUT_STACKS;  // (another cfg is refused as such, not for its missing stacks)
    CHECK(!rollout_cfg_same(again, stored));
    REFUSED(rollout_enable_plan(&again, nullptr, &f, &stored, msg), IMGENV_EINVAL, "imgenv_rollout_enable: the handle already keeps a rollout of horizon 3, final_capacity 4, fields 3");
}

static void check_minibatch() {
    FeatureFacts f = bare();
    f.roll_on = true; f.roll_horizon = 3;
    f.roll_fields = IMGENV_ROLLOUT_SENSOR_MAPS | IMGENV_ROLLOUT_VECTOR_STATES | IMGENV_ROLLOUT_NORM_REWARDS;
    imgenv_minibatch_cfg c = sized<imgenv_minibatch_cfg>();
    c.batch = 4; c.buffers = 2; c.fields = 0;
    int want = -1;
    ACCEPTED(minibatch_enable_plan(&c, nullptr, &f, nullptr, &want, msg), IMGENV_OK);
    CHECK(want == 3);  // every field the rollout stores; NORM_REWARDS names none
    c.fields = IMGENV_ROLLOUT_VECTOR_STATES;
    ACCEPTED(minibatch_enable_plan(&c, nullptr, &f, nullptr, &want, msg), IMGENV_OK);
    CHECK(want == 2);
    REFUSED(minibatch_enable_plan(&c, nullptr, nullptr, nullptr, &want, msg), IMGENV_EINVAL, "null argument");
    imgenv_minibatch_cfg bad = c;
    bad.batch = 0;
    REFUSED(minibatch_enable_plan(&bad, nullptr, nullptr, nullptr, &want, msg), IMGENV_EINVAL, "imgenv_minibatch_cfg.batch 0: at least 1");
    bad = c; bad.buffers = 5;
    REFUSED(minibatch_enable_plan(&bad, nullptr, &f, nullptr, &want, msg), IMGENV_EINVAL, "imgenv_minibatch_cfg.buffers 5: 1 .. 4");
    bad = c; bad.fields = IMGENV_ROLLOUT_NORM_REWARDS;
    REFUSED(minibatch_enable_plan(&bad, nullptr, &f, nullptr, &want, msg), IMGENV_EINVAL, "imgenv_minibatch_cfg.fields 256");
    bad.fields = IMGENV_ROLLOUT_NORM_STATES;
    REFUSED(minibatch_enable_plan(&bad, nullptr, nullptr, nullptr, &want, msg), IMGENV_EINVAL, "imgenv_minibatch_cfg.fields 128: IMGENV_ROLLOUT_NORM_* before imgenv_normalise_enable");
    REFUSED(minibatch_enable_plan(&bad, nullptr, &f, nullptr, &want, msg), IMGENV_EINVAL, "imgenv_minibatch_cfg.fields 128: IMGENV_ROLLOUT_NORM_* before imgenv_normalise_enable");
    f.norm_on = true;
    REFUSED(minibatch_enable_plan(&bad, nullptr, &f, nullptr, &want, msg), IMGENV_EINVAL, "imgenv_minibatch_cfg.fields 128: the rollout stores 259");
    bad.fields = IMGENV_ROLLOUT_LASERS;
    REFUSED(minibatch_enable_plan(&bad, nullptr, &f, nullptr, &want, msg), IMGENV_EINVAL, "imgenv_minibatch_cfg.fields 4: the rollout stores 259");
    // the rollout first -- in front of the repeated call
    FeatureFacts none = bare();
    REFUSED(minibatch_enable_plan(&c, nullptr, &none, nullptr, &want, msg), IMGENV_ESTATE, "imgenv_rollout_minibatch_enable before imgenv_rollout_enable");
    none.mb_on = true;
    REFUSED(minibatch_enable_plan(&c, nullptr, &none, &c, &want, msg), IMGENV_ESTATE, "imgenv_rollout_minibatch_enable before imgenv_rollout_enable");
    f.mb_on = true;
    const imgenv_minibatch_cfg stored = c;
    imgenv_minibatch_cfg again = c;
    CHECK(minibatch_cfg_same(again, stored));
    ACCEPTED(minibatch_enable_plan(&again, nullptr, &f, &stored, &want, msg), ENABLE_REPEAT);
    again.batch = 5;
    CHECK(!minibatch_cfg_same(again, stored));
    REFUSED(minibatch_enable_plan(&again, nullptr, &f, &stored, &want, msg), IMGENV_EINVAL,
            "imgenv_rollout_minibatch_enable: the handle already gathers minibatches of batch 4, buffers 2, fields 2");
    again = c; again.buffers = 3;
    CHECK(!minibatch_cfg_same(again, stored));
    again = c; again.fields = 0;  // (0 is compared as written, not as the bits it stands for)
    CHECK(!minibatch_cfg_same(again, stored));
}

// ---------------------------------------------------------------------------------------- the catalogue and the selection
static const void* fake(int k) { return (const void*)(uintptr_t)(4096 * (k + 1)); }
// the catalogue of a handle with 181 beams, 48 x 48 images, state_dim 3; `all`: every optional array, stacks of depth (3, 3, 2)
static void catalogue(bool all, ObsField (&f)[OBSF_COUNT]) {
    ObsFacts a;
    memset(&a, 0, sizeof(a));
    a.out.view_h = a.out.view_w = a.out.image_h = a.out.image_w = 48;
    a.out.n_beams = 181; a.out.state_dim = 3; a.out.ped_vec_len = 15;
    a.ped_image_size[0] = a.ped_image_size[1] = 48;
    a.out.vector_states = (float*)fake(0); a.out.sensor_maps = (uint16_t*)fake(1); a.out.lasers = (double*)fake(2);
    a.out.ped_vector_states = (float*)fake(3); a.out.ped_maps = (float*)fake(4); a.out.is_collisions = (int8_t*)fake(5);
    a.out.is_arrives = (uint8_t*)fake(6); a.out.step_ds = (double*)fake(7); a.out.ped_min_dists = (double*)fake(8);
    a.out.view_maps = (uint8_t*)fake(9); a.out.lasers_raw = (float*)fake(10);
    if (all) {
        a.stack.image_depth = 3; a.stack.state_depth = 3; a.stack.laser_depth = 2;
        a.stack.sensor_maps = (uint16_t*)fake(11); a.stack.vector_states = (float*)fake(12); a.stack.lasers = (double*)fake(13);
        a.ped_vector_norm = fake(14); a.norm_vector_states = fake(15); a.norm_state_stack = fake(16);
        a.norm_K = 3;
    }
    obs_fields(a, f);
}
// which member of `base` (of `bytes` bytes, all zero before) holds `p`: its offset, -1 if none or several do
static long holder(const void* base, size_t bytes, const void* p) {
    long at = -1;
    for (size_t off = 0; off + sizeof(void*) <= bytes; off += sizeof(void*)) {
        const void* v;
        memcpy(&v, (const unsigned char*)base + off, sizeof(v));
        if (v == p) at = at < 0 ? (long)off : -2;
    }
    return at;
}
struct WantField {
    int id;
    size_t row_bytes;
    long a, b;   // the member(s) the pointer lands in: final -> (out, -); rollout -> (ring, final list); minibatch -> (buffer, -)
    bool norm;   // ... of imgenv_normalise_out
};
#define FO(m) (long)offsetof(imgenv_final_obs_out, m)
#define RO(m) (long)offsetof(imgenv_rollout_out, m)
#define MB(m) (long)offsetof(imgenv_minibatch_buffer, m)
#define NO(m) (long)offsetof(imgenv_normalise_out, m)

static void check_selection(FieldFeature which, bool all, int want, const std::vector<WantField>& expect) {
    ObsField cat[OBSF_COUNT];
    catalogue(all, cat);
    FieldSelection s;
    FeatureMsg msg = "";
    CHECK(select_feature_fields(which, cat, want, want, s, msg) == IMGENV_OK && msg[0] == 0);
    CHECK(s.n == (int)expect.size());
    for (int k = 0; k < s.n && k < (int)expect.size(); k++) {
        const WantField& e = expect[(size_t)k];
        CHECK(s.id[k] == e.id);
        CHECK(s.row_bytes[k] == e.row_bytes);
        const ObsSlot& slot = OBS_SLOTS[s.id[k]];
        CHECK(slot.norm == e.norm);
        // the pointers through the catalogue into zeroed out structs: each lands in exactly the member written down here
        imgenv_final_obs_out fo = {};
        imgenv_rollout_out ro = {};
        imgenv_minibatch_buffer mb = {};
        imgenv_normalise_out no = {};
        const void *p = fake(100 + k), *q = fake(200 + k);
        const int buffer = which == FIELDS_MINIBATCH ? 2 : 0;
        if (which == FIELDS_FINAL) obs_slot_put(slot, slot.final_out, &fo, &no, (void*)p);
        if (which == FIELDS_ROLLOUT) {
            obs_slot_put(slot, slot.ring_out, &ro, &no, (void*)p);
            obs_slot_put(slot, slot.fin_out, &ro, &no, (void*)q);
        }
        if (which == FIELDS_MINIBATCH) obs_slot_put_mb(slot, &mb, &no, buffer, (void*)p);
        const void* own = which == FIELDS_FINAL ? (const void*)&fo : which == FIELDS_ROLLOUT ? (const void*)&ro : (const void*)&mb;
        const size_t own_bytes = which == FIELDS_FINAL ? sizeof(fo) : which == FIELDS_ROLLOUT ? sizeof(ro) : sizeof(mb);
        CHECK(holder(e.norm ? (const void*)&no : own, e.norm ? sizeof(no) : own_bytes, p) == e.a);
        CHECK(holder(e.norm ? own : (const void*)&no, e.norm ? own_bytes : sizeof(no), p) == -1);
        if (which == FIELDS_ROLLOUT) CHECK(holder(e.norm ? (const void*)&no : own, e.norm ? sizeof(no) : own_bytes, q) == e.b);
    }
}

static void check_catalogue() {
    CHECK(sizeof(FINAL_FIELD_ORDER) / sizeof(int) == 17 && sizeof(ROLLOUT_FIELD_ORDER) / sizeof(int) == 11);
    // the final observations: every bit, every optional array present -- the enum's order
    const std::vector<WantField> final_all = {
        {OBSF_VECTOR_STATES, 12, FO(vector_states), 0, false},
        {OBSF_SENSOR_MAPS, 4608, FO(sensor_maps), 0, false},
        {OBSF_LASERS, 1448, FO(lasers), 0, false},
        {OBSF_PED_VECTOR_STATES, 60, FO(ped_vector_states), 0, false},
        {OBSF_PED_MAPS, 27648, FO(ped_maps), 0, false},
        {OBSF_IS_COLLISIONS, 1, FO(is_collisions), 0, false},
        {OBSF_IS_ARRIVES, 1, FO(is_arrives), 0, false},
        {OBSF_STEP_DS, 8, FO(step_ds), 0, false},
        {OBSF_PED_MIN_DISTS, 8, FO(ped_min_dists), 0, false},
        {OBSF_VIEW_MAPS, 2304, FO(view_maps), 0, false},
        {OBSF_LASERS_RAW, 724, FO(lasers_raw), 0, false},
        {OBSF_STACK_SENSOR_MAPS, 13824, FO(stack_sensor_maps), 0, false},
        {OBSF_STACK_VECTOR_STATES, 36, FO(stack_vector_states), 0, false},
        {OBSF_STACK_LASERS, 2896, FO(stack_lasers), 0, false},
        {OBSF_PED_VECTOR_NORM, 60, FO(ped_vector_norm), 0, false},
        {OBSF_NORM_VECTOR_STATES, 12, NO(final_norm_vector_states), 0, true},
        {OBSF_NORM_STATE_STACK, 36, NO(final_norm_state_stack), 0, true},
    };
    check_selection(FIELDS_FINAL, true, IMGENV_FINAL_ALL | IMGENV_FINAL_NORM_STATES, final_all);
    // none present: the stacks, the pedestrian norm and the normalised states are skipped silently
    check_selection(FIELDS_FINAL, false, IMGENV_FINAL_ALL | IMGENV_FINAL_NORM_STATES, std::vector<WantField>(final_all.begin(), final_all.begin() + 11));
    check_selection(FIELDS_FINAL, true, IMGENV_FINAL_LASERS_RAW | IMGENV_FINAL_VECTOR_STATES, {final_all[0], final_all[10]});
    // the rollout: sensor_maps in front of vector_states, ped_vector_norm in front of the stacks
    const std::vector<WantField> roll_all = {
        {OBSF_SENSOR_MAPS, 4608, RO(obs_sensor_maps), RO(final_sensor_maps), false},
        {OBSF_VECTOR_STATES, 12, RO(obs_vector_states), RO(final_vector_states), false},
        {OBSF_LASERS, 1448, RO(obs_lasers), RO(final_lasers), false},
        {OBSF_PED_VECTOR_STATES, 60, RO(obs_ped_vector_states), RO(final_ped_vector_states), false},
        {OBSF_PED_MAPS, 27648, RO(obs_ped_maps), RO(final_ped_maps), false},
        {OBSF_PED_VECTOR_NORM, 60, RO(obs_ped_vector_norm), RO(final_ped_vector_norm), false},
        {OBSF_STACK_SENSOR_MAPS, 13824, RO(obs_stack_sensor_maps), RO(final_stack_sensor_maps), false},
        {OBSF_STACK_VECTOR_STATES, 36, RO(obs_stack_vector_states), RO(final_stack_vector_states), false},
        {OBSF_STACK_LASERS, 2896, RO(obs_stack_lasers), RO(final_stack_lasers), false},
        {OBSF_NORM_VECTOR_STATES, 12, NO(rollout_obs_norm_vector_states), NO(rollout_final_norm_vector_states), true},
        {OBSF_NORM_STATE_STACK, 36, NO(rollout_obs_norm_state_stack), NO(rollout_final_norm_state_stack), true},
    };
    check_selection(FIELDS_ROLLOUT, true, IMGENV_ROLLOUT_ALL | IMGENV_ROLLOUT_NORM_STATES | IMGENV_ROLLOUT_NORM_REWARDS, roll_all);
    check_selection(FIELDS_ROLLOUT, false, IMGENV_ROLLOUT_ALL | IMGENV_ROLLOUT_NORM_STATES, std::vector<WantField>(roll_all.begin(), roll_all.begin() + 5));
    check_selection(FIELDS_ROLLOUT, true, IMGENV_ROLLOUT_VECTOR_STATES | IMGENV_ROLLOUT_STACKS, {roll_all[1], roll_all[6], roll_all[7], roll_all[8]});
    // the minibatches: the same order; the normalised fields' pointers are entry `buffer` (here 2) of imgenv_normalise_out's arrays
    const std::vector<WantField> mb_all = {
        {OBSF_SENSOR_MAPS, 4608, MB(mb_sensor_maps), 0, false},
        {OBSF_VECTOR_STATES, 12, MB(mb_vector_states), 0, false},
        {OBSF_LASERS, 1448, MB(mb_lasers), 0, false},
        {OBSF_PED_VECTOR_STATES, 60, MB(mb_ped_vector_states), 0, false},
        {OBSF_PED_MAPS, 27648, MB(mb_ped_maps), 0, false},
        {OBSF_PED_VECTOR_NORM, 60, MB(mb_ped_vector_norm), 0, false},
        {OBSF_STACK_SENSOR_MAPS, 13824, MB(mb_stack_sensor_maps), 0, false},
        {OBSF_STACK_VECTOR_STATES, 36, MB(mb_stack_vector_states), 0, false},
        {OBSF_STACK_LASERS, 2896, MB(mb_stack_lasers), 0, false},
        {OBSF_NORM_VECTOR_STATES, 12, NO(mb_norm_vector_states) + 2 * (long)sizeof(void*), 0, true},
        {OBSF_NORM_STATE_STACK, 36, NO(mb_norm_state_stack) + 2 * (long)sizeof(void*), 0, true},
    };
    check_selection(FIELDS_MINIBATCH, true, IMGENV_ROLLOUT_ALL | IMGENV_ROLLOUT_NORM_STATES, mb_all);
    check_selection(FIELDS_MINIBATCH, false, IMGENV_ROLLOUT_ALL | IMGENV_ROLLOUT_NORM_STATES, std::vector<WantField>(mb_all.begin(), mb_all.begin() + 5));

    // the refusal of a required field of no bytes (no beams) or without an array; the skipped optional ones stay skipped
    ObsField cat[OBSF_COUNT];
    catalogue(false, cat);
    cat[OBSF_LASERS].row_bytes = 0;
    FieldSelection s;
    REFUSED(select_feature_fields(FIELDS_FINAL, cat, IMGENV_FINAL_ALL, IMGENV_FINAL_ALL, s, msg), IMGENV_EINVAL,
            "imgenv_final_obs_cfg.fields: bit 4 names a field of no bytes on this handle");
    REFUSED(select_feature_fields(FIELDS_ROLLOUT, cat, IMGENV_ROLLOUT_ALL, IMGENV_ROLLOUT_ALL, s, msg), IMGENV_EINVAL,
            "imgenv_rollout_cfg.fields: bit 4 names a field of no bytes on this handle");
    REFUSED(select_feature_fields(FIELDS_MINIBATCH, cat, IMGENV_ROLLOUT_ALL, IMGENV_ROLLOUT_ALL, s, msg), IMGENV_EINVAL,
            "imgenv_minibatch_cfg.fields: bit 4 names a field of no bytes on this handle");
    catalogue(false, cat);
    cat[OBSF_VIEW_MAPS].src = nullptr;
    REFUSED(select_feature_fields(FIELDS_FINAL, cat, IMGENV_FINAL_VIEW_MAPS, IMGENV_FINAL_VIEW_MAPS, s, msg), IMGENV_EINVAL,
            "imgenv_final_obs_cfg.fields: bit 512 names a field of no bytes on this handle");
    catalogue(true, cat);  // an optional field with an array of no bytes is refused too
    cat[OBSF_STACK_LASERS].row_bytes = 0;
    REFUSED(select_feature_fields(FIELDS_ROLLOUT, cat, IMGENV_ROLLOUT_STACKS, IMGENV_ROLLOUT_STACKS, s, msg), IMGENV_EINVAL,
            "imgenv_rollout_cfg.fields: bit 64 names a field of no bytes on this handle");
    // the minibatches' own refusal: the bits name nothing the ring keeps (a ring of vector_states alone, asked for its stacks)
    ObsField ring[OBSF_COUNT] = {};
    ring[OBSF_VECTOR_STATES] = {fake(0), 12};
    REFUSED(select_feature_fields(FIELDS_MINIBATCH, ring, IMGENV_ROLLOUT_STACKS, IMGENV_ROLLOUT_STACKS, s, msg), IMGENV_EINVAL,
            "imgenv_minibatch_cfg.fields 64: no field of the rollout");
    ACCEPTED(select_feature_fields(FIELDS_ROLLOUT, ring, IMGENV_ROLLOUT_STACKS, IMGENV_ROLLOUT_STACKS, s, msg), IMGENV_OK);  // (the others hand out an empty selection)
    CHECK(s.n == 0);
}

// with everything on, every enable's own cfg again is a repeated call -- but for the two that refuse any second call
static void check_everything_on() {
    const FeatureFacts f = full();
    int want = 0;
    imgenv_stack_cfg s = sized<imgenv_stack_cfg>();
    REFUSED(stack_enable_plan(&s, nullptr, &f, msg), IMGENV_ESTATE, "imgenv_stack_enable has already been called on this handle");
    imgenv_episodes_cfg e = sized<imgenv_episodes_cfg>();
    e.dt = 0.4;
    ACCEPTED(episodes_enable_plan(&e, nullptr, &f, &e, msg), ENABLE_REPEAT);
    imgenv_episode_log_cfg l = sized<imgenv_episode_log_cfg>();
    l.capacity = 8;
    ACCEPTED(episode_log_enable_plan(&l, nullptr, &f, msg), ENABLE_REPEAT);
    imgenv_policy_cfg p = sized<imgenv_policy_cfg>();
    p.flags = IMGENV_POLICY_STORE;
    ACCEPTED(policy_enable_plan(&p, nullptr, &f, &p, msg), ENABLE_REPEAT);
    imgenv_policy_loss_cfg pl = sized<imgenv_policy_loss_cfg>();
    pl.max_rows = 2;
    ACCEPTED(policy_loss_enable_plan(&pl, nullptr, &f, &pl, msg), ENABLE_REPEAT);
    const imgenv_obs_post_cfg op = post_cfg(IMGENV_OBS_PED_NORM | IMGENV_OBS_CLOSE);
    ACCEPTED(obs_post_enable_plan(&op, nullptr, &f, &op, msg), ENABLE_REPEAT);
    imgenv_normalise_cfg n = sized<imgenv_normalise_cfg>();
    n.flags = IMGENV_NORM_OBS; n.gamma = 0.99; n.clip_obs = n.clip_reward = 10.0; n.eps = 1e-8;
    REFUSED(normalise_enable_plan(&n, nullptr, &f, msg), IMGENV_EINVAL, "imgenv_normalise_enable has already been called on this handle");
    imgenv_final_obs_cfg fo = sized<imgenv_final_obs_cfg>();
    fo.fields = IMGENV_FINAL_ALL | IMGENV_FINAL_NORM_STATES;
    ACCEPTED(final_obs_enable_plan(&fo, nullptr, &f, &fo, msg), ENABLE_REPEAT);
    imgenv_rollout_cfg r = sized<imgenv_rollout_cfg>();
    r.horizon = 3; r.final_capacity = 2; r.fields = f.roll_fields;
    ACCEPTED(rollout_enable_plan(&r, nullptr, &f, &r, msg), ENABLE_REPEAT);
    imgenv_minibatch_cfg m = sized<imgenv_minibatch_cfg>();
    m.batch = 2; m.buffers = 2;
    ACCEPTED(minibatch_enable_plan(&m, nullptr, &f, &m, &want, msg), ENABLE_REPEAT);
}

int main() {
    check_everything_on();
    check_args();
    check_stack();
    check_episodes();
    check_actions();
    check_policy();
    check_obs_post();
    check_normalise();
    check_final_obs();
    check_rollout();
    check_minibatch();
    check_catalogue();
    if (n_bad) {
        printf("%d of %d checks failed\n", n_bad, n_checks);
        return 1;
    }
    printf("OK %d checks\n", n_checks);
    return 0;
}
