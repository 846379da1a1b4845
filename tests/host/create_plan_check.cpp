// What imgenv_create decides without a device (csrc/create_plan.h, csrc/out_fields.h), on the CPU.  tests/test_create_plan.py builds
// and runs this, once more under the sanitizers.
//
// Every literal below is DERIVED BY HAND from the arithmetic imgenv_create and plan_arena spelled out before these headers existed
// (each array rounded up to 256 bytes in plan_arena's order, an empty one taking one slot; the refusals' texts copied from their
// FAIL lines) -- none is printed from the code under test.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#define WAVE_SZ 64  // (host_tables.h: the .hip defines it in front of its includes)
#include "../../img_env_amd/csrc/create_plan.h"

static int n_checks = 0, n_bad = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        n_checks++;                                                  \
        if (!(cond)) {                                               \
            n_bad++;                                                 \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                            \
    } while (0)

// RL = n_robots = 4, state_dim 3, 48 x 48 view = image, 181 beams, max_ped 3, 48 x 48 ped image, 3 pedestrians, no extras
static imgenv_cfg base_cfg() {
    imgenv_cfg c;
    memset(&c, 0, sizeof(c));
    c.abi_version = IMGENV_ABI_VERSION;
    c.struct_size = (int32_t)sizeof(imgenv_cfg);
    c.view_resolution = 0.125f;
    c.global_resolution = 0.125f;
    c.view_width = 6.0f;
    c.view_height = 6.0f;
    c.step_hz = 0.4f;
    c.state_dim = 3;
    c.use_laser = 1;
    c.range_total = 181;
    c.view_angle_begin = -1.5f;
    c.view_angle_end = 1.5f;
    c.view_max_dist = 3.0f;
    c.ped_scene_type = IMGENV_SCENE_RVO;
    c.n_robots = 4;
    c.n_peds = 3;
    c.image_size[0] = c.image_size[1] = 48;
    c.ped_image_size[0] = c.ped_image_size[1] = 48;
    c.max_ped = 3;
    c.ped_vec_dim = 7;
    c.n_worlds = 1;
    return c;
}

static RobotClassHost robot_class(int box_rad, int ray_stride = 184, bool big = false) {
    RobotClassHost k;
    k.shape = IMGENV_SHAPE_CIRCLE;
    k.box_rad = box_rad;
    k.ray_stride = ray_stride;
    k.big = big;
    k.big_ta = k.big_tb = 6;
    k.fp.x.assign(40, 0.0);
    k.fp.y.assign(40, 0.0);
    return k;
}
static PedClassHost ped_class(int box_rad) {
    PedClassHost k;
    k.shape = IMGENV_SHAPE_LEG;
    k.box_rad = box_rad;
    return k;
}

// ---------------------------------------------------------------------------------------- the arena
static const char* const NAMES[32] = {"vector_states", "view_maps", "sensor_maps", "lasers_raw", "lasers", "ped_vector_states", "ped_maps",
                                      "is_collisions", "is_arrives", "step_ds", "ped_min_dists", "base_rewards", "base_dones", "rewards", "dones",
                                      "dones_info", "is_clean", "robot_pose", "ped_state", "counters", "records", "paper_rewards", "step_rewards",
                                      "step_dones", "step_dones_info", "step_is_clean", "step_is_arrives", "step_is_collisions", "step_all_down",
                                      "hits_x", "hits_y", "angular_map"};

static void check_arena(const imgenv_cfg& c, int RL, const size_t (&off)[32], size_t total, const std::vector<int>& empty) {
    const ViewGeom g = make_view_geom(c);
    const OutFacts s = out_facts(c, g.Hv, g.Wv, g.B, RL);
    const ArenaLayout l = plan_arena(s);
    OutFieldRow f[OUTF_COUNT];
    out_field_rows(s, f);
    CHECK(OUTF_COUNT == 32);
    CHECK(l.total == total);
    CHECK(l.total % 256 == 0);
    for (int q = 0; q < 32; q++) {
        CHECK(l.off[q] == off[q]);
        CHECK(l.off[q] % 256 == 0);
        CHECK(!strcmp(f[q].name, NAMES[q]));
        CHECK(f[q].guarded == (q != 20));   // exactly the records are unguarded
        CHECK(f[q].extra == (q >= 29));     // exactly hits_x, hits_y, angular_map are conditional
        CHECK(out_field_exists(s, f[q]) == (q < 29 || ((c.flags & IMGENV_FLAG_AGENT_STATE_EXTRAS) && g.B > 0)));
        const size_t end = q + 1 < 32 ? l.off[q + 1] : l.total;
        CHECK(l.off[q] + (f[q].bytes ? f[q].bytes : 1) <= end);  // no overlap: the array ends in front of the next one
        CHECK(l.slot(q) == end - l.off[q] && l.slot(q) >= 256);
    }
    for (int q : empty) CHECK(f[q].bytes == 0 && l.slot(q) == 256);  // an empty array still takes 256 bytes
}

static void arena_layouts() {
    // configuration 1.  Bytes: 48 | 9216 | 18432 | 2896 -> 3072 | 5792 -> 5888 | 352 -> 512 | 110592 | eleven arrays of at most 96 bytes,
    // ped_state 96, counters 16, records 4 * 8 * 8 = 256, eight more per-robot scalars: one slot each | three empty extras
    imgenv_cfg c = base_cfg();
    const size_t off1[32] = {0,      256,    9472,   27904,  30976,  36864,  37376,  147968, 148224, 148480, 148736,
                             148992, 149248, 149504, 149760, 150016, 150272, 150528, 150784, 151040, 151296, 151552,
                             151808, 152064, 152320, 152576, 152832, 153088, 153344, 153600, 153856, 154112};
    check_arena(c, 4, off1, 154368, {29, 30, 31});
    // configuration 2: the extras.  hits_x / hits_y 4 * 181 * 4 = 2896 -> 3072, angular_map 4 * 72 * 4 = 1152 -> 1280
    c.flags = IMGENV_FLAG_AGENT_STATE_EXTRAS;
    size_t off2[32];
    memcpy(off2, off1, sizeof(off2));
    off2[30] = 156672;
    off2[31] = 159744;
    check_arena(c, 4, off2, 161024, {});
    // configuration 3: robots [2, 5) of 8, no laser (B = 0 counts as one beam), no pedestrians (ped_state keeps one row).  Bytes:
    // 36 | 6912 | 13824 | 12 | 24 | 264 -> 512 | 82944 | thirteen slots | records 8 * 8 * 8 = 512 | eight slots | three empty extras
    c = base_cfg();
    c.n_robots = 8;
    c.robot_begin = 2;
    c.robot_end = 5;
    c.use_laser = 0;
    c.n_peds = 0;
    const size_t off3[32] = {0,      256,    7168,   20992,  21248,  21504,  22016,  104960, 105216, 105472, 105728,
                             105984, 106240, 106496, 106752, 107008, 107264, 107520, 107776, 108032, 108288, 108800,
                             109056, 109312, 109568, 109824, 110080, 110336, 110592, 110848, 111104, 111360};
    check_arena(c, 3, off3, 111616, {29, 30, 31});
    // ... and with the extras asked for but no beam to fill them: sized (one beam), but no pointer
    c.flags = IMGENV_FLAG_AGENT_STATE_EXTRAS;
    const ViewGeom g = make_view_geom(c);
    const OutFacts s = out_facts(c, g.Hv, g.Wv, g.B, 3);
    OutFieldRow f[OUTF_COUNT];
    out_field_rows(s, f);
    CHECK(f[OUTF_hits_x].bytes == 12 && f[OUTF_angular_map].bytes == 3 * 72 * 4 && !out_field_exists(s, f[OUTF_hits_x]));
}

// ---------------------------------------------------------------------------------------- layer mode and the SUM word's bits
static void layer_modes() {
    const std::vector<RobotClassHost> r5 = {robot_class(5)}, r6 = {robot_class(6)}, r5_r4 = {robot_class(5), robot_class(4)};
    const std::vector<PedClassHost> p3 = {ped_class(3)};
    // a full handle where SUM fits: 1024 robots and 200 pedestrians on 400 x 400 cells (160000 <= 512 * 1224: not stamped);
    // bits(1023) = 10, bits(200) = 8, 3 + 8 + 6 + 10 = 27
    LayerPlan l = plan_layer_mode(1024, 1024, 200, 1, 400, 400, 0, r5, p3);
    CHECK(l.sum && !l.stamp && !l.sum_shard && l.pc_bits == 8 && l.id_bits == 10);
    CHECK(l.sum_pc_mask == 255u && l.sum_rc_shift == 11u && l.sum_id_shift == 22u && l.rm_rad == 0);
    CHECK(l.sum_wg_magic == 2748779070ull);  // (2^40 + 399) / 400
    // the same in 4 worlds: the index counts within a world, bits(255) = 8, bits(50) = 6
    l = plan_layer_mode(1024, 1024, 200, 4, 200, 200, 0, r5, p3);
    CHECK(l.sum && l.pc_bits == 6 && l.id_bits == 8 && l.sum_pc_mask == 63u && l.sum_rc_shift == 9u && l.sum_id_shift == 24u);
    // past 32 bits: bits(2047) = 11, bits(8192) = 14, 3 + 14 + 6 + 11 = 34 -- the composed / stamped choice stands
    l = plan_layer_mode(2048, 2048, 8192, 1, 400, 400, 0, r5, p3);
    CHECK(!l.sum && !l.stamp && l.pc_bits == 14 && l.id_bits == 11 && l.sum_pc_mask == 0 && l.sum_rc_shift == 0 && l.sum_id_shift == 0);
    l = plan_layer_mode(2048, 2048, 8192, 1, 400, 400, IMGENV_FLAG_COMPOSE_SPARSE, r5, p3);
    CHECK(!l.sum && l.stamp);
    l = plan_layer_mode(2048, 2048, 8191, 1, 400, 400, 0, r5, p3);  // bits(8191) = 13: 33, still past
    CHECK(!l.sum && l.pc_bits == 13);
    l = plan_layer_mode(1024, 1024, 8191, 1, 400, 400, 0, r5, p3);  // bits(1023) = 10: 32, fits
    CHECK(l.sum && l.sum_id_shift == 22u && l.sum_rc_shift == 16u && l.sum_pc_mask == 8191u);
    // a shard: its own robots 1 .. RL in the index field, bits(1024) = 11; a box of 2 * 5 - 3 = 7 cells a side fits 64 bits ...
    l = plan_layer_mode(2048, 1024, 200, 1, 400, 400, 0, r5, p3);
    CHECK(l.sum && l.sum_shard && !l.stamp && l.id_bits == 11 && l.sum_id_shift == 21u && l.rm_rad == 3);
    l = plan_layer_mode(2048, 1024, 200, 1, 400, 400, 0, r5_r4, p3);  // two radii: no common bitmap
    CHECK(l.sum && l.sum_shard && l.rm_rad == -1);
    // ... one of 2 * 6 - 3 = 9 a side (81 cells) does not: SUM refused, composed (a shard never stamps)
    l = plan_layer_mode(2048, 1024, 200, 1, 400, 400, 0, r6, p3);
    CHECK(!l.sum && !l.stamp && !l.sum_shard && l.rm_rad == 0);
    l = plan_layer_mode(2048, 2048, 200, 1, 400, 400, 0, r6, p3);  // (the whole handle takes the same box)
    CHECK(l.sum);
    // the overrides.  COMPOSE_DENSE: composed where SUM would have been chosen; LAYER_SUM: SUM where the small handle would stamp
    l = plan_layer_mode(1024, 1024, 200, 1, 400, 400, IMGENV_FLAG_COMPOSE_DENSE, r5, p3);
    CHECK(!l.sum && !l.stamp);
    l = plan_layer_mode(4, 4, 3, 1, 100, 100, 0, r5, p3);
    CHECK(!l.sum && l.stamp);
    l = plan_layer_mode(4, 4, 3, 1, 100, 100, IMGENV_FLAG_LAYER_SUM, r5, p3);  // bits(3) = 2 twice
    CHECK(l.sum && !l.stamp && l.sum_pc_mask == 3u && l.sum_rc_shift == 5u && l.sum_id_shift == 30u);
    l = plan_layer_mode(4, 4, 3, 1, 100, 100, IMGENV_FLAG_LAYER_SUM | IMGENV_FLAG_COMPOSE_DENSE, r5, p3);
    CHECK(l.sum && !l.stamp);
    l = plan_layer_mode(1, 1, 0, 1, 100, 100, IMGENV_FLAG_LAYER_SUM, r5, {});  // one robot still has an index bit, no pedestrian bit
    CHECK(l.sum && l.id_bits == 1 && l.pc_bits == 0 && l.sum_pc_mask == 0u && l.sum_rc_shift == 3u && l.sum_id_shift == 31u);
    // what SUM cannot hold: a map of 2^24 cells, a big view, a footprint or pedestrian box beyond the rasters' 2048 cells (46 x 46)
    l = plan_layer_mode(4, 4, 3, 1, 4096, 4096, IMGENV_FLAG_LAYER_SUM, r5, p3);
    CHECK(!l.sum && l.stamp);
    l = plan_layer_mode(4, 4, 3, 1, 100, 100, IMGENV_FLAG_LAYER_SUM, {robot_class(5, 184, true)}, p3);
    CHECK(!l.sum);
    l = plan_layer_mode(4, 4, 3, 1, 100, 100, IMGENV_FLAG_LAYER_SUM, {robot_class(23)}, p3);  // 47 x 47 = 2209
    CHECK(!l.sum);
    l = plan_layer_mode(4, 4, 3, 1, 100, 100, IMGENV_FLAG_LAYER_SUM, {robot_class(22)}, {ped_class(23)});  // 45 x 45 = 2025 fits, the pedestrian's not
    CHECK(!l.sum);
    l = plan_layer_mode(4, 4, 3, 1, 100, 100, IMGENV_FLAG_LAYER_SUM, {robot_class(22)}, {ped_class(22)});
    CHECK(l.sum);
}

// ---------------------------------------------------------------------------------------- sub-steps, the early rule
static void sub_steps_and_early() {
    // cur = 0, 0.05, 0.1, 0.15000000000000002, 0.2, 0.25, 0.3, 0.35, 0.39999999999999997 <= 0.4f: nine rounds; 0.44999999999999996 is past
    CHECK(plan_n_sub((double)0.4f) == 9);
    CHECK(plan_n_sub((double)0.1f) == 3);   // 0, 0.05, 0.1 <= 0.10000000149
    CHECK(plan_n_sub((double)0.05f) == 2);  // 0, 0.05 <= 0.05000000074505806
    CHECK(plan_n_sub(0.0) == 1 && plan_n_sub(-1.0) == 0);
    CHECK(plan_pow2(0.125) && plan_pow2(0.5) && !plan_pow2(0.1) && !plan_pow2(0.375));
    // the early rule over every corner: not serial, pedestrians, a crowd that stands still during the step (ORCA agents or a
    // social-force crowd a step ahead), no beep lottery, no limiters, views through k_view, sub-steps that fit k_integrate's table
    for (int m = 0; m < 256; m++) {
        const bool serial = m & 1, peds = m & 2, agents = m & 4, ahead = m & 8, beep = m & 16, lim = m & 32, big = m & 64, fits = m & 128;
        const bool want = !serial && peds && (agents || ahead) && !beep && !lim && !big && fits;
        CHECK(plan_early_obs(serial, peds ? 7 : 0, agents ? 7 : 0, ahead, beep, lim, big, fits ? 9 : 31) == want);
    }
    CHECK(plan_early_obs(false, 1, 1, false, false, false, false, 30) && !plan_early_obs(false, 1, 1, false, false, false, false, 0));
    imgenv_cfg c = base_cfg();
    CHECK(!cfg_has_limiters(c));
    for (int q = 0; q < 6; q++) {
        c = base_cfg();
        int32_t* flags[6] = {&c.limiter_v.has_velocity_limits, &c.limiter_v.has_acceleration_limits, &c.limiter_v.has_jerk_limits,
                             &c.limiter_w.has_velocity_limits, &c.limiter_w.has_acceleration_limits, &c.limiter_w.has_jerk_limits};
        *flags[q] = 1;
        CHECK(cfg_has_limiters(c));
    }
}

// ---------------------------------------------------------------------------------------- the refusals
static void refused(int rc, const CreateMsg& msg, const std::string& want) {
    CHECK(rc == IMGENV_EINVAL);
    CHECK(want == msg);
    if (want != msg) printf("  got  \"%s\"\n  want \"%s\"\n", msg, want.c_str());
}
static void args_refused(const imgenv_cfg& c, const std::string& want, int Hg = 100, int Wg = 100) {
    CreateMsg msg = "";
    CreateArgs a;
    refused(create_check_args(&c, true, true, Hg, Wg, a, msg), msg, want);
}
static void plan_refused(const imgenv_cfg& c, const std::vector<RobotClassHost>& rcls, const std::vector<PedClassHost>& pcls, const std::string& want) {
    CreateMsg msg = "";
    CreateArgs a;
    CreatePlan p;
    CHECK(create_check_args(&c, true, true, 100, 100, a, msg) == IMGENV_OK);
    refused(plan_create(c, a, 100, 100, false, rcls, pcls, p, msg), msg, want);
}

static void refusals() {
    CreateMsg msg = "";
    CreateArgs a;
    imgenv_cfg c = base_cfg();
    refused(create_check_args(nullptr, true, true, 100, 100, a, msg), msg, "null argument");
    refused(create_check_args(&c, false, true, 100, 100, a, msg), msg, "null argument");
    refused(create_check_args(&c, true, false, 100, 100, a, msg), msg, "null argument");
    CHECK(create_check_args(&c, true, true, 100, 100, a, msg) == IMGENV_OK);
    CHECK(a.W == 1 && a.r0 == 0 && a.r1 == 4 && !a.beep_on && !a.view_resize && a.g.Hv == 48 && a.g.Wv == 48 && a.g.B == 181);
    c.abi_version = 1;
    args_refused(c, "imgenv_cfg ABI mismatch (version 1 size " + std::to_string(sizeof(imgenv_cfg)) + ", want 2 " + std::to_string(sizeof(imgenv_cfg)) + ")");
    c = base_cfg(); c.n_robots = 0;
    args_refused(c, "bad sizes");
    c = base_cfg();
    args_refused(c, "bad sizes", 0, 100);
    c.n_worlds = 3;
    args_refused(c, "n_robots 4 and n_peds 3 must be multiples of n_worlds 3");
    c = base_cfg(); c.n_peds = 4;
    args_refused(c, "n_peds 4 > max_ped 3 (IndexError in yaml_env.py:401)");
    c.n_peds = 65001; c.max_ped = 70000;
    args_refused(c, "more than 65000 pedestrians in one world unsupported");
    c = base_cfg(); c.n_robots = 0xFFFFFE;
    args_refused(c, "more than 2^24 - 3 robots unsupported");
    c = base_cfg(); c.image_size[1] = 0;
    args_refused(c, "bad image_size");
    c = base_cfg(); c.state_dim = 6;
    args_refused(c, "state_dim must be 3, 4 or 5");
    c = base_cfg(); c.ped_vec_dim = 6;
    args_refused(c, "ped_vec_dim must be 7");
    c = base_cfg(); c.ped_scene_type = IMGENV_SCENE_PEDSIM; c.relation_ped_robo = 1; c.n_robots = 9;
    args_refused(c, "pedscene with relation_ped_robo=1 and more than 8 robots: the reference node recurses forever in "
                    "Ttree::addAgent (all robot Tagents start at (0,0,0), ped_tree.cpp:65-96)");
    c = base_cfg(); c.ped_scene_type = IMGENV_SCENE_PEDSIM; c.n_peds = 257; c.max_ped = 300;
    args_refused(c, "pedscene crowds larger than 256 agents are not supported");
    c = base_cfg(); c.robot_begin = 5; c.robot_end = 3;
    args_refused(c, "bad robot shard [5,3)");
    c = base_cfg(); c.ped_scene_type = IMGENV_SCENE_ERVO; c.beep_r = 1.0f; c.ped_ca_p = 0.5f; c.robot_end = 2;
    args_refused(c, "beep_r / ped_ca_p > 0 in a robot shard: the beep lottery needs every robot's action on every rank");
    c = base_cfg(); c.n_worlds = 2; c.n_peds = 2; c.robot_end = 2;
    args_refused(c, "n_worlds > 1 cannot be combined with a robot shard: give each rank whole worlds (its own handle)");
    c = base_cfg(); c.view_width = 0.0f;
    args_refused(c, "view of 48 x 0 cells unsupported");
    c = base_cfg(); c.range_total = 65536;
    args_refused(c, "more than 65535 beams unsupported");

    // the grid: the resize, and the world-cell limit once, on the grid the handle works on, in its two wordings
    int Hg = 100, Wg = 60;
    c = base_cfg();
    CHECK(create_grid_size(c, 1, Hg, Wg, msg) == IMGENV_OK && Hg == 100 && Wg == 60);
    c.global_resolution = 0.25f;
    CHECK(create_grid_size(c, 1, Hg, Wg, msg) == IMGENV_OK && Hg == 200 && Wg == 120);
    c.global_resolution = 0.0f;
    refused(create_grid_size(c, 1, Hg, Wg, msg), msg, "the map would be resized to 0 x 0 cells");
    c = base_cfg();
    Hg = Wg = 46341;  // 46341^2 = 2147488281 cells, 2147488288 a copy: two copies pass 2^32
    refused(create_grid_size(c, 2, Hg, Wg, msg), msg, "n_worlds x map cells must stay below 2^32");
    CHECK(create_grid_size(c, 1, Hg, Wg, msg) == IMGENV_OK);
    Hg = Wg = 46340;  // 2147395600 cells a copy
    CHECK(create_grid_size(c, 2, Hg, Wg, msg) == IMGENV_OK);
    c.global_resolution = 0.25f;
    Hg = Wg = 18919;  // (a resized map stays below 2^31 cells, so three worlds: 37838^2 = 1431714244, 1431714256 a copy, 4295142768 in all)
    refused(create_grid_size(c, 3, Hg, Wg, msg), msg, "n_worlds x map cells must stay below 2^32 (the map is resized to 37838 x 37838 cells)");
    Hg = Wg = 23171;
    refused(create_grid_size(c, 2, Hg, Wg, msg), msg, "the map would be resized to 46342 x 46342 cells");
    c.global_resolution = 0.0625f;  // a map above the limit as given, below it as the handle works on it
    Hg = Wg = 50000;
    CHECK(create_grid_size(c, 2, Hg, Wg, msg) == IMGENV_OK && Hg == 25000 && Wg == 25000);

    // the refusals that need the class tables
    const std::vector<RobotClassHost> r5 = {robot_class(5)};
    const std::vector<PedClassHost> p3 = {ped_class(3)};
    c = base_cfg();
    const int32_t shapes[4] = {IMGENV_SHAPE_CIRCLE, 7, IMGENV_SHAPE_RECTANGLE, 9};
    c.robot_shape = shapes;
    refused(create_check_shapes(c, msg), msg, "robot 1: unsupported shape 7");
    const int32_t good[4] = {IMGENV_SHAPE_CIRCLE, IMGENV_SHAPE_RECTANGLE, IMGENV_SHAPE_RECTANGLE, IMGENV_SHAPE_CIRCLE};
    c.robot_shape = good;
    CHECK(create_check_shapes(c, msg) == IMGENV_OK);
    c = base_cfg();
    std::vector<RobotClassHost> bad = {robot_class(5), robot_class(5)};
    bad[1].ok = false;
    plan_refused(c, bad, p3, "laser ray tables overflow their packing (too many beams x view cells)");
    plan_refused(c, std::vector<RobotClassHost>(7, robot_class(5)), p3, "more than 6 robot or 4 pedestrian classes (shape, size, sensor) in one world");
    plan_refused(c, r5, std::vector<PedClassHost>(5, ped_class(3)), "more than 6 robot or 4 pedestrian classes (shape, size, sensor) in one world");
    plan_refused(c, {robot_class(5, 184, true), robot_class(5)}, p3, "robot classes with and without big views in one world");
    c.n_robots = 8; c.robot_end = 4; c.flags = IMGENV_FLAG_FULL_REWRITE;
    plan_refused(c, r5, p3, "IMGENV_FLAG_FULL_REWRITE is not available in a robot shard");
    c = base_cfg(); c.out_arena = &c; c.out_arena_bytes = 154367;
    plan_refused(c, r5, p3, "out_arena too small: 154367 < 154368");
    // taps_lds_bytes(40000) = 16 * 10001 + 16 * 256 + 32 * 256 + 16 = 172320 > 163840
    c = base_cfg(); c.range_total = 40000;
    plan_refused(c, {robot_class(5, 40000, true)}, p3, "the hit words of 40000 beams do not fit the 160 KiB LDS");
    // 20000 pedestrians: 32768 slots, LDS sort: 32768 * 8 + 20000 * 8 + 32768 * 4 + 64 * 7 * 4 + 16 = 555024; the view of 48 x 48
    // cells and 188 hit words: 2320 + 752 + 768 + 16 + 4 * (2 * 24 + 4) = 4064
    c = base_cfg(); c.n_peds = 20000; c.max_ped = 20000;
    plan_refused(c, r5, p3, "view (4064 B) or pedestrian list (555024 B) does not fit the 160 KiB LDS");
    // among themselves they keep their order: the overflowed table in front of the class count in front of the arena
    c = base_cfg(); c.out_arena = &c; c.out_arena_bytes = 1;
    std::vector<RobotClassHost> many(7, robot_class(5));
    plan_refused(c, many, p3, "more than 6 robot or 4 pedestrian classes (shape, size, sensor) in one world");
    many[6].ok = false;
    plan_refused(c, many, p3, "laser ray tables overflow their packing (too many beams x view cells)");
}

// ---------------------------------------------------------------------------------------- the smaller facts of a plan
static void plan_facts_of(const imgenv_cfg& c, int Hg, int Wg, bool serial, const std::vector<RobotClassHost>& rcls,
                          const std::vector<PedClassHost>& pcls, CreatePlan& p) {
    CreateMsg msg = "";
    CreateArgs a;
    CHECK(create_check_args(&c, true, true, Hg, Wg, a, msg) == IMGENV_OK);
    CHECK(plan_create(c, a, Hg, Wg, serial, rcls, pcls, p, msg) == IMGENV_OK);
}
static void small_facts() {
    CreatePlan p;
    imgenv_cfg c = base_cfg();
    // the small handle stamps: no pedestrian lists; box 11 x 11 = 121, 40 footprint samples; margin ceil(0.5 * sqrt(2 * 48^2)) + 5 + 3 = 42
    plan_facts_of(c, 100, 60, false, {robot_class(5)}, {ped_class(3)}, p);
    CHECK(p.R == 4 && p.RL == 4 && p.P == 3 && p.W == 1 && p.Rw == 4 && p.Pw == 3 && p.NA == 3 && p.G == 6000 && p.Gs == 6000 && p.Gp == 6000);
    CHECK(p.layer.stamp && p.box_cells == 121 && p.fp_cap == 40 && p.pd_cap == 0 && p.region_margin == 42);
    CHECK(p.pow2 && p.wv_magic == 89478486u && p.ped_res == 0.125 && p.ped_inv_res == 8.0 && p.n_sub == 9);  // (2^32 + 47) / 48
    CHECK(p.hit_stride == 188 && p.lds_view == 4064 && !p.big_view && p.big_words == 0 && p.big_hit_stride == 0 && p.big_full_chunks == 1);
    CHECK(p.PP == 64 && p.obs_E == 1 && p.obs_passes == 0 && p.lds_obs == 3 * 8 + 64 * 4 + 64 * 7 * 4 + 16);
    CHECK(p.early && !p.sfm_ahead && !p.full_rewrite && p.arena.total == 154368);
    plan_facts_of(c, 100, 60, true, {robot_class(5)}, {ped_class(3)}, p);
    CHECK(!p.early);
    // SUM: the pedestrians' 7 x 7 box joins; a footprint of 3 x 3 cells caps its list at 9; two worlds pad a copy to 16 cells
    c.flags = IMGENV_FLAG_LAYER_SUM; c.n_worlds = 2; c.n_peds = 2;
    plan_facts_of(c, 101, 61, false, {robot_class(1)}, {ped_class(3)}, p);
    CHECK(p.layer.sum && p.box_cells == 49 && p.fp_cap == 9 && p.pd_cap == 49 && p.region_margin == 38);
    CHECK(p.G == 6161 && p.Gs == 6176 && p.Gp == 12352 && p.Rw == 2 && p.Pw == 1);
    // a footprint beyond the rasters' box goes without a list
    c = base_cfg();
    plan_facts_of(c, 100, 60, false, {robot_class(23), robot_class(2)}, {ped_class(3)}, p);
    CHECK(p.box_cells == 25 && p.fp_cap == 25 && p.region_margin == 60);
    // a shrunk image: big view; 6 x 6 tiles -> (72 + 1 + 3) & ~3 = 76 words, (181 + 6) & ~3 = 184, ceil(2304 / 1024) = 3 chunks
    c.image_size[0] = c.image_size[1] = 24;
    plan_facts_of(c, 100, 60, false, {robot_class(5, 184, true)}, {ped_class(3)}, p);
    CHECK(p.view_resize && p.big_view && p.big_words == 76 && p.big_hit_stride == 184 && p.big_full_chunks == 3 && p.lds_view == 16);
    CHECK(p.big_bits_in_lds && p.lds_view_big == 4 * 76 + 16 && !p.early);
    // the pedestrians' order is kept from 128 slots on: 3 passes, 6 from 512 slots on
    c = base_cfg(); c.n_peds = 65; c.max_ped = 65;
    plan_facts_of(c, 100, 60, false, {robot_class(5)}, {ped_class(3)}, p);
    CHECK(p.PP == 128 && p.obs_E == 2 && p.obs_passes == 3);
    c.n_peds = 513; c.max_ped = 513;
    plan_facts_of(c, 100, 60, false, {robot_class(5)}, {ped_class(3)}, p);
    CHECK(p.PP == 1024 && p.obs_E == 16 && p.obs_passes == 6);
    c.n_peds = 1025; c.max_ped = 1025;
    plan_facts_of(c, 100, 60, false, {robot_class(5)}, {ped_class(3)}, p);
    CHECK(p.PP == 2048 && p.obs_E == 0 && p.obs_passes == 0);
    // a social-force crowd that ignores the robots runs a step ahead (not in a serial handle), and the early step follows it
    c = base_cfg(); c.ped_scene_type = IMGENV_SCENE_PEDSIM;
    plan_facts_of(c, 100, 60, false, {robot_class(5)}, {ped_class(3)}, p);
    CHECK(p.NA == 0 && p.sfm_ahead && p.early);
    c.relation_ped_robo = 1;
    plan_facts_of(c, 100, 60, false, {robot_class(5)}, {ped_class(3)}, p);
    CHECK(!p.sfm_ahead && !p.early);
    c = base_cfg(); c.relation_ped_robo = 1;
    plan_facts_of(c, 100, 60, false, {robot_class(5)}, {ped_class(3)}, p);
    CHECK(p.NA == 7);
}

int main() {
    arena_layouts();
    layer_modes();
    sub_steps_and_early();
    refusals();
    small_facts();
    if (n_bad) {
        printf("%d of %d checks FAILED\n", n_bad, n_checks);
        return 1;
    }
    printf("OK %d checks\n", n_checks);
    return 0;
}
