// field_rows_check.cpp -- what the row-copy features share, on the CPU: the chunk walk and the unit dispatch of
// img_env_amd/csrc/field_rows.h, the catalogue of capturable fields of obs_fields.h, and the block layouts of launch_plan.h
// (plan_stack, plan_final_obs_layout, plan_rollout_layout, plan_minibatch_layout, plan_normalise_layout, plan_policy_layout,
// plan_policy_loss_layout).
//   g++ -std=c++17 tests/host/field_rows_check.cpp -o check && ./check
// (also built with -fsanitize=address,undefined by tests/test_field_rows.py)
//
// The layouts' literals are the offsets of the commit before these plans existed, derived by hand from the arithmetic the enable
// functions of imgenv_hip.hip then spelled out (every array rounded up to 256 bytes, in the order written there).
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../img_env_amd/csrc/final_obs.h"
#include "../../img_env_amd/csrc/obs_fields.h"
#include "../../img_env_amd/csrc/rollout.h"

static int g_fail = 0, g_checks = 0;
#define CHECK_EQ(a, b)                                                                                     \
    do {                                                                                                   \
        g_checks++;                                                                                        \
        const long long a_ = (long long)(a), b_ = (long long)(b);                                          \
        if (a_ != b_) {                                                                                    \
            g_fail++;                                                                                      \
            printf("FAIL %s:%d: %s = %lld, expected %s = %lld\n", __FILE__, __LINE__, #a, a_, #b, b_);     \
        }                                                                                                  \
    } while (0)

// ---------------------------------------------------------------------------------------- the walk and the dispatch
// row sizes that exercise every unit: 16 (27648, 4608, 2880), 8 (1448), 4 (724, 20, 12), 2 (6), 1 (1)
static const size_t WALK_ROWS[] = {27648, 4608, 2880, 1448, 724, 20, 12, 6, 1};
static const uint32_t WALK_UNITS[] = {16, 16, 16, 8, 4, 4, 4, 2, 1};
static const int N_WALK_ROWS = 9;

// a table of type Dev (its f[] of N entries) with `n` fields in use, field k of row size WALK_ROWS[(k + shift) % 9] and marked by
// its chunk count and unit; every chunk number of the row, and the first one past it
template <typename Dev, int N>
static void walk_case(int n, int shift) {
    Dev d;
    memset(&d, 0, sizeof(d));
    std::vector<uint32_t> chunks((size_t)n);
    uint32_t cpr = 0;
    for (int k = 0; k < n; k++) {
        const FinalFieldPlan p = plan_final_field(WALK_ROWS[(k + shift) % N_WALK_ROWS]);
        CHECK_EQ(p.unit, WALK_UNITS[(k + shift) % N_WALK_ROWS]);
        d.f[k].unit = p.unit;
        d.f[k].chunks = chunks[(size_t)k] = p.chunks;
        d.f[k].src = (const unsigned char*)(uintptr_t)(256 * (k + 1));  // (which entry the walk took its copy from)
        cpr += p.chunks;
    }
    for (int k = n; k < N; k++) d.f[k].chunks = 1u << 30;  // (an entry behind n_fields is never looked at)
    size_t wrong_field = 0, wrong_chunk = 0, wrong_member = 0;
    int k = 0;
    uint32_t rel = 0;
    for (uint32_t c = 0; c <= cpr; c++, rel++) {
        // the literal walk; c == cpr stays in the last field, one chunk past its end
        while (k < n - 1 && rel >= chunks[(size_t)k]) {
            rel -= chunks[(size_t)k];
            k++;
        }
        uint32_t got = c;
        const auto f = field_walk(d.f, n, got);
        wrong_field += f.src != d.f[k].src;
        wrong_chunk += got != rel;
        wrong_member += f.unit != d.f[k].unit || f.chunks != d.f[k].chunks;
    }
    CHECK_EQ(k, n - 1);
    CHECK_EQ(rel, chunks[(size_t)n - 1] + 1);
    CHECK_EQ(wrong_field, 0);
    CHECK_EQ(wrong_chunk, 0);
    CHECK_EQ(wrong_member, 0);
}

template <int MIN_UNIT>
static void dispatch_case(uint32_t unit, size_t want_size) {
    size_t size = 0, align = 0;
    int calls = 0;
    field_dispatch<MIN_UNIT>(unit, [&](auto chunk) {
        typedef typename decltype(chunk)::type T;
        size = sizeof(T);
        align = alignof(T);
        calls++;
    });
    CHECK_EQ(calls, 1);
    CHECK_EQ(size, want_size);
    CHECK_EQ(align, want_size);
}

static void check_walk() {
    static_assert(FINAL_MAX_FIELDS == 18 && ROLLOUT_TABLE_FIELDS == 11, "the full tables of this check");
    for (int shift = 0; shift < N_WALK_ROWS; shift++) {
        walk_case<FinalObsDev, FINAL_MAX_FIELDS>(FINAL_MAX_FIELDS, shift);  // filled to the last entry
        walk_case<RolloutDev, ROLLOUT_TABLE_FIELDS>(ROLLOUT_TABLE_FIELDS, shift);
        walk_case<FinalObsDev, FINAL_MAX_FIELDS>(1, shift);
        walk_case<FinalObsDev, FINAL_MAX_FIELDS>(2, shift);
        walk_case<RolloutDev, ROLLOUT_TABLE_FIELDS>(1, shift);
        walk_case<RolloutDev, ROLLOUT_TABLE_FIELDS>(2, shift);
    }
    for (uint32_t unit : {16u, 8u, 4u, 2u, 1u}) dispatch_case<1>(unit, unit);
    for (uint32_t unit : {16u, 8u, 4u, 2u}) dispatch_case<2>(unit, unit);
}

// ---------------------------------------------------------------------------------------- the catalogue and the selection
static const void* fake(int k) { return (const void*)(uintptr_t)(4096 * (k + 1)); }

// a handle of 181 beams, a 48 x 48 view, image and pedestrian image, ped_vec_len 15; `all`: stacks of depth (3, 3, 2), the
// pedestrian norm and the normalised states with a stack of depth 3
static ObsFacts facts(int state_dim, bool all) {
    ObsFacts a;
    memset(&a, 0, sizeof(a));
    a.out.view_h = a.out.view_w = a.out.image_h = a.out.image_w = 48;
    a.out.n_beams = 181;
    a.out.state_dim = state_dim;
    a.out.ped_vec_len = 15;
    a.ped_image_size[0] = a.ped_image_size[1] = 48;
    a.out.vector_states = (float*)fake(0);
    a.out.sensor_maps = (uint16_t*)fake(1);
    a.out.lasers = (double*)fake(2);
    a.out.ped_vector_states = (float*)fake(3);
    a.out.ped_maps = (float*)fake(4);
    a.out.is_collisions = (int8_t*)fake(5);
    a.out.is_arrives = (uint8_t*)fake(6);
    a.out.step_ds = (double*)fake(7);
    a.out.ped_min_dists = (double*)fake(8);
    a.out.view_maps = (uint8_t*)fake(9);
    a.out.lasers_raw = (float*)fake(10);
    if (all) {
        a.stack.image_depth = 3; a.stack.state_depth = 3; a.stack.laser_depth = 2;
        a.stack.sensor_maps = (uint16_t*)fake(11);
        a.stack.vector_states = (float*)fake(12);
        a.stack.lasers = (double*)fake(13);
        a.ped_vector_norm = fake(14);
        a.norm_vector_states = fake(15);
        a.norm_state_stack = fake(16);
        a.norm_K = 3;
    }
    return a;
}

struct Want {
    int bit, id;
};

static void check_catalogue() {
    CHECK_EQ(OBSF_COUNT, 17);
    ObsField f[OBSF_COUNT];
    // every optional array present, state_dim 3 and 5
    static const size_t ROWS3[OBSF_COUNT] = {12, 4608, 1448, 60, 27648, 1, 1, 8, 8, 2304, 724, 13824, 36, 2896, 60, 12, 36};
    static const size_t ROWS5[OBSF_COUNT] = {20, 4608, 1448, 60, 27648, 1, 1, 8, 8, 2304, 724, 13824, 60, 2896, 60, 20, 60};
    obs_fields(facts(3, true), f);
    for (int k = 0; k < OBSF_COUNT; k++) {
        CHECK_EQ(f[k].row_bytes, ROWS3[k]);
        CHECK_EQ((uintptr_t)f[k].src, (uintptr_t)fake(k));
    }
    obs_fields(facts(5, true), f);
    for (int k = 0; k < OBSF_COUNT; k++) CHECK_EQ(f[k].row_bytes, ROWS5[k]);
    // none present: the eleven of imgenv_out as before, no array behind them
    obs_fields(facts(3, false), f);
    for (int k = 0; k < OBSF_COUNT; k++) {
        CHECK_EQ((uintptr_t)f[k].src, k < OBSF_FIRST_OPTIONAL ? (uintptr_t)fake(k) : 0);
        if (k < OBSF_FIRST_OPTIONAL) CHECK_EQ(f[k].row_bytes, ROWS3[k]);
    }
    CHECK_EQ(f[OBSF_STACK_SENSOR_MAPS].row_bytes, 0);
    CHECK_EQ(f[OBSF_STACK_VECTOR_STATES].row_bytes, 0);
    CHECK_EQ(f[OBSF_STACK_LASERS].row_bytes, 0);
    CHECK_EQ(f[OBSF_NORM_STATE_STACK].row_bytes, 0);
    // a stack of depth 1 is the field itself: no array of its own, whatever its pointer
    ObsFacts one = facts(3, true);
    one.stack.image_depth = 1;
    obs_fields(one, f);
    CHECK_EQ((uintptr_t)f[OBSF_STACK_SENSOR_MAPS].src, 0);
    CHECK_EQ(f[OBSF_STACK_SENSOR_MAPS].row_bytes, 4608);
    CHECK_EQ((uintptr_t)f[OBSF_STACK_VECTOR_STATES].src, (uintptr_t)fake(12));

    // the selection: a feature's order, not the catalogue's
    const Want list[] = {{1, OBSF_SENSOR_MAPS},        {2, OBSF_VECTOR_STATES},  {4, OBSF_LASERS},          {8, OBSF_STACK_SENSOR_MAPS},
                         {8, OBSF_STACK_VECTOR_STATES}, {8, OBSF_STACK_LASERS},   {16, OBSF_PED_VECTOR_NORM}, {32, OBSF_NORM_VECTOR_STATES},
                         {32, OBSF_NORM_STATE_STACK}};
    const Want* sel[9];
    int bad = 0;
    obs_fields(facts(3, true), f);
    CHECK_EQ(obs_fields_select(f, list, 63, sel, &bad), 9);
    for (int k = 0; k < 9; k++) CHECK_EQ(sel[k] - list, k);
    CHECK_EQ(obs_fields_select(f, list, 2 | 8, sel, &bad), 4);
    CHECK_EQ(sel[0]->id, OBSF_VECTOR_STATES);
    CHECK_EQ(sel[3]->id, OBSF_STACK_LASERS);
    CHECK_EQ(obs_fields_select(f, list, 0, sel, &bad), 0);
    // the silent skip: the stacks, the pedestrian norm and the normalised states of a handle that has none; one stack of three
    obs_fields(facts(3, false), f);
    CHECK_EQ(obs_fields_select(f, list, 63, sel, &bad), 3);
    CHECK_EQ(sel[2]->id, OBSF_LASERS);
    CHECK_EQ(obs_fields_select(f, list, 8 | 16 | 32, sel, &bad), 0);
    obs_fields(one, f);
    CHECK_EQ(obs_fields_select(f, list, 8, sel, &bad), 2);
    CHECK_EQ(sel[0]->id, OBSF_STACK_VECTOR_STATES);
    // the refusal: a field of imgenv_out of no bytes (no beams), or without an array
    ObsFacts blind = facts(3, true);
    blind.out.n_beams = 0;
    blind.stack.laser_depth = 0;  // (imgenv_stack_out: no laser stack on a handle without lasers, whatever laser_batch says)
    blind.stack.lasers = nullptr;
    obs_fields(blind, f);
    CHECK_EQ(f[OBSF_LASERS].row_bytes, 0);
    CHECK_EQ(f[OBSF_LASERS_RAW].row_bytes, 0);
    CHECK_EQ(obs_fields_select(f, list, 63, sel, &bad), -1);
    CHECK_EQ(bad, 4);
    CHECK_EQ(obs_fields_select(f, list, 63 & ~4, sel, &bad), 7);  // (the laser stack it lacks is skipped)
    blind.stack.lasers = (double*)fake(13);                        // an optional field with an array of no bytes is refused too
    blind.stack.laser_depth = 2;
    obs_fields(blind, f);
    CHECK_EQ(obs_fields_select(f, list, 8, sel, &bad), -1);
    CHECK_EQ(bad, 8);
    ObsFacts gone = facts(3, true);
    gone.out.sensor_maps = nullptr;
    obs_fields(gone, f);
    bad = 0;
    CHECK_EQ(obs_fields_select(f, list, 1, sel, &bad), -1);
    CHECK_EQ(bad, 1);
}

// ---------------------------------------------------------------------------------------- the layouts
// the arrays of a block: (offset, bytes).  Every offset a multiple of 256, no two arrays of any bytes overlapping, all within total
static void check_block(std::vector<std::pair<size_t, size_t>> arrays, size_t total) {
    size_t unaligned = 0, overlapping = 0;
    for (const auto& a : arrays) unaligned += a.first % 256 != 0;
    arrays.erase(std::remove_if(arrays.begin(), arrays.end(), [](const std::pair<size_t, size_t>& a) { return a.second == 0; }), arrays.end());
    std::sort(arrays.begin(), arrays.end());
    for (size_t k = 0; k < arrays.size(); k++)
        overlapping += arrays[k].first + arrays[k].second > (k + 1 < arrays.size() ? arrays[k + 1].first : total);
    CHECK_EQ(unaligned, 0);
    CHECK_EQ(overlapping, 0);
    CHECK_EQ(total % 256, 0);
}

struct Shape {
    size_t RL;
    int D;
    size_t stack[4];                                // three offsets, total
    size_t final_rows[17], final_off[19];           // count, 17 fields, total
    size_t roll_rows[11], roll_ring[11], roll_fin[11], roll_rest[10];  // nine arrays, total
    size_t mb_head[8], mb_field[2][11], mb_scalar[2][7], mb_total;
    size_t norm_all[8], norm_obs[8], norm_rew[8];   // seven arrays, total: obs + reward with a stack of 3; obs alone; reward alone
};
// 181 beams, 48 x 48 image, view and pedestrian image, ped_vec_len 15, stacks of depth (3, 3, 2), T = 3, F = 4, batch 4, 2 buffers
static const Shape SHAPES[2] = {
    {4, 3,
     {0, 55296, 55552, 67328},
     {12, 4608, 1448, 60, 27648, 1, 1, 8, 8, 2304, 724, 13824, 36, 2896, 60, 12, 36},
     {0, 256, 512, 18944, 24832, 25088, 135680, 135936, 136192, 136448, 136704, 145920, 148992, 204288, 204544, 216320, 216576, 216832, 217088},
     {4608, 12, 1448, 60, 27648, 60, 13824, 36, 2896, 12, 36},
     {0, 92160, 92672, 121856, 123136, 676096, 677376, 953856, 954880, 1012992, 1013504},
     {73728, 92416, 115968, 122880, 565504, 677120, 898560, 954624, 1001216, 1013248, 1014272},
     {1014528, 1014784, 1015040, 1015296, 1015552, 1015808, 1016064, 1016320, 1016576, 1016832},
     {0, 256, 512, 768, 1024, 1280, 1536, 1792},
     {{2048, 38912, 39424, 51200, 51712, 272896, 273408, 384000, 384512, 408064, 408576},
      {20480, 39168, 45312, 51456, 162304, 273152, 328704, 384256, 396288, 408320, 408832}},
     {{409088, 409600, 410112, 410624, 411136, 411648, 412160}, {409344, 409856, 410368, 410880, 411392, 411904, 412416}},
     412672,
     {0, 256, 512, 768, 1024, 1280, 1536, 1792},
     {0, 256, 256, 512, 768, 1024, 1024, 1024},
     {0, 256, 512, 768, 1024, 1024, 1024, 1280}},
    {5, 5,
     {0, 69120, 69632, 84224},
     {20, 4608, 1448, 60, 27648, 1, 1, 8, 8, 2304, 724, 13824, 60, 2896, 60, 20, 60},
     {0, 256, 512, 23552, 30976, 31488, 169728, 169984, 170240, 170496, 170752, 182272, 186112, 255232, 255744, 270336, 270848, 271104, 271616},
     {4608, 20, 1448, 60, 27648, 60, 13824, 60, 2896, 20, 60},
     {0, 110592, 111360, 146432, 147968, 811520, 813056, 1144832, 1146368, 1216256, 1217024},
     {92160, 111104, 140544, 147712, 700928, 812800, 1089536, 1146112, 1204480, 1216768, 1218304},
     {1218560, 1218816, 1219072, 1219328, 1219584, 1219840, 1220096, 1220352, 1220608, 1220864},
     {0, 256, 512, 768, 1024, 1280, 1536, 1792},
     {{2048, 38912, 39424, 51200, 51712, 272896, 273408, 384000, 384512, 408064, 408576},
      {20480, 39168, 45312, 51456, 162304, 273152, 328704, 384256, 396288, 408320, 408832}},
     {{409088, 409600, 410112, 410624, 411136, 411648, 412160}, {409344, 409856, 410368, 410880, 411392, 411904, 412416}},
     412672,
     {0, 256, 512, 768, 1024, 1280, 1792, 2048},
     {0, 256, 256, 512, 768, 1024, 1024, 1024},
     {0, 256, 512, 768, 1024, 1024, 1024, 1280}},
};

static void check_normalise(const Shape& s, int K, bool obs, bool rew, const size_t* want) {
    const size_t RL = s.RL, D = (size_t)s.D;
    const NormaliseLayout l = plan_normalise_layout(RL, s.D, K, obs, rew);
    const size_t got[8] = {l.stats, l.returns, l.part, l.part_n, l.norm_vector_states, l.norm_state_stack, l.norm_rewards, l.total};
    for (int k = 0; k < 8; k++) CHECK_EQ(got[k], want[k]);
    // (one tile of rows at these sizes: the partial sums are 16 bytes per column, the observed states and the return)
    const size_t cols = (obs ? D : 0) + (rew ? 1 : 0);
    check_block({{l.stats, 2 * (4 + 2 * D) * 8}, {l.returns, rew ? 2 * RL * 8 : 0}, {l.part, cols * 16}, {l.part_n, 4},
                 {l.norm_vector_states, obs ? RL * D * 4 : 0}, {l.norm_state_stack, (size_t)K * RL * D * 4}, {l.norm_rewards, rew ? RL * 8 : 0}},
                l.total);
}

static void check_layouts() {
    const size_t T = 3, F = 4, B = 4, NB = 2;
    for (const Shape& s : SHAPES) {
        const size_t RL = s.RL;
        {   // the stacks: depths (3, 3, 2) from batches (3, 3, 2); a depth of 1 or 0 takes no room
            const StackPlan p = plan_stack(48 * 48, s.D, 181, 3, 3, 2, RL);
            for (int k = 0; k < 3; k++) CHECK_EQ(p.off[k], s.stack[k]);
            CHECK_EQ(p.total, s.stack[3]);
            CHECK_EQ(p.depth[0], 3); CHECK_EQ(p.depth[1], 3); CHECK_EQ(p.depth[2], 2);
            CHECK_EQ(p.frame_bytes[0], 4608); CHECK_EQ(p.frame_bytes[1], 4 * s.D); CHECK_EQ(p.frame_bytes[2], 1448);
            check_block({{p.off[0], RL * 3 * 4608}, {p.off[1], RL * 3 * 4 * (size_t)s.D}, {p.off[2], RL * 2 * 1448}}, p.total);
            const StackPlan q = plan_stack(48 * 48, s.D, 181, 1, 0, 0, RL);
            CHECK_EQ(q.total, 0);
            CHECK_EQ(q.depth[0], 1); CHECK_EQ(q.depth[1], 0); CHECK_EQ(q.depth[2], 1);  // (laser_batch 0 is a depth of 1; below 0: none)
            CHECK_EQ(plan_stack(48 * 48, s.D, 181, 0, 0, -1, RL).depth[2], 0);
            CHECK_EQ(plan_stack(48 * 48, s.D, 0, 0, 0, 4, RL).depth[2], 0);
            const StackPlan r = plan_stack(48 * 48, s.D, 181, 1, 2, 0, RL);  // only the states are deep
            CHECK_EQ(r.off[1], 0);
            CHECK_EQ(r.total, (RL * 2 * 4 * (size_t)s.D + 255) / 256 * 256);
        }
        {   // the final observations: every field
            const FinalObsLayout l = plan_final_obs_layout(s.final_rows, 17, RL);
            std::vector<std::pair<size_t, size_t>> arrays = {{l.count, 4 * RL}};
            CHECK_EQ(l.count, s.final_off[0]);
            for (int k = 0; k < 17; k++) {
                CHECK_EQ(l.field[k], s.final_off[k + 1]);
                arrays.push_back({l.field[k], RL * s.final_rows[k]});
            }
            CHECK_EQ(l.total, s.final_off[18]);
            check_block(arrays, l.total);
        }
        {   // the rollout: every field
            const RolloutLayout l = plan_rollout_layout(s.roll_rows, 11, RL, T, F);
            std::vector<std::pair<size_t, size_t>> arrays;
            for (int k = 0; k < 11; k++) {
                CHECK_EQ(l.ring[k], s.roll_ring[k]);
                CHECK_EQ(l.fin[k], s.roll_fin[k]);
                arrays.push_back({l.ring[k], (T + 1) * RL * s.roll_rows[k]});
                arrays.push_back({l.fin[k], F * s.roll_rows[k]});
            }
            const size_t got[10] = {l.actions, l.rewards, l.dones, l.is_clean, l.dones_info, l.final_idx, l.final_slot, l.final_row, l.final_n, l.total};
            const size_t bytes[9] = {T * RL * 12, T * RL * 4, T * RL, T * RL, T * RL * 4, (T + 1) * RL * 4, F * 4, F * 4, 8};
            for (int k = 0; k < 10; k++) CHECK_EQ(got[k], s.roll_rest[k]);
            for (int k = 0; k < 9; k++) arrays.push_back({got[k], bytes[k]});
            check_block(arrays, l.total);
        }
        {   // the minibatches: every field of the ring, batch 4, 2 buffers
            const MinibatchLayout l = plan_minibatch_layout(s.roll_rows, 11, RL, T, B, NB);
            const size_t head[8] = {l.valid, l.order, l.valid_n, l.norm, l.tile_count, l.tile_base, l.stat_part, l.stat_mean};
            const size_t head_bytes[8] = {T * RL * 4, T * RL * 4, 4, 8, 4, 4, 8, 8};  // (one tile at these sizes)
            const size_t scalar_bytes[7] = {B * 12, B * 4, B, B * 4, B * 4, B * 4, B * 4 * 6};
            std::vector<std::pair<size_t, size_t>> arrays;
            for (int k = 0; k < 8; k++) {
                CHECK_EQ(head[k], s.mb_head[k]);
                arrays.push_back({head[k], head_bytes[k]});
            }
            for (size_t b = 0; b < NB; b++) {
                for (int k = 0; k < 11; k++) {
                    CHECK_EQ(l.field[b][k], s.mb_field[b][k]);
                    arrays.push_back({l.field[b][k], B * s.roll_rows[k]});
                }
                for (int q = 0; q < 7; q++) {
                    CHECK_EQ(l.scalar[b][q], s.mb_scalar[b][q]);
                    arrays.push_back({l.scalar[b][q], scalar_bytes[q]});
                }
            }
            CHECK_EQ(l.total, s.mb_total);
            check_block(arrays, l.total);
        }
        check_normalise(s, 3, true, true, s.norm_all);
        check_normalise(s, 0, true, false, s.norm_obs);
        check_normalise(s, 0, false, true, s.norm_rew);
    }
}

// The policy head's and the PPO loss's blocks.  The literals are the offsets of the commit before plan_policy_layout and
// plan_policy_loss_layout existed, derived by hand from the cv.take lines imgenv_policy_enable and imgenv_policy_loss_enable then
// spelled out (each array rounded up to 256 bytes, in the order written there; an array of no bytes sits at the next one's offset).
static void check_policy_layouts() {
    const size_t RL = 4, T = 3;
    struct PolicyCase {
        bool cat;
        size_t cols, T;
        size_t want[8];  // index, raw, logp, entropy, pol_raw, pol_logp, pol_value, total
        size_t bytes[7];
    };
    const PolicyCase policy[4] = {
        // categorical, A = 11: index [RL] i32 and no raw sample; without STORE nothing behind entropy
        {true, 1, 0, {0, 256, 256, 512, 768, 768, 768, 768}, {16, 0, 16, 16, 0, 0, 0}},
        // with STORE: pol_raw [1][T][RL], pol_logp [T][RL], pol_value [T + 1][RL]
        {true, 1, T, {0, 256, 256, 512, 768, 1024, 1280, 1536}, {16, 0, 16, 16, 48, 48, 64}},
        // Gaussian, C = 2: raw [RL][2] and no index
        {false, 2, 0, {0, 0, 256, 512, 768, 768, 768, 768}, {0, 32, 16, 16, 0, 0, 0}},
        {false, 2, T, {0, 0, 256, 512, 768, 1024, 1280, 1536}, {0, 32, 16, 16, 96, 48, 64}},
    };
    for (const PolicyCase& c : policy) {
        const PolicyLayout l = plan_policy_layout(c.cat, c.cols, RL, c.T);
        const size_t got[8] = {l.index, l.raw, l.logp, l.entropy, l.pol_raw, l.pol_logp, l.pol_value, l.total};
        std::vector<std::pair<size_t, size_t>> arrays;
        for (int k = 0; k < 8; k++) CHECK_EQ(got[k], c.want[k]);
        for (int k = 0; k < 7; k++) arrays.push_back({got[k], c.bytes[k]});
        check_block(arrays, l.total);
    }
    // the loss: max_rows 5; one workgroup's record (PLOSS_REC = 10 float64) at these sizes
    const size_t B = 5, REC = 10;
    struct LossCase {
        bool cat;
        int n;
        size_t want[18];  // logp, entropy, ratio, pg, vl, d_params, d_log_std, d_log_std_shared, d_values, stats, n_bad, inv_w,
                          // row_m, row_log_s, row_gu, row_w, rec, total
        size_t bytes[17];
    };
    const LossCase loss[2] = {
        {true, 11,
         {0, 256, 512, 768, 1024, 1280, 1536, 1536, 1536, 1792, 2048, 2304, 2560, 2816, 3072, 3328, 3584, 3840},
         {20, 20, 20, 20, 20, 220, 0, 0, 20, 32, 4, 4, 20, 20, 20, 20, 80}},
        {false, 2,
         {0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 2560, 2816, 3072, 3072, 3072, 3328, 3584, 3840},
         {20, 20, 20, 20, 20, 40, 40, 8, 20, 32, 4, 4, 0, 0, 20, 20, 80}},
    };
    for (const LossCase& c : loss) {
        const size_t n_rec = plan_policy_loss_launch((int)B, c.cat ? c.n : 0).grid;
        CHECK_EQ(n_rec, 1);
        const PolicyLossLayout l = plan_policy_loss_layout(c.cat, B, (size_t)c.n, n_rec, REC);
        const size_t got[18] = {l.logp, l.entropy, l.ratio, l.pg, l.vl, l.d_params, l.d_log_std, l.d_log_std_shared, l.d_values, l.stats, l.n_bad, l.inv_w,
                                l.row_m, l.row_log_s, l.row_gu, l.row_w, l.rec, l.total};
        std::vector<std::pair<size_t, size_t>> arrays;
        for (int k = 0; k < 18; k++) CHECK_EQ(got[k], c.want[k]);
        for (int k = 0; k < 17; k++) arrays.push_back({got[k], c.bytes[k]});
        check_block(arrays, l.total);
    }
}

int main() {
    check_walk();
    check_catalogue();
    check_layouts();
    check_policy_layouts();
    if (g_fail) {
        printf("%d of %d checks failed\n", g_fail, g_checks);
        return 1;
    }
    printf("OK %d checks\n", g_checks);
    return 0;
}
