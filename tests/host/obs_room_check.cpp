// obs_room_check.cpp -- plan_obs_lds / plan_obs (img_env_amd/csrc/launch_plan.h): the LDS an early k_obs asks for so that a compute
// unit keeps room for the packed raster launch behind it.  The expected values are worked out here from the hardware's figures
// (a compute unit: 160 KiB of LDS in 1280-byte granules, 32 wavefronts), not read off a run of the header.
//   g++ -std=c++17 -I include tests/host/obs_room_check.cpp -o obs_room_check && ./obs_room_check
#include <stdio.h>

#include "../../img_env_amd/csrc/launch_plan.h"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        g_checks++;                                                      \
        if (!(cond)) {                                                   \
            g_fail++;                                                    \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
        }                                                                \
    } while (0)
#define CHECK_EQ(a, b)                                                                                     \
    do {                                                                                                   \
        g_checks++;                                                                                        \
        const long long a_ = (long long)(a), b_ = (long long)(b);                                          \
        if (a_ != b_) {                                                                                    \
            g_fail++;                                                                                      \
            printf("FAIL %s:%d: %s = %lld, expected %s = %lld\n", __FILE__, __LINE__, #a, a_, #b, b_);     \
        }                                                                                                  \
    } while (0)

static const size_t GRANULE = 1280, CU_LDS = 160 * 1024, CU_WAVES = 32;
static size_t granules(size_t bytes) { return (bytes + GRANULE - 1) / GRANULE; }
// k_obs workgroups (one wavefront each) a compute unit holds when each asks for `bytes` of LDS
static size_t obs_per_cu(size_t bytes) { return std::min(CU_WAVES, CU_LDS / GRANULE / std::max<size_t>(granules(bytes), 1)); }

// the headline handle: 8192 robots + 200 RVO pedestrians in SUM mode, one robot class with a 7 x 7 box and a 3 x 3 bitmap
static PlanHandle headline() {
    PlanHandle h;
    h.W = 1; h.Rw = 8192; h.Pw = 200;
    h.R = h.RL = 8192;
    h.P = h.NA = 200;
    h.relation = 1;
    h.scene = IMGENV_SCENE_RVO;
    h.layer = LAYER_SUM;
    h.pow2 = true;
    h.obs_E = plan_obs_E(plan_obs_slots(200));
    h.lds_obs = plan_lds_obs(h.obs_E, plan_obs_slots(200), 200);
    h.n_sub = 8;
    h.box_cells = 49;
    h.robot_classes = 1; h.pack_rows = true; h.pack_bitmap_cells = 9;
    h.early = h.gates_work = true;
    return h;
}
static PlanChain step_chain(const PlanHandle& h) {
    PlanChain c;
    c.act_nw = h.W; c.act_ng = h.R; c.act_nl = h.RL; c.act_np = h.P;
    c.orca_ran = c.view_ran = true;
    c.in_step = true;
    return c;
}

// every room from 1 to 31 at these sizes: either the size is left alone, or a compute unit full of k_obs has the room asked for
static void sweep(size_t lds_obs, size_t raster_lds) {
    for (int room = 1; room < 32; room++) {
        const size_t got = plan_obs_lds(lds_obs, 2248, raster_lds, room);
        CHECK(got <= LDS_MAX);
        if (got == lds_obs) continue;
        CHECK(got > lds_obs && got % GRANULE == 0);
        const size_t n = obs_per_cu(got);
        CHECK(n >= 1);
        CHECK(CU_WAVES - n >= (size_t)room);                                                     // wavefront slots
        CHECK(CU_LDS / GRANULE - n * granules(got) >= (size_t)room * granules(raster_lds));      // and the rasters' LDS
        // the smallest such size: one granule less does not leave the room (or is less than k_obs uses)
        if (granules(got) - 1 >= granules(lds_obs)) {
            const size_t less = got - GRANULE, m = obs_per_cu(less);
            CHECK(CU_WAVES - m < (size_t)room || CU_LDS / GRANULE - m * granules(less) < (size_t)room * granules(raster_lds));
        }
    }
}

int main() {
    PlanHandle h = headline();
    const PlanChain c = step_chain(h);
    CHECK_EQ(h.lds_obs, 4432);  // 200 x 8 + 256 x 4 + 64 x 7 x 4 + 16: four granules, 32 of them are a compute unit's whole LDS
    CHECK_EQ(obs_per_cu(h.lds_obs), 32);
    const RasterPackPlan k = plan_raster_pack(h, c);
    CHECK_EQ(k.rpw, 4);
    CHECK_EQ(k.launch.grid, 2048 + 200);
    CHECK_EQ(k.launch.lds, 4 * (4 * 49 + 16));  // 848 B: one granule

    // the switch: 0 is off, whatever follows
    CHECK_EQ(plan_obs_lds(h.lds_obs, k.launch.grid, k.launch.lds, 0), h.lds_obs);
    // nothing packed behind the observation: unchanged, whatever the switch says
    CHECK_EQ(plan_obs_lds(h.lds_obs, 0, 0, 4), h.lds_obs);
    // the steps at the headline's sizes (128 granules per compute unit; floor(128 / g) workgroups of g granules):
    // 5 granules -> 25 workgroups, 7 slots and 3 granules free; 10 -> 12, 20 slots and 8 granules; 13 -> 9, 23 slots and 11 granules
    // (11 -> 11 workgroups and 7 granules, 12 -> 10 and 8: neither has nine granules left)
    CHECK_EQ(plan_obs_lds(h.lds_obs, k.launch.grid, k.launch.lds, 1), 5 * 1280);
    CHECK_EQ(plan_obs_lds(h.lds_obs, k.launch.grid, k.launch.lds, 3), 5 * 1280);
    CHECK_EQ(plan_obs_lds(h.lds_obs, k.launch.grid, k.launch.lds, 4), 10 * 1280);  // the threshold between the first two steps ...
    CHECK_EQ(plan_obs_lds(h.lds_obs, k.launch.grid, k.launch.lds, 8), 10 * 1280);
    CHECK_EQ(plan_obs_lds(h.lds_obs, k.launch.grid, k.launch.lds, 9), 13 * 1280);  // ... and between the second and the third
    CHECK_EQ(plan_obs_lds(h.lds_obs, k.launch.grid, k.launch.lds, 32), h.lds_obs);  // a compute unit has 32 slots: nothing to plan
    sweep(h.lds_obs, k.launch.lds);
    sweep(h.lds_obs, 2 * 1280 + 1);  // rasters of three granules
    sweep(100, 848);                 // a k_obs of one granule
    sweep(70 * 1024, 848);           // ... of 56: two workgroups per compute unit already

    // plan_obs: the rule's own value without the switch, the switch's with it -- on an early step of a chain that packs, only there
    h.obs_room_force = 4;
    CHECK_EQ(plan_obs(h, c, true).lds, 10 * 1280);
    CHECK_EQ(plan_obs(h, c, true).grid, 8192);
    CHECK_EQ(plan_obs(h, c, false).lds, h.lds_obs);  // not an early step
    CHECK_EQ(plan_obs(h, c).lds, h.lds_obs);
    h.obs_room_force = -1;
    CHECK_EQ(plan_obs(h, c, true).lds, plan_obs_lds(h.lds_obs, k.launch.grid, k.launch.lds, OBS_ROOM_RULE));
    h.obs_room_force = 0;
    CHECK_EQ(plan_obs(h, c, true).lds, h.lds_obs);
    h.obs_room_force = 4;
    {   // chains and handles that refuse packing are untouched
        PlanChain r = c;
        r.is_reset = true;
        CHECK_EQ(plan_obs(h, r, true).lds, h.lds_obs);
        r = c; r.listed = true;
        CHECK_EQ(plan_obs(h, r, true).lds, h.lds_obs);
        r = c; r.n_dev = true;
        CHECK_EQ(plan_obs(h, r, true).lds, h.lds_obs);
        r = c; r.act_ng = h.R - 1;
        CHECK_EQ(plan_obs(h, r, true).lds, h.lds_obs);
        PlanHandle g = h;
        g.scene = IMGENV_SCENE_PEDSIM;  // cfg-4: a social-force crowd
        CHECK_EQ(plan_obs(g, c, true).lds, g.lds_obs);
        g = h; g.pack_bitmap_cells = 25;  // cfg-5: a 5 x 5 bitmap fits two per wavefront only
        CHECK_EQ(plan_obs(g, c, true).lds, g.lds_obs);
        g = h; g.sharded = true; g.RL = 4096;  // a robot shard
        CHECK_EQ(plan_obs(g, c, true).lds, g.lds_obs);
        g = h; g.sum_shard = true;
        CHECK_EQ(plan_obs(g, c, true).lds, g.lds_obs);
        g = h; g.layer = LAYER_COMPOSED;
        CHECK_EQ(plan_obs(g, c, true).lds, g.lds_obs);
        g = h; g.pack_force = 0;  // IMGENV_RASTER_PACK=0
        CHECK_EQ(plan_obs(g, c, true).lds, g.lds_obs);
        g = h; g.R = g.RL = g.Rw = 7992;  // 8192 robots and pedestrians together: plan_rasters' roomy launch, not packed
        PlanChain s = step_chain(g);
        CHECK_EQ(plan_obs(g, s, true).lds, g.lds_obs);
        g.R = g.RL = g.Rw = 7993;  // one more: packed
        s = step_chain(g);
        CHECK_EQ(plan_obs(g, s, true).lds, 10 * 1280);
    }
    if (g_fail) {
        printf("%d of %d checks failed\n", g_fail, g_checks);
        return 1;
    }
    printf("OK %d checks\n", g_checks);
    return 0;
}
