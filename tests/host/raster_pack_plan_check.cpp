// raster_pack_plan_check.cpp -- plan_raster_pack (img_env_amd/csrc/launch_plan.h): which chains of which handles draw their
// robots RPW to a wavefront (k_raster_pack), at which grid and LDS size; every reason it refuses for; the size threshold with its
// two neighbours; and that plan_rasters, the plan of everything it refuses, has not moved.
// The expected values are written down from DESIGN.md §5 and the comments beside the rule, not from a run of the header.
//   g++ -std=c++17 -I include tests/host/raster_pack_plan_check.cpp -o raster_pack_plan_check && ./raster_pack_plan_check
#include <stdio.h>

#include "../../img_env_amd/csrc/launch_plan.h"

// what the rule answers for the two measured shapes (the "> 4096 robots" row; docs/HISTORY.md "robot rasters, packed")
#define RASTER_PACK_HEADLINE_RPW 4  // a bitmap of 3 x 3 cells fits a segment of 16 lanes: 87.8 -> 83.5 us per step
#define RASTER_PACK_CFG5_RPW 0      // one of 5 x 5 only a segment of 32, and two robots per wavefront did not pay there

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

// a SUM handle of one world that owns it, one robot class of r = 0.17 m at 0.25 m cells: a box of 7 x 7 cells (the pedestrians'
// is no larger), a bitmap of 3 x 3, lattice rows
static PlanHandle handle(int R, int P) {
    PlanHandle h;
    h.W = 1; h.Rw = R; h.Pw = P;
    h.R = h.RL = R;
    h.P = h.NA = P;
    h.relation = 1;
    h.scene = IMGENV_SCENE_RVO;
    h.layer = LAYER_SUM;
    h.pow2 = true;
    h.n_sub = 8;
    h.box_cells = 49;
    h.robot_classes = 1;
    h.pack_rows = true;
    h.pack_bitmap_cells = 9;
    return h;
}
static PlanChain step_chain(const PlanHandle& h) {
    PlanChain c;
    c.act_nw = h.W; c.act_ng = h.R; c.act_nl = h.RL; c.act_np = h.P;
    c.act_cells = h.Gs * h.W;
    return c;
}

int main() {
    {   // the headline: 8192 robots + 200 pedestrians
        const PlanHandle h = handle(8192, 200);
        const PlanChain c = step_chain(h);
        const RasterPackPlan k = plan_raster_pack(h, c);
        CHECK_EQ(k.rpw, RASTER_PACK_HEADLINE_RPW);
        if (k.rpw) {
            CHECK_EQ(k.launch.grid, (8192 + k.rpw - 1) / k.rpw + 200);
            CHECK_EQ(k.launch.block, 64);
            CHECK_EQ(k.launch.lds, (size_t)k.rpw * (4 * 49 + 16));
        }
        // plan_rasters: as tests/host/launch_plan_check.cpp pins it
        const RasterPlan r = plan_rasters(h, c);
        CHECK_EQ(r.launch.grid, 8192);
        CHECK_EQ(r.launch.block, 64);
        CHECK_EQ(r.nw, 1);
        CHECK_EQ(r.split, 0);
        CHECK_EQ(r.move, 0);
        CHECK_EQ(r.launch.lds, 4 * 49 + 16);
        // the switch: 0 never, 2 / 4 that RPW
        for (int f : {0, 2, 4}) {
            PlanHandle hf = h;
            hf.pack_force = f;
            const RasterPackPlan kf = plan_raster_pack(hf, c);
            CHECK_EQ(kf.rpw, f);
            if (f) CHECK_EQ(kf.launch.grid, 8192 / f + 200);
            if (f) CHECK_EQ(kf.launch.lds, (size_t)f * (4 * 49 + 16));
        }
    }
    {   // cfg-5: 8192 robots + 1000 pedestrians at 0.125 m cells (box 9 x 9, bitmap 5 x 5: 25 cells fit 32 lanes, not 16)
        PlanHandle h = handle(8192, 1000);
        h.box_cells = 81;
        h.pack_bitmap_cells = 25;
        const PlanChain c = step_chain(h);
        CHECK_EQ(plan_raster_pack(h, c).rpw, RASTER_PACK_CFG5_RPW);
        h.pack_force = 2;
        CHECK_EQ(plan_raster_pack(h, c).rpw, 2);
        CHECK_EQ(plan_raster_pack(h, c).launch.grid, 4096 + 1000);
        CHECK_EQ(plan_raster_pack(h, c).launch.lds, 2 * (4 * 81 + 16));
        h.pack_force = 4;  // the bitmap does not fit a segment of 16 lanes
        CHECK_EQ(plan_raster_pack(h, c).rpw, 0);
    }
    {   // cfg-4's share of one GPU: 8192 robots beside 200 social-force pedestrians that ignore them, 0.5 m cells (box 7 x 7, bitmap 3 x 3)
        PlanHandle h = handle(8192, 200);
        h.scene = IMGENV_SCENE_PEDSIM;
        h.NA = 0;
        h.relation = 0;
        const PlanChain c = step_chain(h);
        CHECK_EQ(plan_raster_pack(h, c).rpw, 0);  // (measured slower packed: the rule leaves social-force crowds out)
        h.pack_force = 4;
        CHECK_EQ(plan_raster_pack(h, c).rpw, 4);
        CHECK_EQ(plan_raster_pack(h, c).launch.grid, 2048 + 200);
    }
    for (int R : {1024, 4096}) {  // small and roomy launches keep k_raster (with 200 pedestrians; their steps fuse the move or not)
        const PlanHandle h = handle(R, 200);
        CHECK_EQ(plan_raster_pack(h, step_chain(h)).rpw, 0);
    }
    {   // the size threshold: n_g + n_p > 8192 (what plan_rasters calls neither small nor roomy)
        for (int R : {7991, 7992, 7993}) {
            const PlanHandle h = handle(R, 200);
            const PlanChain c = step_chain(h);
            CHECK_EQ(plan_rasters(h, c).roomy, R + 200 <= 8192);
            CHECK_EQ(plan_raster_pack(h, c).rpw, R + 200 > 8192 ? RASTER_PACK_HEADLINE_RPW : 0);
        }
    }
    {   // each reason to refuse, on a handle whose switch asks for 2 on every eligible chain
        PlanHandle h = handle(70, 5);
        h.pack_force = 2;
        const PlanChain c = step_chain(h);
        CHECK_EQ(plan_raster_pack(h, c).rpw, 2);
        CHECK_EQ(plan_raster_pack(h, c).launch.grid, 35 + 5);
        { PlanHandle x = handle(7, 5); x.pack_force = 4; CHECK_EQ(plan_raster_pack(x, step_chain(x)).launch.grid, 2 + 5); }  // (the last block holds 3)
        { PlanHandle x = h; x.layer = LAYER_STAMP; CHECK_EQ(plan_raster_pack(x, c).rpw, 0); }
        { PlanHandle x = h; x.layer = LAYER_COMPOSED; CHECK_EQ(plan_raster_pack(x, c).rpw, 0); }
        { PlanHandle x = h; x.RL = 35; x.sharded = true; CHECK_EQ(plan_raster_pack(x, c).rpw, 0); }
        { PlanHandle x = h; x.RL = 35; x.sharded = x.sum_shard = true; CHECK_EQ(plan_raster_pack(x, c).rpw, 0); }
        { PlanHandle x = h; x.robot_classes = 2; CHECK_EQ(plan_raster_pack(x, c).rpw, 0); }
        { PlanHandle x = h; x.pack_rows = false; CHECK_EQ(plan_raster_pack(x, c).rpw, 0); }  // a class without rows, or a box beyond box_cells
        { PlanHandle x = h; x.pack_bitmap_cells = 33; CHECK_EQ(plan_raster_pack(x, c).rpw, 0); }
        { PlanHandle x = h; x.pack_bitmap_cells = 32; CHECK_EQ(plan_raster_pack(x, c).rpw, 2); }
        { PlanHandle x = h; x.pack_force = 4; x.pack_bitmap_cells = 17; CHECK_EQ(plan_raster_pack(x, c).rpw, 0); }
        { PlanHandle x = h; x.pack_force = 4; x.pack_bitmap_cells = 16; CHECK_EQ(plan_raster_pack(x, c).rpw, 4); }
        // LDS: RPW boxes may not cost a compute unit its 32 wavefronts -- 160 KiB / 32 = 5120 bytes, in units of 1280
        { PlanHandle x = h; x.box_cells = 636; CHECK_EQ(plan_raster_pack(x, c).rpw, 2); }   // 2 * (2544 + 16) = 5120
        { PlanHandle x = h; x.box_cells = 637; CHECK_EQ(plan_raster_pack(x, c).rpw, 0); }
        { PlanChain y = c; y.is_reset = true; CHECK_EQ(plan_raster_pack(h, y).rpw, 0); }
        { PlanChain y = c; y.listed = true; CHECK_EQ(plan_raster_pack(h, y).rpw, 0); }
        { PlanChain y = c; y.listed = y.n_dev = true; CHECK_EQ(plan_raster_pack(h, y).rpw, 0); }
        { PlanChain y = c; y.act_ng = 60; CHECK_EQ(plan_raster_pack(h, y).rpw, 0); }  // not every world
        { PlanChain y = c; y.moved = true; CHECK_EQ(plan_raster_pack(h, y).rpw, 0); }  // the fused move keeps k_move_raster
        { PlanChain y = c; y.local_only = true; CHECK_EQ(plan_raster_pack(h, y).rpw, 0); }
        { PlanHandle x = h; x.pack_force = 0; CHECK_EQ(plan_raster_pack(x, c).rpw, 0); }
        { PlanHandle x = h; x.pack_force = -1; CHECK_EQ(plan_raster_pack(x, c).rpw, 0); }  // the rule: 75 blocks are a small launch
    }
    if (g_fail) {
        printf("%d of %d checks failed\n", g_fail, g_checks);
        return 1;
    }
    printf("OK %d checks\n", g_checks);
    return 0;
}
