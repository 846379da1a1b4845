// launch_plan_check.cpp -- the launch-shape rules (img_env_amd/csrc/launch_plan.h) against what the project's documents say
// about them: the table of DESIGN.md §5, the measurement comments that travel with each threshold, and the docstrings of
// tests/test_gpu_large_launches.py, which pick their shapes to cross these thresholds.  Every threshold with its two
// neighbours: a threshold that moves fails here instead of silently changing what the GPU suite covers.
// The expected values are written down from those documents, not from a run of the header.
//   g++ -std=c++17 -I include tests/host/launch_plan_check.cpp -o launch_plan_check && ./launch_plan_check
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

// a handle of W worlds x (Rw robots + Pw pedestrians) that owns all of them; an RVO crowd that sees the robots; a 48 x 48-cell
// view of 360 beams (5 KB of LDS: "at 48 x 48 cells, 5 KB and 32 workgroups per unit")
static PlanHandle handle(int W, int Rw, int Pw, int layer) {
    PlanHandle h;
    h.W = W; h.Rw = Rw; h.Pw = Pw;
    h.R = h.RL = W * Rw;
    h.P = h.NA = W * Pw;
    h.relation = 1;
    h.scene = IMGENV_SCENE_RVO;
    h.layer = layer;
    h.pow2 = true; h.view_a4 = true;
    h.B = 360;
    h.lds_view = 5 * 1024;
    h.obs_E = plan_obs_E(plan_obs_slots(Pw));
    h.lds_obs = plan_lds_obs(h.obs_E, plan_obs_slots(Pw), Pw);
    h.n_sub = 8;
    h.Gs = 120 * 120;
    h.box_cells = 81;
    h.early = Pw > 0;
    h.gates_work = true;
    return h;
}
// a chain over every world of the handle: a step (is_reset 0) or imgenv_reset
static PlanChain all_worlds(const PlanHandle& h, bool is_reset) {
    PlanChain c;
    c.act_nw = h.W; c.act_ng = h.R; c.act_nl = h.RL; c.act_np = h.P;
    c.act_cells = h.Gs * h.W;
    c.is_reset = is_reset;
    c.orca_ran = c.view_ran = true;  // (not the first step behind the first reset)
    c.in_step = !is_reset;
    return c;
}
// the reset of n listed worlds
static PlanChain listed(const PlanHandle& h, int n) {
    PlanChain c = all_worlds(h, true);
    c.listed = true;
    c.act_nw = n; c.act_ng = c.act_nl = n * h.Rw; c.act_np = n * h.Pw;
    return c;
}

static void headline() {  // 8192 robots + 200 RVO pedestrians, 48^2 / 360 beams
    PlanHandle h = handle(1, 8192, 200, LAYER_SUM);
    const PlanChain c = all_worlds(h, false);
    const RasterPlan r = plan_rasters(h, c);
    CHECK(!r.move);  // k_raster
    CHECK_EQ(r.nw, 1);
    CHECK_EQ(r.split, 0);  // "the headline's 8192 + 200 stay as they are: a second, nearly empty round"
    CHECK_EQ(r.launch.grid, 8192);
    CHECK_EQ(r.launch.block, 64);
    CHECK(!r.sweep);
    CHECK_EQ(plan_views(h, c).nw, 1);
    CHECK_EQ(plan_views(h, c).view.grid, 8192);
    CHECK(!plan_views(h, c).lds_bound);  // "at 48 x 48 cells, 5 KB and 32 workgroups per unit, it loses"
    const SidePlan s = plan_side(h, c);
    CHECK(s.overlap && !s.one_side);  // two side streams
    CHECK(!s.fold_side);
    CHECK_EQ(s.slices, 4);            // "8192 robots x 200 pedestrians = 128 x 4 wavefronts"
    CHECK_EQ(s.robots.grid, 128 * 4);
    CHECK(s.orca && s.L.G == 4 && s.L.groups == 50 && s.orca_blocks == 50);
    CHECK(!s.state && !s.remote_only);
    const StepPlan sp = plan_step(h, c);
    CHECK(!sp.fuse_move && !sp.serial_move);
    CHECK(sp.early_step);             // "early k_obs where eligible"
    CHECK(sp.fork_on_move);
    CHECK_EQ(sp.nb_robot, 256);       // 32 robots per 256-thread block
    CHECK_EQ(sp.move.grid, 257);      // + one block for 200 pedestrians
    CHECK_EQ(sp.move.block, 256);
    CHECK_EQ(h.obs_E, 4);             // 200 pedestrians: 256 slots, 4 per lane
    CHECK_EQ(plan_obs(h, c).grid, 8192);
    // the first step behind the first reset has no snapshots to read; a half-way chain or a closed gate keep k_obs behind the move
    PlanChain c2 = c;
    c2.view_ran = false;
    CHECK(!plan_step(h, c2).early_step);
    c2 = c; c2.orca_ran = false;
    CHECK(!plan_step(h, c2).early_step);
    c2 = c; c2.chain_open = true;
    CHECK(!plan_step(h, c2).early_step && !plan_step(h, c2).fork_on_move);
    c2 = c; c2.early_off = true;
    CHECK(!plan_step(h, c2).early_step);
    h.gates_work = false;
    CHECK(!plan_step(h, c).early_step);
    h.gates_work = true; h.serial = true;
    CHECK(!plan_step(h, c).fork_on_move && !plan_side(h, c).overlap && !plan_side(h, c).one_side);
}

static void cfg2() {  // 1024 robots, no pedestrians
    const PlanHandle h = handle(1, 1024, 0, LAYER_STAMP);
    PlanChain c = all_worlds(h, false);
    // "cfg-2, 1024 robots at 156 cells per agent": STAMP although dense, because rasters and views are single small launches
    CHECK(plan_layer_stamp(true, (size_t)156 * 1024, 1024, 0, 0));
    CHECK(!plan_layer_stamp(true, (size_t)156 * 1025, 1025, 0, 0));
    CHECK(!plan_layer_stamp(false, (size_t)156 * 1024, 1024, 0, 0));  // a shard does not stamp
    CHECK(!plan_layer_stamp(true, (size_t)156 * 1024, 1024, 0, IMGENV_FLAG_COMPOSE_DENSE));
    CHECK(plan_layer_stamp(true, (size_t)156 * 1025, 1025, 0, IMGENV_FLAG_COMPOSE_SPARSE));
    // "maps much larger than what the agents touch": more than 512 cells per agent
    CHECK(!plan_layer_stamp(true, (size_t)512 * 5000, 4000, 1000, 0));
    CHECK(plan_layer_stamp(true, (size_t)512 * 5000 + 1, 4000, 1000, 0));
    CHECK(!plan_layer_stamp(true, (size_t)1 << 40, STAMP_MAX_ROBOTS, 0, 0));  // the stamp's owner field
    const StepPlan sp = plan_step(h, c);
    CHECK(sp.fuse_move && !sp.sum_shard_now && !sp.early_step);
    c.moved = true;  // launch_views finds the move pending
    const RasterPlan r = plan_rasters(h, c);
    CHECK(r.move);  // k_move_raster
    CHECK_EQ(r.nw, 4);
    CHECK_EQ(r.move_peds, 0);
    CHECK_EQ(r.launch.grid, 1024);
    CHECK_EQ(r.launch.block, 256);
    CHECK_EQ(plan_views(h, c).nw, 8);
    CHECK_EQ(plan_views(h, c).view.block, 512);
    const SidePlan s = plan_side(h, c);  // no side launches
    CHECK(!s.overlap && !s.orca && !s.state && !s.remote_only);
    CHECK(plan_side(h, all_worlds(h, true)).state);
    // imgenv_step_begin / imgenv_step_end apart (the caller runs an exchange in between): the move keeps its own launch
    PlanChain apart = all_worlds(h, false);
    apart.in_step = false;
    CHECK(!plan_step(h, apart).fuse_move);
    apart.in_step = true; apart.comm = true;
    CHECK(!plan_step(h, apart).fuse_move);
}

static void cfg5() {  // 8192 robots + 1000 pedestrians, 96^2 / 720 beams
    PlanHandle h = handle(1, 8192, 1000, LAYER_SUM);
    h.lds_view = 15 * 1024;  // "crop + hit words + column table: 15 KB at 96 x 96 cells and 720 beams"
    const PlanChain c = all_worlds(h, false);
    const ViewPlan v = plan_views(h, c);
    CHECK(v.lds_bound);
    CHECK_EQ(v.nw, 4);
    CHECK_EQ(v.view.block, 256);
    CHECK_EQ(v.view.lds, 15 * 1024);
    CHECK_EQ(h.obs_E, 16);  // k_obs<16>
    CHECK_EQ(plan_side(h, c).slices, 4);  // "cfg-5's 1000 pedestrians in 16 slices only take issue slots": four at most
    CHECK(!plan_step(h, c).fuse_move);
    // a small launch of an LDS-bound handle: four wavefronts, not eight ("8 waves per view (4 when LDS-bound)")
    CHECK_EQ(plan_views(h, listed(h, 1)).nw, 4);
    // 16 or fewer one-wavefront workgroups per compute unit of 160 KiB, LDS granted in 1280-byte steps: 7 steps leave 18, 8 leave 16
    CHECK(!plan_lds_bound(7 * 1280));
    CHECK(plan_lds_bound(7 * 1280 + 1));
    CHECK(plan_lds_bound(8 * 1280));
    CHECK(!plan_lds_bound(5 * 1024));
}

static void worlds_300() {  // tests/test_gpu_large_launches.py: 300 worlds x (4 + 3), STAMP
    const PlanHandle h = handle(300, 4, 3, LAYER_STAMP);
    PlanChain c = all_worlds(h, false);
    c.stamp_seq = 1;
    RasterPlan r = plan_rasters(h, c);
    CHECK(!r.move);  // "k_raster<.., true, 1>, split"
    CHECK_EQ(r.nw, 1);
    CHECK_EQ(r.split, 1200);
    CHECK_EQ(r.launch.grid, 2100);
    CHECK(!r.sweep);
    CHECK_EQ(plan_views(h, c).nw, 2);  // "k_view<.., true, 2>"
    SidePlan s = plan_side(h, c);
    CHECK(s.one_side && s.overlap);
    CHECK(s.fold_side);  // several worlds with RVO crowds: no k_side_robots
    CHECK(s.orca && s.L.G == 4 && s.L.groups == 1 && s.L.fold_side == 1 && s.L.zero_vel == 0);
    CHECK_EQ(s.orca_blocks, 300);
    CHECK(!plan_step(h, c).fuse_move);  // 1200 robots with pedestrians
    CHECK_EQ(plan_step(h, c).nb_robot, 38);
    CHECK_EQ(plan_step(h, c).move.grid, 38 + 4);
    // "the resets of a few worlds in mid-flight the four-wavefront ones"
    PlanChain few = listed(h, 3);
    CHECK_EQ(plan_rasters(h, few).nw, 4);
    CHECK_EQ(plan_rasters(h, few).launch.grid, 12 + 9);
    CHECK_EQ(plan_views(h, few).nw, 8);
    CHECK_EQ(plan_side(h, few).L.zero_vel, 1);
    CHECK_EQ(plan_side(h, few).orca_blocks, 3);
    // "the reset of 250 worlds at once (1000 robots + ...) sits just below the threshold, the one of all 300 above it"
    PlanChain big = listed(h, 250);
    r = plan_rasters(h, big);
    CHECK_EQ(r.nw, 4);
    CHECK_EQ(r.split, 1000);
    CHECK_EQ(r.launch.grid, 1750);
    CHECK_EQ(r.launch.block, 256);
    CHECK_EQ(plan_views(h, big).nw, 8);
    CHECK_EQ(plan_views(h, big).view.grid, 1000);
    PlanChain every = listed(h, 300);
    CHECK_EQ(plan_rasters(h, every).nw, 1);
    CHECK_EQ(plan_views(h, every).nw, 2);
    // the sweep: every STAMP_TAGS steps, in a step only; 4 cells per thread over everything
    c.stamp_seq = 254; CHECK(!plan_rasters(h, c).sweep);
    c.stamp_seq = 255; CHECK(plan_rasters(h, c).sweep);
    c.stamp_seq = 256; CHECK(!plan_rasters(h, c).sweep);
    c.stamp_seq = 0; CHECK(plan_rasters(h, c).sweep);
    CHECK_EQ(plan_rasters(h, c).sweep_blocks, (120 * 120 * 300 / 4 + 255) / 256 + 1);
    big.stamp_seq = 255; CHECK(!plan_rasters(h, big).sweep);
    CHECK_EQ(plan_compose_blocks(h, big), ((120 * 120 / 4 + 255) / 256) * 250);  // a fixed number of blocks per listed world
    // chain tail: a step covers every local robot, a reset chain the robots of its worlds
    CHECK_EQ(plan_tail_rows(h, c), 1200);
    CHECK_EQ(plan_tail_rows(h, big), 1000);
    CHECK_EQ(plan_tail_rows(h, all_worlds(h, true)), 1200);
    CHECK_EQ(plan_tail_launch(h, big, 1, EP_BLOCK, EP_MAX_BLOCKS).grid, 4);
    CHECK_EQ(plan_tail_launch(h, c, 1, EP_BLOCK, EP_MAX_BLOCKS).grid, 5);
    CHECK_EQ(plan_tail_launch(h, c, 100, STACK_BLOCK, STACK_MAX_BLOCKS).grid, (1200 * 100 + 255) / 256);
    CHECK_EQ(plan_tail_launch(h, c, 100, STACK_BLOCK, STACK_MAX_BLOCKS).block, STACK_BLOCK);
    CHECK_EQ(plan_tail_launch(h, c, 10000, STACK_BLOCK, STACK_MAX_BLOCKS).grid, STACK_MAX_BLOCKS);
    CHECK_EQ(plan_tail(0, EP_BLOCK, EP_MAX_BLOCKS).grid, 1);
    CHECK_EQ(plan_tail((size_t)EP_BLOCK * EP_MAX_BLOCKS + 1, EP_BLOCK, EP_MAX_BLOCKS).grid, EP_MAX_BLOCKS);
    // the upload launch: segment copies | MAP_BLOCKS per world | 256 robots | 256 pedestrians per block
    const ResetPlan rp = plan_reset(h, big, 5, 100000, 500);
    CHECK_EQ(rp.per_seg, 16);
    CHECK_EQ(rp.apply.grid, 5 * 16 + 250 * 8 + 4 + 3);
    CHECK_EQ(rp.obstacles.grid, 500);
    CHECK_EQ(plan_reset(h, big, 5, 160, 500).per_seg, 2);
}

static void worlds_1400() {  // 1400 worlds x (4 + 3) = 5600 robots + 4200 pedestrians
    const PlanHandle h = handle(1400, 4, 3, LAYER_STAMP);
    PlanChain c = all_worlds(h, false);
    c.stamp_seq = 1;
    RasterPlan r = plan_rasters(h, c);
    CHECK_EQ(r.nw, 1);
    CHECK_EQ(r.split, 0);  // "beyond 8192 raster blocks a block draws a robot AND a pedestrian"
    CHECK_EQ(r.launch.grid, 5600);
    CHECK_EQ(plan_views(h, c).nw, 1);  // "beyond 4096 robots the views are the one-wavefront variant"
    CHECK(plan_side(h, c).overlap && !plan_side(h, c).one_side);  // two side streams
    // "the reset of 900 worlds at once (3600 robots) takes the two-wavefront views and the split rasters"
    const PlanChain big = listed(h, 900);
    r = plan_rasters(h, big);
    CHECK_EQ(r.nw, 1);
    CHECK_EQ(r.split, 3600);
    CHECK_EQ(r.launch.grid, 6300);
    CHECK_EQ(plan_views(h, big).nw, 2);
}

static void worlds_1100_without_pedestrians() {  // 1100 one-robot worlds
    const PlanHandle h = handle(1100, 1, 0, LAYER_STAMP);
    PlanChain c = all_worlds(h, false);
    c.stamp_seq = 1;
    CHECK(plan_step(h, c).fuse_move);
    c.moved = true;
    const RasterPlan r = plan_rasters(h, c);
    CHECK(r.move);  // "k_move_raster<.., true, 1>"
    CHECK_EQ(r.nw, 1);
    CHECK_EQ(r.launch.grid, 1100);
    CHECK_EQ(plan_views(h, c).nw, 2);  // "k_view<.., true, 2>"
    CHECK(!plan_side(h, c).state && !plan_side(h, c).orca && !plan_side(h, c).overlap);  // no side streams
    const SidePlan s = plan_side(h, listed(h, 3));  // "k_state after a reset"
    CHECK(s.state);
    CHECK_EQ(s.state_shape.grid, 1);
    CHECK_EQ(s.state_shape.block, 128);
    CHECK_EQ(plan_side(h, all_worlds(h, true)).state_shape.grid, 9);
}

static PlanHandle shipped(int E) {  // test.yaml: 1 robot + 4 leg pedestrians per env, 400 x 400-cell views shrunk to 48 x 48, 1000 beams
    PlanHandle h = handle(E, 1, 4, LAYER_STAMP);
    h.pow2 = false;
    h.big_view = true;
    h.B = 1000;
    h.lds_view = 16;
    h.big_max_crop = 2500;
    h.big_full_chunks = 157;
    h.big_tap_chunks_dyn = 6;
    h.lds_view_big = plan_lds_view_big(5000);
    h.crop_map = true;
    h.img_w = h.img_h = 48;
    h.resize = true;
    h.early = false;  // (views through view_big.h)
    return h;
}
static void shipped_geometry() {
    PlanHandle h = shipped(64);
    PlanChain c = all_worlds(h, false);
    ViewPlan v = plan_views(h, c);
    CHECK_EQ(v.tpw, 32);  // "k_crop_big with 32 tiles per wavefront (>= 48 robots)"
    CHECK_EQ(v.qpw, 1);
    CHECK_EQ(v.quarters, 4);
    CHECK_EQ(v.crop_chunks, (2500 + 127) / 128);
    CHECK_EQ(v.crop.grid, 64 * v.crop_chunks);
    CHECK_EQ(v.crop_sel, 2);
    CHECK_EQ(v.beams.grid, 64 * 4);
    CHECK_EQ(v.beams.lds, 4 * 5000 + 16);
    CHECK(v.taps && !v.full);  // a shrunk view is never materialised unless it is an output
    CHECK(v.listed);           // a step only runs the chunks of pixels a beam can reach
    CHECK_EQ(v.tap_wgs, 6);
    CHECK_EQ(v.taps_shape.grid, 64 * 6);
    CHECK_EQ(v.taps_shape.lds, 16 * 251 + 16 * 256 + 32 * 256 + 16);
    v = plan_views(h, listed(h, 3));  // "resets of 3 worlds (8 tiles per wavefront) and of 60 worlds (32)"
    CHECK_EQ(v.tpw, 8);
    CHECK_EQ(v.crop.grid, 8 * ((2500 + 31) / 32));  // (robots rounded up to 8)
    CHECK(!v.listed);
    CHECK_EQ(v.tap_wgs, 9);  // a reset writes every chunk of the 48 x 48 pixels
    CHECK_EQ(plan_views(h, listed(h, 60)).tpw, 32);
    CHECK_EQ(plan_views(h, listed(h, 47)).tpw, 8);
    CHECK_EQ(plan_views(h, listed(h, 48)).tpw, 32);
    h.keep_view_maps = true;
    v = plan_views(h, c);
    CHECK(v.full && v.taps);
    CHECK_EQ(v.fullview.grid, 64 * 157);
    CHECK_EQ(v.fullview.lds, 16 * 251);
    h = shipped(1024);  // "k_crop_big with 64 tiles per wavefront"; "end to end two win"
    c = all_worlds(h, false);
    v = plan_views(h, c);
    CHECK_EQ(v.tpw, 64);
    CHECK_EQ(v.qpw, 2);
    CHECK_EQ(v.beams.grid, 1024 * 2);
    CHECK_EQ(plan_views(h, listed(h, 1023)).tpw, 32);
    CHECK_EQ(plan_views(h, listed(h, 1023)).qpw, 1);
    CHECK_EQ(plan_views(h, listed(h, 1024)).tpw, 64);
    CHECK_EQ(plan_rasters(h, c).nw, 1);  // "k_raster<false, true, 1> (4096 leg pedestrians)"
    CHECK_EQ(plan_rasters(h, c).split, 1024);
    h.layer = LAYER_COMPOSED;
    CHECK_EQ(plan_views(h, c).crop_sel, 0);
    h.layer = LAYER_STAMP; h.crop_map = false;
    CHECK_EQ(plan_views(h, c).crop_sel, 1);
    h.B = 200;  // fewer than 256 beams: one block of them, one per workgroup
    CHECK_EQ(plan_views(h, c).quarters, 1);
    CHECK_EQ(plan_views(h, c).qpw, 1);
    // the crop bitmap next to the hit words up to 150 KiB
    CHECK(plan_big_bits_in_lds(150 * 1024 / 4));
    CHECK(!plan_big_bits_in_lds(150 * 1024 / 4 + 1));
    CHECK_EQ(plan_lds_view_big(150 * 1024 / 4 + 1), 16);
}

static void device_side_chain() {  // act_n_dev set: 1024 worlds x 4 robots, act_hint 64
    const PlanHandle h = handle(1024, 4, 3, LAYER_STAMP);
    PlanChain c = listed(h, 1024);  // "the launches behind: sized for every world, the list and its length read from device memory"
    c.n_dev = true;
    c.act_hint = 64;
    const RasterPlan r = plan_rasters(h, c);
    CHECK(r.small);  // by the hint
    CHECK_EQ(r.nw, 4);
    CHECK_EQ(r.launch.grid, 4096 + 3072);  // by every world
    CHECK_EQ(plan_views(h, c).nw, 8);
    CHECK_EQ(plan_views(h, c).view.grid, 4096);
    c.act_hint = 1025;
    CHECK_EQ(plan_rasters(h, c).nw, 1);
    CHECK_EQ(plan_views(h, c).nw, 2);
    c.act_hint = 1 << 20;  // a hint beyond the handle: the handle's own size counts
    CHECK_EQ(plan_views(h, c).nw, 2);
    c.act_hint = 64;
    CHECK_EQ(plan_tail_rows(h, c), 64);
    c.act_hint = 2;
    CHECK_EQ(plan_tail_rows(h, c), 4);  // at least one world
    c.act_hint = 1 << 20;
    CHECK_EQ(plan_tail_rows(h, c), 4096);
    // "grids for a guess of the finished worlds (four times the last count ...)"
    DevResetPlan d = plan_dev_reset(h, 0, 2);
    CHECK_EQ(d.guess, 16);
    CHECK_EQ(d.restore.grid, 16 * 4 * MAP_BLOCKS);
    CHECK_EQ(d.obstacles.grid, 16 * 2 * 4);
    CHECK_EQ(plan_dev_reset(h, 100, 2).guess, 400);
    CHECK_EQ(plan_dev_reset(h, 1000, 2).guess, 1024);
    CHECK_EQ(plan_dev_reset(h, -1, 2).guess, 16);
    // "twice the last count: with four times, 64 worlds of 4 pedestrians sat ON the 1024 threshold"
    CHECK_EQ(plan_act_hint(shipped(2048), 64), 512);
    CHECK_EQ(plan_act_hint(h, 0), 8 * 4);
}

static void robot_shard() {  // SUM layer, 1024 local robots of 8192, 200 pedestrians every rank keeps
    PlanHandle h = handle(1, 8192, 200, LAYER_SUM);
    h.RL = 1024;
    h.sharded = h.sum_shard = true;
    PlanChain c = all_worlds(h, false);
    c.act_nl = 1024;
    c.in_step = false;
    c.comm = true;
    StepPlan sp = plan_step(h, c);
    CHECK(sp.fuse_move && sp.sum_shard_now);  // "in k_move_raster with the move for <= 1024 robots"
    c.moved = c.local_only = true;
    RasterPlan r = plan_rasters(h, c);
    CHECK(r.move);
    CHECK_EQ(r.n_g, 1024);  // this rank's robots and the pedestrians
    CHECK_EQ(r.nw, 4);
    CHECK_EQ(r.launch.grid, 1024 + 200);
    CHECK_EQ(r.move_peds, 1);
    c.moved = c.local_only = false;
    SidePlan s = plan_side(h, c);
    CHECK(s.remote_only);  // in the step ...
    CHECK_EQ(s.remote.grid, (8192 - 1024) / 256);
    CHECK(s.side_reads_all);
    CHECK(s.overlap && !s.one_side);  // two side streams, any size
    CHECK_EQ(s.robots.grid, 128 * 4);  // every rank's robots are RVO agents
    PlanChain reset = all_worlds(h, true);
    reset.act_nl = 1024;
    CHECK(!plan_side(h, reset).remote_only);  // ... not in the reset
    CHECK_EQ(plan_views(h, c).nw, 8);  // "by the LOCAL robot count"
    CHECK_EQ(plan_reset(h, reset, 0, 0, 0).bbox.grid, 4);
    h.RL = 1025;
    c.act_nl = 1025;
    sp = plan_step(h, c);
    CHECK(!sp.fuse_move && !sp.sum_shard_now);
    CHECK_EQ(plan_views(h, c).nw, 2);
    // a COMPOSED shard: no fused move, no k_remote
    h.RL = 1024; h.sum_shard = false; h.layer = LAYER_COMPOSED;
    CHECK(!plan_step(h, c).fuse_move);
    CHECK(!plan_side(h, c).remote_only);
    h.relation = 0;  // a crowd that ignores the robots reads nothing of the other ranks
    CHECK(!plan_side(h, c).side_reads_all);
    CHECK_EQ(plan_side(h, c).rvo_agents, 0);
    CHECK_EQ(plan_side(h, c).slices, 1);
}

static void long_steps() {  // n_sub + 2 > INT_ITEMS
    PlanHandle h = handle(1, 1000, 100, LAYER_STAMP);
    h.n_sub = INT_ITEMS - 1;
    h.early = false;  // (imgenv_create: plan_integrate_fits)
    const PlanChain c = all_worlds(h, false);
    const StepPlan sp = plan_step(h, c);
    CHECK(sp.serial_move && !sp.fuse_move && !sp.early_step && !sp.fork_on_move);  // k_integrate_serial; no fuse, no early step
    CHECK_EQ(sp.nb_robot, 8);
    CHECK_EQ(sp.move.grid, 9);
    CHECK_EQ(sp.move.block, 128);
    CHECK(!plan_integrate_fits(INT_ITEMS - 1));
    CHECK(plan_integrate_fits(INT_ITEMS - 2));
    CHECK(plan_integrate_fits(1));
    CHECK(!plan_integrate_fits(0));
    h.n_sub = INT_ITEMS - 2;
    CHECK(plan_step(h, c).fuse_move);
}

static void thresholds() {
    // rasters: four wavefronts up to 1024 blocks, by the larger of robots and pedestrians
    for (int n : {1024, 1025}) {
        PlanHandle h = handle(1, n, 10, LAYER_SUM);
        CHECK_EQ(plan_rasters(h, all_worlds(h, false)).nw, n <= 1024 ? 4 : 1);
        CHECK_EQ(plan_rasters(h, all_worlds(h, false)).split, n);
        h = handle(1, 10, n, LAYER_SUM);
        CHECK_EQ(plan_rasters(h, all_worlds(h, false)).nw, n <= 1024 ? 4 : 1);
    }
    // ... blocks of their own up to 8192 of them
    for (int n : {8192, 8193}) {
        const PlanHandle h = handle(1, n - 100, 100, LAYER_SUM);
        const RasterPlan r = plan_rasters(h, all_worlds(h, false));
        CHECK_EQ(r.split, n <= 8192 ? n - 100 : 0);
        CHECK_EQ(r.launch.grid, n <= 8192 ? n : n - 100);
    }
    {   // no pedestrians (or no robots in the launch): nothing to split
        const PlanHandle h = handle(1, 2000, 0, LAYER_SUM);
        CHECK_EQ(plan_rasters(h, all_worlds(h, false)).split, 0);
        CHECK_EQ(plan_rasters(h, all_worlds(h, false)).launch.grid, 2000);
        CHECK_EQ(plan_rasters(h, all_worlds(h, false)).launch.lds, 4 * 81 + 16);
    }
    // views: 8 / 2 / 1 wavefronts up to 1024 / up to 4096 / more robots
    for (int n : {1024, 1025, 4096, 4097}) {
        const PlanHandle h = handle(1, n, 10, LAYER_SUM);
        CHECK_EQ(plan_views(h, all_worlds(h, false)).nw, n <= 1024 ? 8 : n <= 4096 ? 2 : 1);
        // one side stream up to 4096 robots
        CHECK_EQ(plan_side(h, all_worlds(h, false)).one_side, n <= 4096);
    }
    // the move inside the raster launch: up to 4096 robots without pedestrians, up to 1024 with
    for (int n : {4096, 4097}) {
        const PlanHandle h = handle(1, n, 0, LAYER_STAMP);
        CHECK_EQ(plan_step(h, all_worlds(h, false)).fuse_move, n <= 4096);
    }
    for (int n : {1024, 1025}) {
        const PlanHandle h = handle(1, n, 10, LAYER_STAMP);
        CHECK_EQ(plan_step(h, all_worlds(h, false)).fuse_move, n <= 1024);
    }
    // k_side_robots: "slices of >= 48 pedestrians, four at most"; one where the crowd is no RVO crowd or the worlds are several
    const int want[][2] = {{1, 1}, {48, 1}, {49, 2}, {96, 2}, {97, 3}, {145, 4}, {1000, 4}};
    for (const auto& w : want) {
        const PlanHandle h = handle(1, 5000, w[0], LAYER_SUM);
        CHECK_EQ(plan_side(h, all_worlds(h, false)).slices, w[1]);
    }
    {
        PlanHandle h = handle(1, 5000, 200, LAYER_SUM);
        h.NA = 0; h.scene = IMGENV_SCENE_PEDSIM;  // a social-force crowd: no solve, no RVO agents, and it has moved in k_sfm
        const SidePlan s = plan_side(h, all_worlds(h, false));
        CHECK(!s.orca && !s.fold_side);
        CHECK_EQ(s.slices, 1);
        CHECK_EQ(s.robots.grid, (5000 + 63) / 64);
        CHECK(!plan_peds_move(h));
        CHECK_EQ(plan_step(h, all_worlds(h, false)).move.grid, (5000 + 31) / 32);
        h.scene = IMGENV_SCENE_DATASET;  // a recorded crowd moves with the robots
        CHECK(plan_peds_move(h));
        // the early step of a social-force crowd needs the crowd a step ahead, not the solve
        h.scene = IMGENV_SCENE_PEDSIM;
        PlanChain c = all_worlds(h, false);
        c.orca_ran = false;
        CHECK(!plan_step(h, c).early_step);
        c.crowd_ahead = true;
        CHECK(plan_step(h, c).early_step);
    }
    // k_orca: a row of 16 lanes per agent, up to 4 agents per wavefront; scratch by the largest obstacle table
    {
        PlanHandle h = handle(10, 2, 1, LAYER_STAMP);
        PlanChain c = all_worlds(h, false);
        c.orca_cap = 0;
        SidePlan s = plan_side(h, c);
        CHECK(s.L.G == 1 && s.L.groups == 1 && s.orca_blocks == 10);
        CHECK_EQ(s.L.cap_on, ORCA_ROW - ORCA_MAX_AN);  // "a round's 16 candidate lines borrow the projection area"
        CHECK_EQ(s.L.cap_stack, 2);
        CHECK_EQ(s.L.stage_obst, 1);
        c.orca_cap = 1000;
        s = plan_side(h, c);
        CHECK_EQ(s.L.cap_on, ORCA_MAX_ON);
        CHECK_EQ(s.L.cap_stack, ORCA_STACK);
        CHECK_EQ(s.L.stage_obst, 256);  // "the table itself staged into LDS when it fits 256 segments"
        h = handle(10, 2, 2, LAYER_STAMP);
        CHECK_EQ(plan_side(h, all_worlds(h, false)).L.G, 2);
        h = handle(10, 2, 9, LAYER_STAMP);
        s = plan_side(h, all_worlds(h, false));
        CHECK(s.L.G == 4 && s.L.groups == 3 && s.orca_blocks == 30);
    }
    // k_obs: 64 * E sort slots in registers up to 1024 pedestrians, the LDS sort beyond
    const int slots[][3] = {{0, 64, 1}, {64, 64, 1}, {65, 128, 2}, {200, 256, 4}, {512, 512, 8}, {513, 1024, 16}, {1024, 1024, 16}, {1025, 2048, 0}};
    for (const auto& s : slots) {
        CHECK_EQ(plan_obs_slots(s[0]), s[1]);
        CHECK_EQ(plan_obs_E(s[1]), s[2]);
    }
    CHECK_EQ(plan_lds_obs(0, 2048, 1025), 2048 * 8 + 1025 * 8 + 2048 * 4 + 64 * 7 * 4 + 16);
    CHECK_EQ(plan_lds_obs(4, 256, 200), 200 * 8 + 256 * 4 + 64 * 7 * 4 + 16);
    CHECK_EQ(plan_lds_obs(1, 64, 0), 8 + 64 * 4 + 64 * 7 * 4 + 16);
    // k_view's LDS: src u8 (+ dummy cells, to 16 bytes) | hit u32 | column terms | cursors | three levels of largest hit steps
    CHECK_EQ(plan_lds_view(48 * 48, 364, 48), 2320 + 4 * 364 + 16 * 48 + 16 + 4 * (2 * 46 + 4));
    // the room of k_view's step (5): descriptors (8 bytes) in what the skip list (rounded to an even count) leaves of the crop's
    // 2320 bytes, slots (4 bytes) in the column table's 16 bytes per column; the tiny build's caps
    CHECK_EQ(plan_resolve_room(48 * 48, 48, 0).cap_d, 290);
    CHECK_EQ(plan_resolve_room(48 * 48, 48, 35).cap_d, (580 - 36) / 2);
    CHECK_EQ(plan_resolve_room(48 * 48, 48, 36).cap_d, (580 - 36) / 2);
    CHECK_EQ(plan_resolve_room(48 * 48, 48, 35).cap_r, 192);
    CHECK_EQ(plan_resolve_room(16 * 16, 16, 21).cap_d, 23);
    CHECK_EQ(plan_resolve_room(48 * 8, 8, 82).cap_d, 9);
    CHECK_EQ(plan_resolve_room(48 * 8, 8, 82).cap_r, 32);
    CHECK_EQ(plan_resolve_room(12, 4, 3).cap_d, 0);  // (never negative: a view of NC cells lists at most (NC + 3) / 4 entries)
    CHECK_EQ(plan_resolve_room(48 * 48, 48, 35, true).cap_d, 5);
    CHECK_EQ(plan_resolve_room(48 * 48, 48, 35, true).cap_r, 2);
    CHECK_EQ(LDS_DEFAULT_MAX, 64 * 1024);
    CHECK_EQ(LDS_MAX, 160 * 1024);
}

static void selectors() {  // pick: runtime selectors to compile-time constants, in argument order; an unknown value takes the list's last
    int got = -1;
    pick([&](auto A, auto B, auto N) { got = A() * 1000 + B() * 100 + N(); }, true, false, OneOf<1, 2, 4, 8>{4});
    CHECK_EQ(got, 1004);
    pick([&](auto N, auto A) { got = N() * 10 + A(); }, OneOf<1, 2, 4, 8>{8}, true);
    CHECK_EQ(got, 81);
    pick([&](auto N) { got = N(); }, OneOf<1, 2, 4, 8, 16, 0>{16});
    CHECK_EQ(got, 16);
    pick([&](auto N) { got = N(); }, OneOf<1, 2, 4, 8, 16, 0>{3});
    CHECK_EQ(got, 0);
    pick([&](auto L, auto N) { got = L() * 10 + N(); }, OneOf<0, 1, 2>{LAYER_SUM}, OneOf<1, 4>{1});
    CHECK_EQ(got, 21);
    int calls = 0;
    pick([&](auto A, auto B, auto C) { calls++; got = A() * 4 + B() * 2 + C(); }, false, true, true);
    CHECK(calls == 1 && got == 3);
}

int main() {
    headline();
    cfg2();
    cfg5();
    worlds_300();
    worlds_1400();
    worlds_1100_without_pedestrians();
    shipped_geometry();
    device_side_chain();
    robot_shard();
    long_steps();
    thresholds();
    selectors();
    if (g_fail) {
        printf("%d of %d checks failed\n", g_fail, g_checks);
        return 1;
    }
    printf("OK %d checks\n", g_checks);
    return 0;
}
