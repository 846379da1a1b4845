// What a host-side reset decides and computes without a device (csrc/reset_plan.h), on the CPU.  tests/test_reset_plan.py builds and
// runs this, once more under the sanitizers.
//
// Every literal below is DERIVED BY HAND (lattice bounds from the 0.01 m lattice, the 3-4-5 rotation of tests/test_oracle_tf.py,
// capacities from the growth rules, the refusals' texts copied from the FAIL lines they had in imgenv_hip.hip) -- none is printed
// from the code under test.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#define WAVE_SZ 64  // (host_tables.h: the .hip defines it in front of its includes)
#include "../../img_env_amd/csrc/reset_plan.h"

static int n_checks = 0, n_bad = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        n_checks++;                                                  \
        if (!(cond)) {                                               \
            n_bad++;                                                 \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                            \
    } while (0)
static bool near(double a, double b, double tol = 1e-12) { return fabs(a - b) <= tol; }

// a batch that owns its arrays: R robots, P pedestrians with trajectories of `cap` points (all of length `cap`), no obstacles
struct Batch {
    imgenv_reset_batch b;
    std::vector<double> robot_pose, robot_goal, ped_pose, ped_goal, ped_traj, ped_traj_v, obs_pose;
    std::vector<int32_t> ped_traj_len, obs_shape;
    std::vector<float> obs_size;
    Batch(int R, int P, int cap) {
        memset(&b, 0, sizeof(b));
        b.struct_size = (int32_t)sizeof(imgenv_reset_batch);
        robot_pose.assign(4 * (size_t)R, 0.0);
        for (int i = 0; i < R; i++) robot_pose[4 * i + 3] = 1.0;
        robot_goal.assign(2 * (size_t)R, 0.0);
        ped_pose.assign(4 * (size_t)P, 0.0);
        for (int j = 0; j < P; j++) ped_pose[4 * j + 3] = 1.0;
        ped_goal.assign(2 * (size_t)P, 0.0);
        ped_traj.assign(3 * (size_t)P * cap, 0.0);
        ped_traj_len.assign((size_t)P, cap);
        b.ped_traj_cap = cap;
        link();
    }
    void add_obstacle(int shape, float s0, float s1, float s2, float s3, double x, double y, double qz, double qw) {
        obs_shape.push_back(shape);
        for (float s : {s0, s1, s2, s3}) obs_size.push_back(s);
        for (double p : {x, y, qz, qw}) obs_pose.push_back(p);
        b.n_obstacles = (int32_t)obs_shape.size();
        link();
    }
    void link() {
        b.robot_pose = robot_pose.data(); b.robot_goal = robot_goal.data();
        b.ped_pose = ped_pose.data(); b.ped_goal = ped_goal.data(); b.ped_traj = ped_traj.data(); b.ped_traj_len = ped_traj_len.data();
        b.ped_traj_v = ped_traj_v.empty() ? nullptr : ped_traj_v.data();
        b.obs_shape = obs_shape.data(); b.obs_size = obs_size.data(); b.obs_pose = obs_pose.data();
    }
};

static ResetFacts facts(int W, int Rw, int Pw, int scene) {
    ResetFacts f;
    f.W = W; f.Rw = Rw; f.Pw = Pw; f.r0 = 0; f.RL = W * Rw; f.NA = Pw;
    f.scene = scene;
    return f;
}

// list position 1 of two batches is bad in one way: the code and the text
static void refusal(const ResetFacts& f, Batch& good, Batch& bad, int peds, int code, const char* text) {
    const imgenv_reset_batch two[2] = {good.b, bad.b};
    ResetMsg msg = "";
    CHECK(reset_check_batches(f, 2, two, peds, msg) == code);
    CHECK(std::string(msg) == text);
    if (std::string(msg) != text) printf("  got: %s\n", msg);
    msg[0] = 0;
    CHECK(reset_check_batches(f, 1, two, peds, msg) == IMGENV_OK && msg[0] == 0);  // (the good one alone passes)
}
static void check_refusals() {
    const ResetFacts rvo = facts(3, 2, 3, IMGENV_SCENE_RVO);
    Batch good(2, 3, 2);
    ResetMsg msg = "";
    CHECK(reset_check_batches(rvo, 1, nullptr, 3, msg) == IMGENV_EINVAL && std::string(msg) == "null argument");
    { Batch b(2, 3, 2); b.b.struct_size += 8; refusal(rvo, good, b, 3, IMGENV_EINVAL, "reset batch ABI mismatch"); }
    { Batch b(2, 3, 2); b.b.n_obstacles = -1; refusal(rvo, good, b, 3, IMGENV_EINVAL, "bad reset batch"); }
    { Batch b(2, 3, 2); b.b.ped_traj_cap = 0; refusal(rvo, good, b, 3, IMGENV_EINVAL, "bad reset batch"); }
    { Batch b(2, 3, 2); b.b.n_obstacles = 1; b.b.obs_size = nullptr; refusal(rvo, good, b, 3, IMGENV_EINVAL, "reset batch 1: null obstacle arrays"); }
    { Batch b(2, 3, 2); b.b.robot_goal = nullptr; refusal(rvo, good, b, 3, IMGENV_EINVAL, "reset batch 1: null robot arrays"); }
    {
        Batch b(2, 3, 2);
        b.add_obstacle(IMGENV_SHAPE_CIRCLE, 0, 0, 0.3f, 0, 1, 1, 0, 1);
        b.add_obstacle(IMGENV_SHAPE_LEG, 0, 0, 0.3f, 0, 1, 1, 0, 1);
        char want[128];
        snprintf(want, sizeof(want), "reset batch 1, obstacle 1: unsupported shape %d", IMGENV_SHAPE_LEG);
        refusal(rvo, good, b, 3, IMGENV_EINVAL, want);
    }
    { Batch b(2, 3, 2); b.b.ped_traj = nullptr; refusal(rvo, good, b, 3, IMGENV_EINVAL, "reset batch 1: null pedestrian arrays"); }
    {
        const ResetFacts ds = facts(3, 2, 3, IMGENV_SCENE_DATASET);
        Batch g2(2, 3, 2), b(2, 3, 2);
        g2.ped_traj_v.assign(2 * 3 * 2, 0.0);
        g2.link();
        refusal(ds, g2, b, 3, IMGENV_EINVAL, "dataset scene: ped_traj_v is missing from the reset batch");
        ResetFacts bank = ds;  // with a track bank the same batch is bank-fed: its pedestrian arrays are not even looked at
        bank.track_bank = true;
        b.b.ped_pose = nullptr;
        const imgenv_reset_batch two[2] = {g2.b, b.b};
        CHECK(reset_check_batches(bank, 2, two, 3, msg) == IMGENV_OK);
        CHECK(!reset_bank_fed(bank, g2.b) && reset_bank_fed(bank, b.b) && !reset_bank_fed(ds, b.b));
    }
    {
        const ResetFacts ps = facts(3, 2, 3, IMGENV_SCENE_PEDSIM);
        Batch b(2, 3, 2);
        b.b.ped_goal = nullptr;
        refusal(ps, good, b, 3, IMGENV_EINVAL, "pedscene: ped_goal is missing from the reset batch");
    }
    { Batch b(2, 3, 2); b.ped_traj_len[2] = 3; refusal(rvo, good, b, 3, IMGENV_EINVAL, "reset batch 1, ped 2: bad trajectory length 3"); }
    { Batch b(2, 3, 2); b.ped_traj_len[0] = 0; refusal(rvo, good, b, 3, IMGENV_EINVAL, "reset batch 1, ped 0: bad trajectory length 0"); }

    // the three that used to fire in the middle of staging: they read what prepare made of the batches
    {
        Batch a(2, 3, 2), b(2, 3, 2);
        a.add_obstacle(IMGENV_SHAPE_CIRCLE, 0, 0, 0.3f, 0, 1, 1, 0, 1);
        b.add_obstacle(IMGENV_SHAPE_CIRCLE, 0, 0, 0.3f, 0, 1, 1, 0, 1);
        b.add_obstacle(IMGENV_SHAPE_RECTANGLE, 0.5f, -0.5f, -0.1f, 0.1f, 1, 1, 0, 1);  // reversed x-extent
        std::vector<ResetWorld> w(2);
        reset_prepare_world(rvo, 0, a.b, w[0]);
        reset_prepare_world(rvo, 1, b.b, w[1]);
        CHECK(reset_check_worlds(rvo, w.data(), 1, msg) == IMGENV_OK);
        CHECK(reset_check_worlds(rvo, w.data(), 2, msg) == IMGENV_EINVAL && std::string(msg) == "obstacle 1: degenerate or oversized footprint");
    }
    {
        ResetFacts ps = facts(3, 2, 3, IMGENV_SCENE_PEDSIM);
        ps.sfm_cap_obs = 1;
        Batch a(2, 3, 2), b(2, 3, 2);
        a.add_obstacle(IMGENV_SHAPE_CIRCLE, 0, 0, 0.3f, 0, 1, 1, 0, 1);
        b.add_obstacle(IMGENV_SHAPE_CIRCLE, 0, 0, 0.3f, 0, 1, 1, 0, 1);
        b.add_obstacle(IMGENV_SHAPE_CIRCLE, 0, 0, 0.3f, 0, 4, 4, 0, 1);
        std::vector<ResetWorld> w(2);
        reset_prepare_world(ps, 0, a.b, w[0]);
        reset_prepare_world(ps, 2, b.b, w[1]);
        CHECK(w[0].sfm_obs.size() == 4 && w[1].sfm_obs.size() == 8);
        CHECK(reset_check_worlds(ps, w.data(), 2, msg) == IMGENV_EINVAL &&
              std::string(msg) == "world 2: more than 1 obstacles in a pedscene world of a multi-world handle");
        ps.W = 1;  // a single crowd grows instead (reset_growth)
        CHECK(reset_check_worlds(ps, w.data(), 2, msg) == IMGENV_OK);
        b.b.ignore_obstacle = 1;  // PedScene::addObs is not called
        reset_prepare_world(ps, 2, b.b, w[1]);
        CHECK(w[1].sfm_obs.empty() && w[1].rvo.ob.empty() && w[1].inst.size() == 2);
    }
}

static void check_obstacles() {
    const double pose[4] = {2.0, 3.0, 0.0, 1.0};
    {   // 0.30 / 0.01 rounds to 30 exactly in float64: bb = ceil(30) = 30
        const double s[4] = {0.05, -0.02, 0.30, 0};
        const ObstInst o = obstacle_instance(IMGENV_SHAPE_CIRCLE, s, pose, 7);
        CHECK(o.m0 == -30 && o.m1 == 30 && o.n0 == -30 && o.n1 == 30 && obstacle_footprint_ok(o));
        CHECK(o.x == 2.0 && o.y == 3.0 && o.sh == 0.0 && o.ch == 1.0 && o.cx == 0.05 && o.cy == -0.02 && o.r == 0.30 && o.world == 7 && o.shape == IMGENV_SHAPE_CIRCLE);
    }
    {   // a radius just above the lattice point: the batch carries float32, and float32(0.30) = 0.300000011920928955 > 0.30
        const double s[4] = {0, 0, (double)0.30f, 0};
        const ObstInst o = obstacle_instance(IMGENV_SHAPE_CIRCLE, s, pose, 0);
        CHECK(o.m0 == -31 && o.m1 == 31 && o.n0 == -31 && o.n1 == 31);
        const double s2[4] = {0, 0, 0.3000001, 0};
        CHECK(obstacle_instance(IMGENV_SHAPE_CIRCLE, s2, pose, 0).m1 == 31);
    }
    {   // floor(-0.2 / 0.01) = -20, ceil(0.3 / 0.01) = 30, floor(-0.1 / 0.01) = -10, ceil(0.1 / 0.01) = 10: each quotient rounds to the integer
        const double s[4] = {-0.2, 0.3, -0.1, 0.1};
        const ObstInst o = obstacle_instance(IMGENV_SHAPE_RECTANGLE, s, pose, 0);
        CHECK(o.m0 == -20 && o.m1 == 30 && o.n0 == -10 && o.n1 == 10 && obstacle_footprint_ok(o));
    }
    {   // reversed extent: m0 = 50 > m1 = -50
        const double s[4] = {0.5, -0.5, -0.1, 0.1};
        const ObstInst o = obstacle_instance(IMGENV_SHAPE_RECTANGLE, s, pose, 0);
        CHECK(o.m0 == 50 && o.m1 == -50 && !obstacle_footprint_ok(o));
    }
    {   // 10001 x 10001 = 100 020 001 lattice points > 2^26 = 67 108 864; 8192 x 8192 = 2^26 still passes
        const double s[4] = {0, 100, 0, 100};
        const ObstInst o = obstacle_instance(IMGENV_SHAPE_RECTANGLE, s, pose, 0);
        CHECK(o.m0 == 0 && o.m1 == 10000 && o.n0 == 0 && o.n1 == 10000 && !obstacle_footprint_ok(o));
        ObstInst e = o;
        e.m1 = e.n1 = 8191;
        CHECK(obstacle_footprint_ok(e));
        e.m1 = 8192;
        CHECK(!obstacle_footprint_ok(e));
    }
    {   // yaw/2 of the 3-4-5 rotation: sin = 0.6, cos = 0.8
        const double p[4] = {1, 2, 0.6, 0.8}, s[4] = {0, 0, 0.1, 0};
        const ObstInst o = obstacle_instance(IMGENV_SHAPE_CIRCLE, s, p, 0);
        CHECK(near(o.sh, 0.6) && near(o.ch, 0.8));
    }
    {   // the polygon: circle of r = 0.5 at (2, 3), yaw 0: pa = (1.5, 2.5), pb = (2.5, 3.5); pa.x pa.y, pa.x pb.y, pb.x pb.y, pb.x pa.y
        const double s[4] = {0, 0, 0.5, 0};
        double seg[4];
        float v[8];
        obstacle_polygon(IMGENV_SHAPE_CIRCLE, s, 2.0, 3.0, 0.0, 1.0, seg, v);
        const double want_seg[4] = {1.5, 2.5, 2.5, 3.5};
        const float want_v[8] = {1.5f, 2.5f, 1.5f, 3.5f, 2.5f, 3.5f, 2.5f, 2.5f};
        CHECK(memcmp(seg, want_seg, sizeof(seg)) == 0 && memcmp(v, want_v, sizeof(v)) == 0);
        // rectangle (-1, 2, -0.5, 0.25) at the origin: pa = (min x, min y), pb = (max x, max y)
        const double r[4] = {-1, 2, -0.5, 0.25};
        obstacle_polygon(IMGENV_SHAPE_RECTANGLE, r, 0.0, 0.0, 0.0, 1.0, seg, v);
        const float want_r[8] = {-1.f, -0.5f, -1.f, 0.25f, 2.f, 0.25f, 2.f, -0.5f};
        CHECK(memcmp(v, want_r, sizeof(v)) == 0);
    }
    {   // one world: its instances carry the world, RVO gets one quadrilateral (4 vertices, 4 BSP nodes), the crowd one segment
        ResetFacts f = facts(3, 2, 3, IMGENV_SCENE_PEDSIM);
        Batch b(2, 3, 2);
        b.add_obstacle(IMGENV_SHAPE_CIRCLE, 0, 0, 0.5f, 0, 2, 3, 0, 1);
        ResetWorld w;
        reset_prepare_world(f, 2, b.b, w);
        CHECK(w.world == 2 && w.inst.size() == 1 && w.inst[0].world == 2 && w.inst[0].m1 == 50);
        CHECK(w.rvo.ob.size() == 4 && w.rvo.nodes.size() == 4 && w.rvo.root == 0);
        CHECK(w.rvo.ob[0].px == 1.5f && w.rvo.ob[0].py == 2.5f && w.rvo.ob[1].px == 1.5f && w.rvo.ob[1].py == 3.5f);
        CHECK(w.sfm_obs.size() == 4 && w.sfm_obs[0] == 1.5 && w.sfm_obs[3] == 3.5);
        CHECK(!w.fed && w.traj_need == 2);
        f.NA = 0;  // no RVO agents: no polygons
        reset_prepare_world(f, 2, b.b, w);
        CHECK(w.rvo.ob.empty() && w.rvo.root == -1 && w.inst.size() == 1);
    }
}

static void check_robot_rows() {
    // pose (1, 2) with the 3-4-5 rotation q = (0, 0, 0.6, 0.8): cos = 0.28, sin = 0.96, yaw = 2 atan2(0.6, 0.8).  Goal (3, -1):
    // inverse(pose(goal, yaw)) has the transposed basis and origin R^T (-3, 1) = (-0.84 + 0.96, 2.88 + 0.28) = (0.12, 3.16).
    ResetFacts f = facts(1, 3, 0, IMGENV_SCENE_RVO);
    Batch b(3, 0, 1);
    for (int i = 0; i < 3; i++) {
        const double p[4] = {1.0 + i, 2, 0.6, 0.8};
        memcpy(&b.robot_pose[4 * i], p, sizeof(p));
        b.robot_goal[2 * i] = 3;
        b.robot_goal[2 * i + 1] = -1;
    }
    std::vector<double> rob3(15, -7.0);
    ResetRobot blank;
    memset(&blank, 0x5A, sizeof(blank));
    std::vector<ResetRobot> rr(3, blank);
    reset_robot_rows(f, 0, b.b, rob3.data(), rr.data());
    const double yaw = 2.0 * atan2(0.6, 0.8);
    for (int i = 0; i < 3; i++) {
        CHECK(rob3[5 * i] == 1.0 + i && rob3[5 * i + 1] == 2.0 && near(rob3[5 * i + 2], yaw) && near(rob3[5 * i + 3], 0.6) && near(rob3[5 * i + 4], 0.8));
        const Tf2& t = rr[i].world_target;
        CHECK(rr[i].gx == 3.0 && rr[i].gy == -1.0);
        CHECK(near(t.m00, 0.28) && near(t.m01, 0.96) && near(t.m10, -0.96) && near(t.m11, 0.28) && near(t.ox, 0.12) && near(t.oy, 3.16));
    }
    // a shard [1, 2) of the three: only robot 1 is local, its ResetRobot is entry 0; the others write none
    f.r0 = 1;
    f.RL = 1;
    std::vector<ResetRobot> one(1, blank);
    std::fill(rob3.begin(), rob3.end(), -7.0);
    reset_robot_rows(f, 0, b.b, rob3.data(), one.data());
    CHECK(one[0].gx == 3.0 && near(one[0].world_target.ox, 0.12));
    CHECK(rob3[0] == 1.0 && rob3[5] == 2.0 && rob3[10] == 3.0);  // (every robot's pose row is written: the rasters need them all)
    f.r0 = 3;  // a shard that holds none of them
    f.RL = 2;
    std::vector<ResetRobot> none(2, blank);
    reset_robot_rows(f, 0, b.b, rob3.data(), none.data());
    CHECK(memcmp(&none[0], &blank, sizeof(blank)) == 0 && memcmp(&none[1], &blank, sizeof(blank)) == 0);
    // several worlds: world 2 of a handle of 2-robot worlds writes entries 0 and 1 of ITS block
    ResetFacts m = facts(3, 2, 0, IMGENV_SCENE_RVO);
    std::vector<ResetRobot> two(2, blank);
    reset_robot_rows(m, 2, b.b, rob3.data(), two.data());
    CHECK(two[0].gx == 3.0 && two[1].gy == -1.0);
}

static void check_ped_rows() {
    Batch b(1, 2, 2);
    const double pp[8] = {1, 2, 0.6, 0.8, -3, 4, 0, 1};
    memcpy(b.ped_pose.data(), pp, sizeof(pp));
    for (int q = 0; q < 12; q++) b.ped_traj[q] = 10.0 + q;  // ped 0: (10 11 12) (13 14 15); ped 1: (16 17 18) (19 20 21)
    b.ped_traj_len[1] = 1;
    std::vector<double> ped3(6, -1.0), traj(2 * 5 * 3, -1.0);
    std::vector<int> tlen(2, -1);
    reset_ped_rows(2, b.b, false, 5, ped3.data(), tlen.data(), traj.data());
    CHECK(ped3[0] == 1 && ped3[1] == 2 && near(ped3[2], 2.0 * atan2(0.6, 0.8)) && ped3[3] == -3 && ped3[4] == 4 && ped3[5] == 0.0);
    CHECK(tlen[0] == 2 && tlen[1] == 1);
    double want[30] = {0};
    for (int q = 0; q < 6; q++) want[q] = 10.0 + q;   // ped 0, points 0 and 1; points 2..4 zero
    for (int q = 0; q < 3; q++) want[15 + q] = 16.0 + q;  // ped 1 at stride 5 * 3, point 0 only (length 1)
    CHECK(memcmp(traj.data(), want, sizeof(want)) == 0);
    // traj_v: (vx, vy) -> (vx, vy, atan2(vy, vx))
    b.ped_traj_v = {1, 1, -2, 0, 0, -3, 9, 9};
    b.link();
    std::vector<double> tv(30, -1.0);
    reset_traj_v_rows(2, b.b, 5, tv.data());
    double want_v[30] = {0};
    want_v[0] = 1; want_v[1] = 1; want_v[2] = atan2(1.0, 1.0);
    want_v[3] = -2; want_v[4] = 0; want_v[5] = atan2(0.0, -2.0);
    want_v[15] = 0; want_v[16] = -3; want_v[17] = atan2(-3.0, 0.0);
    CHECK(memcmp(tv.data(), want_v, sizeof(want_v)) == 0);
    CHECK(near(tv[2], M_PI / 4) && near(tv[5], M_PI) && near(tv[17], -M_PI / 2));
    // a bank-fed world: zeros for reset_ped, nothing else is touched (no trajectory segment: null pointers are not written)
    std::fill(ped3.begin(), ped3.end(), -1.0);
    reset_ped_rows(2, b.b, true, 5, ped3.data(), nullptr, nullptr);
    for (double v : ped3) CHECK(v == 0.0);
    ResetFacts ds = facts(2, 1, 2, IMGENV_SCENE_DATASET);
    ds.track_bank = true;
    ResetWorld w;
    b.ped_traj_v.clear();
    b.link();
    reset_prepare_world(ds, 1, b.b, w);
    CHECK(w.fed && w.traj_need == 0);
}

static void check_waypoints() {
    // ped 0: 9 trajectory points, cut at SFM_MAX_WP = 8 entries: the goal and the first 7 points; ped 1: 2 points of its 9
    static_assert(SFM_MAX_WP == 8, "the literals below");
    Batch b(1, 2, 9);
    b.ped_goal = {5, 6, -5, -6};
    b.link();
    for (int j = 0; j < 2; j++)
        for (int q = 0; q < 9; q++) {
            double* p = &b.ped_traj[((size_t)j * 9 + q) * 3];
            p[0] = 100 * j + q; p[1] = 100 * j + q + 0.5; p[2] = 0.25 * (q + 1);
        }
    b.ped_traj_len[1] = 2;
    std::vector<double> wx(16, -1), wy(16, -1), wr(16, -1);
    std::vector<int> dq(16, -1), dqn(2, -1), dest(2, -1), last(2, 5);
    reset_waypoint_rows(2, b.b, WaypointRows{wx.data(), wy.data(), wr.data(), dq.data(), dqn.data(), dest.data(), last.data()});
    CHECK(wx[0] == 5 && wy[0] == 6 && wr[0] == 1.0);
    for (int q = 0; q < 7; q++) CHECK(wx[1 + q] == q && wy[1 + q] == q + 0.5 && wr[1 + q] == 0.25 * (q + 1));
    for (int q = 0; q < 8; q++) CHECK(dq[q] == q);
    CHECK(dqn[0] == 8 && dest[0] == 0 && last[0] == -1);
    CHECK(wx[8] == -5 && wy[8] == -6 && wr[8] == 1.0 && wx[9] == 100 && wy[10] == 101.5 && wr[10] == 0.5);
    for (int q = 3; q < 8; q++) CHECK(wx[8 + q] == 0 && wy[8 + q] == 0 && wr[8 + q] == 0 && dq[8 + q] == 0);
    CHECK(dq[8] == 0 && dq[9] == 1 && dq[10] == 2 && dqn[1] == 3 && dest[1] == 0 && last[1] == -1);
}

static ResetWorld need(int world, size_t ob, size_t nodes, int traj, size_t segs) {
    ResetWorld w;
    w.world = world;
    w.rvo.ob.resize(ob);
    w.rvo.nodes.resize(nodes);
    w.traj_need = traj;
    w.sfm_obs.resize(4 * segs);
    return w;
}
static void check_growth() {
    // capacities 8 vertices / 8 nodes / 2 points; worlds 0 and 2 of three bring (10, 10, 7) and (15, 7, 4):
    // vertices 15 > 8 -> 30, nodes 10 > 8 -> 20, trajectories exactly 7
    ResetFacts f = facts(3, 2, 3, IMGENV_SCENE_RVO);
    f.cap_obst = 8; f.cap_nodes = 8; f.traj_cap = 2;
    std::vector<ResetWorld> w = {need(0, 10, 10, 7, 0), need(2, 15, 7, 4, 0)};
    ResetGrowth g = reset_growth(f, w.data(), 2);
    CHECK(g.cap_obst == 30 && g.cap_nodes == 20 && g.traj_cap == 7 && g.rvo_moved && g.traj_moved && !g.sfm_moved && g.sfm_cap_obs == 0);
    // the same whatever the order of the list (the growth is decided once, not world by world)
    std::swap(w[0], w[1]);
    const ResetGrowth g2 = reset_growth(f, w.data(), 2);
    CHECK(g2.cap_obst == 30 && g2.cap_nodes == 20 && g2.traj_cap == 7);
    std::swap(w[0], w[1]);
    // every slice goes up exactly once where they moved: worlds 0, 1, 2 at k * cap, each within its stride, so no two overlap
    const int list[2] = {0, 2};
    const std::vector<int> all = reset_rvo_worlds(3, g, list, 2);
    CHECK(all == std::vector<int>({0, 1, 2}));
    const size_t size_ob[3] = {10, 6, 15};  // (world 1 keeps the 6 vertices it had)
    for (size_t a = 0; a < all.size(); a++)
        for (size_t c = a + 1; c < all.size(); c++) {
            const size_t a0 = (size_t)all[a] * g.cap_obst, a1 = a0 + size_ob[all[a]], c0 = (size_t)all[c] * g.cap_obst, c1 = c0 + size_ob[all[c]];
            CHECK(all[a] != all[c] && (a1 <= c0 || c1 <= a0));
        }
    // nothing outgrown: nothing moves, only the listed worlds' slices go up
    f.cap_obst = 16; f.cap_nodes = 16; f.traj_cap = 7;
    g = reset_growth(f, w.data(), 2);
    CHECK(g.cap_obst == 16 && g.cap_nodes == 16 && g.traj_cap == 7 && !g.rvo_moved && !g.traj_moved);
    CHECK(reset_rvo_worlds(3, g, list, 2) == std::vector<int>({0, 2}));
    CHECK(reset_rvo_worlds(3, g, nullptr, 3) == std::vector<int>({0, 1, 2}));  // a whole-handle reset: every world
    // shorter trajectories than the table's: it stays
    f.traj_cap = 9;
    CHECK(reset_growth(f, w.data(), 2).traj_cap == 9 && !reset_growth(f, w.data(), 2).traj_moved);
    // a single pedscene crowd: 5 segments > 3 -> 10; several worlds: fixed slices
    ResetFacts ps = facts(1, 2, 3, IMGENV_SCENE_PEDSIM);
    ps.sfm_cap_obs = 3;
    std::vector<ResetWorld> one = {need(0, 0, 0, 2, 5)};
    CHECK(reset_growth(ps, one.data(), 1).sfm_cap_obs == 10 && reset_growth(ps, one.data(), 1).sfm_moved);
    ps.W = 2;
    CHECK(reset_growth(ps, one.data(), 1).sfm_cap_obs == 3 && !reset_growth(ps, one.data(), 1).sfm_moved);
    // after the device-side reset has taken the tables over they cannot grow: IMGENV_ESTATE, naming the world
    f.cap_obst = 8; f.cap_nodes = 8;
    f.dev_reset_used = true;
    ResetMsg msg = "";
    CHECK(reset_check_worlds(f, w.data(), 2, msg) == IMGENV_ESTATE);
    CHECK(std::string(msg) == "world 0: more RVO obstacle vertices than the handle has room for, after imgenv_step_autoreset_device has taken over "
                              "the per-world obstacle tables (reset every world with imgenv_reset first)");
    f.cap_obst = 16; f.cap_nodes = 16;
    CHECK(reset_check_worlds(f, w.data(), 2, msg) == IMGENV_OK);
    // the table's column of a world: bases at k * cap, count, root
    std::vector<int> wobst(12, -9);
    RvoObstacles r;
    r.ob.resize(6);
    r.root = 4;
    rvo_table_put(wobst, 3, 1, 30, 20, r);
    CHECK(wobst == std::vector<int>({-9, 30, -9, -9, 20, -9, -9, 6, -9, -9, 4, -9}));
}

static void check_pool() {
    // S = (SPAWN_FILL_PERIOD + 2) max(64, W) with SPAWN_FILL_PERIOD = 2
    static_assert(SPAWN_FILL_PERIOD == 2 && SPAWN_BSP_CAP == 256, "the literals below");
    CHECK(spawn_pool_slots(1) == 256 && spawn_pool_slots(64) == 256 && spawn_pool_slots(65) == 260);
    // 16 vertices per obstacle, at least 16, at most SPAWN_BSP_CAP (reached at 16 obstacles)
    CHECK(spawn_slot_cap(0) == 16 && spawn_slot_cap(1) == 16 && spawn_slot_cap(8) == 128 && spawn_slot_cap(15) == 240 && spawn_slot_cap(16) == 256 &&
          spawn_slot_cap(24) == 256);
    ResetFacts f = facts(4, 2, 3, IMGENV_SCENE_RVO);
    f.traj_cap = 2;
    f.has_traj = true;
    imgenv_spawn_cfg cfg;
    memset(&cfg, 0, sizeof(cfg));
    std::vector<imgenv_spawn_agent> agents(5);
    memset(agents.data(), 0, sizeof(imgenv_spawn_agent) * agents.size());
    cfg.n_robots = 2; cfg.n_peds = 3; cfg.agents = agents.data();
    ResetMsg msg = "";
    CHECK(spawn_pool_check(f, cfg, msg) == IMGENV_OK);
    cfg.n_obstacles = SPAWN_MAX_OBST + 1;
    CHECK(spawn_pool_check(f, cfg, msg) == IMGENV_EINVAL && std::string(msg) == "device-side auto-reset places at most 256 agents and 24 obstacles per world");
    cfg.n_obstacles = 0;
    f.traj_cap = 1;
    CHECK(spawn_pool_check(f, cfg, msg) == IMGENV_ESTATE && std::string(msg) == "device-side auto-reset: reset every world once first (trajectories of two points)");
    f.traj_cap = 2;
    f.scene = IMGENV_SCENE_DATASET;
    CHECK(spawn_pool_check(f, cfg, msg) == IMGENV_EINVAL &&
          std::string(msg) == "device-side auto-reset: dataset scenes (recorded crowds come with the reset call) are reset by the host (imgenv_step_autoreset)");
    f.track_bank = true;
    CHECK(spawn_pool_check(f, cfg, msg) == IMGENV_OK);
    f.scene = IMGENV_SCENE_PEDSIM;
    f.sfm_n = 3; f.sfm_per_world = true; f.sfm_cap_obs = 2;
    cfg.n_obstacles = 3;
    CHECK(spawn_pool_check(f, cfg, msg) == IMGENV_EINVAL && std::string(msg) == "device-side auto-reset: 3 obstacles, a pedscene world of this handle has room for 2");
    cfg.ignore_obstacle = 1;
    CHECK(spawn_pool_check(f, cfg, msg) == IMGENV_OK);
    f.W = 1;
    CHECK(spawn_pool_check(f, cfg, msg) == IMGENV_EINVAL &&
          std::string(msg) == "device-side auto-reset of a pedscene world needs a handle of several worlds (n_worlds > 1: the per-world crowd tables)");
    f = facts(4, 2, 3, IMGENV_SCENE_RVO);
    f.traj_cap = 2; f.has_traj = true;
    cfg.n_obstacles = 0;
    agents[4].target_type = IMGENV_POSE_RANGE_MULTI;
    CHECK(spawn_pool_check(f, cfg, msg) == IMGENV_EINVAL && std::string(msg) == "range_multi target without ranges");
    agents[1].begin_type = IMGENV_POSE_RANGE_MULTI;
    CHECK(spawn_pool_check(f, cfg, msg) == IMGENV_EINVAL && std::string(msg) == "range_multi start without ranges");
}

int main() {
    check_refusals();
    check_obstacles();
    check_robot_rows();
    check_ped_rows();
    check_waypoints();
    check_growth();
    check_pool();
    if (n_bad) return printf("%d of %d checks failed\n", n_bad, n_checks), 1;
    printf("OK %d checks\n", n_checks);
    return 0;
}
