// scenario_bank_check.cpp -- the host half of imgenv_scenarios_add (img_env_amd/csrc/scenario_bank.h: scenarios_convert,
// scenario_to_arrays, scenario_for_placement) without a device: recorded episodes become the slot records the device-side reset
// copies, and come back as the arrays a host reset takes.  Built with -fsanitize=address,undefined by tests/test_scenarios_abi.py:
// the arrays are exactly as large as the prototype says, so a read past a short input or a write past the bank fails it.
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -I include tests/host/scenario_bank_check.cpp -o check && ./check
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "../../img_env_amd/csrc/scenario_bank.h"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        g_checks++;                                                  \
        if (!(cond)) {                                               \
            g_fail++;                                                \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
        }                                                            \
    } while (0)

struct Bank {
    int n, Rw, Pw, O;
    std::vector<double> robot_pose, robot_goal, ped_pose, ped_goal, ped_traj, obs_pose;
    std::vector<int32_t> ped_traj_len, obs_shape;
    std::vector<float> obs_size;
};
static Bank make_bank(int n, int Rw, int Pw, int O) {
    Bank b{n, Rw, Pw, O};
    b.robot_pose.resize((size_t)n * Rw * 4); b.robot_goal.resize((size_t)n * Rw * 2);
    b.ped_pose.resize((size_t)n * Pw * 4); b.ped_goal.resize((size_t)n * Pw * 2); b.ped_traj.resize((size_t)n * Pw * 6);
    b.ped_traj_len.resize((size_t)n * Pw);
    b.obs_shape.resize((size_t)n * O); b.obs_size.resize((size_t)n * O * 4); b.obs_pose.resize((size_t)n * O * 4);
    for (int s = 0; s < n; s++) {
        for (int i = 0; i < Rw; i++) {
            double* p = &b.robot_pose[((size_t)s * Rw + i) * 4];
            const double yaw = 0.4 * i - 0.1 * s;
            p[0] = 1.0 + s + 0.5 * i; p[1] = 2.0 - i; p[2] = sin(yaw / 2); p[3] = cos(yaw / 2);
            b.robot_goal[((size_t)s * Rw + i) * 2] = 9.0 - s; b.robot_goal[((size_t)s * Rw + i) * 2 + 1] = 3.5 + i;
        }
        for (int j = 0; j < Pw; j++) {
            const size_t at = (size_t)s * Pw + j;
            double* p = &b.ped_pose[at * 4];
            p[0] = 4.0 + j; p[1] = 5.0 + s; p[2] = sin(0.3 * j); p[3] = cos(0.3 * j);
            b.ped_goal[at * 2] = 7.0 + j; b.ped_goal[at * 2 + 1] = 8.0 - s;
            const int len = (s + j) % 3;  // 0, 1 and 2 all occur
            b.ped_traj_len[at] = len;
            for (int e = 0; e < 6; e++) b.ped_traj[at * 6 + e] = e < 3 * len ? 0.25 * e + j : 1e9;  // junk behind the length must not come through
        }
        for (int q = 0; q < O; q++) {
            const size_t at = (size_t)s * O + q;
            b.obs_shape[at] = q % 2 ? IMGENV_SHAPE_RECTANGLE : IMGENV_SHAPE_CIRCLE;
            float* z = &b.obs_size[at * 4];
            if (q % 2) { z[0] = -0.15f; z[1] = 0.15f; z[2] = -0.2f; z[3] = 0.2f; } else { z[0] = z[1] = z[3] = 0.0f; z[2] = 0.3f; }
            double* p = &b.obs_pose[at * 4];
            p[0] = 10.0 + q; p[1] = 11.0 + s; p[2] = sin(0.2 * q); p[3] = cos(0.2 * q);
        }
    }
    return b;
}
struct Slots {
    std::vector<SlotAgent> agents;
    std::vector<SlotObstacle> obst;
    int where = -7, which = -7;
};
static int convert(const Bank& b, Slots& o) {
    o.agents.assign((size_t)b.n * (b.Rw + b.Pw), SlotAgent());  // (exactly the size the library allocates)
    o.obst.assign((size_t)b.n * b.O, SlotObstacle());
    memset(o.agents.data(), 0x5A, o.agents.size() * sizeof(SlotAgent));
    memset(o.obst.data(), 0x5A, o.obst.size() * sizeof(SlotObstacle));
    return scenarios_convert(b.n, b.Rw, b.Pw, b.O, b.robot_pose.data(), b.robot_goal.data(), b.Pw ? b.ped_pose.data() : nullptr,
                             b.Pw ? b.ped_goal.data() : nullptr, b.Pw ? b.ped_traj.data() : nullptr, b.Pw ? b.ped_traj_len.data() : nullptr,
                             b.O ? b.obs_shape.data() : nullptr, b.O ? b.obs_size.data() : nullptr, b.O ? b.obs_pose.data() : nullptr, o.agents.data(),
                             o.obst.data(), &o.where, &o.which);
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    Slots o;
    {   // 7 episodes of 2 robots, 3 pedestrians, 2 obstacles: the records, and the way back
        const Bank b = make_bank(7, 2, 3, 2);
        CHECK(convert(b, o) == 0);
        for (int s = 0; s < 7; s++) {
            for (int a = 0; a < 5; a++) {
                const SlotAgent& g = o.agents[(size_t)s * 5 + a];
                const bool robot = a < 2;
                const size_t at = robot ? (size_t)s * 2 + a : (size_t)s * 3 + (a - 2);
                const double* p = (robot ? b.robot_pose.data() : b.ped_pose.data()) + 4 * at;
                const double* gl = (robot ? b.robot_goal.data() : b.ped_goal.data()) + 2 * at;
                CHECK(memcmp(&g.x, p, 32) == 0 && memcmp(&g.gx, gl, 16) == 0 && g.pad == 0);
                if (robot) {
                    CHECK(g.traj_len == 1 && g.traj[0][0] == gl[0] && g.traj[0][1] == gl[1] && g.traj[0][2] == 0.0 && g.traj[1][0] == 0.0);
                } else {
                    const int len = b.ped_traj_len[at];
                    CHECK(g.traj_len == len);
                    for (int e = 0; e < 6; e++) CHECK((&g.traj[0][0])[e] == (e < 3 * len ? b.ped_traj[at * 6 + e] : 0.0));
                }
            }
            for (int q = 0; q < 2; q++) {
                const SlotObstacle& g = o.obst[(size_t)s * 2 + q];
                const size_t at = (size_t)s * 2 + q;
                CHECK(memcmp(&g.x, &b.obs_pose[at * 4], 32) == 0 && memcmp(g.size, &b.obs_size[at * 4], 16) == 0 && g.shape == b.obs_shape[at] && g.pad == 0);
            }
            // back into the arrays of a reset batch: what went in, with zeros behind the lengths
            std::vector<double> rp(8), rg(4), pp(12), pg(6), pt(18), op(8);
            std::vector<int32_t> pl(3), os(2);
            std::vector<float> oz(8);
            scenario_to_arrays(2, 3, 2, &o.agents[(size_t)s * 5], &o.obst[(size_t)s * 2], rp.data(), rg.data(), pp.data(), pg.data(), pt.data(), pl.data(),
                               os.data(), oz.data(), op.data());
            CHECK(memcmp(rp.data(), &b.robot_pose[(size_t)s * 8], 64) == 0 && memcmp(rg.data(), &b.robot_goal[(size_t)s * 4], 32) == 0);
            CHECK(memcmp(pp.data(), &b.ped_pose[(size_t)s * 12], 96) == 0 && memcmp(pg.data(), &b.ped_goal[(size_t)s * 6], 48) == 0);
            CHECK(memcmp(pl.data(), &b.ped_traj_len[(size_t)s * 3], 12) == 0 && memcmp(os.data(), &b.obs_shape[(size_t)s * 2], 8) == 0);
            CHECK(memcmp(oz.data(), &b.obs_size[(size_t)s * 8], 32) == 0 && memcmp(op.data(), &b.obs_pose[(size_t)s * 8], 64) == 0);
            for (int j = 0; j < 3; j++)
                for (int e = 0; e < 6; e++) CHECK(pt[6 * j + e] == (e < 3 * pl[j] ? b.ped_traj[((size_t)s * 3 + j) * 6 + e] : 0.0));
        }
    }
    {   // a one-entry bank without pedestrians and obstacles: null arrays are not touched
        const Bank b = make_bank(1, 1, 0, 0);
        CHECK(convert(b, o) == 0 && o.agents.size() == 1 && o.agents[0].traj_len == 1);
    }
    {   // every kind of bad bank, and where it is reported
        Bank b = make_bank(3, 2, 3, 2);
        b.robot_pose[(1 * 2 + 1) * 4 + 1] = nan;
        CHECK(convert(b, o) == SCENARIO_BAD_FINITE && o.where == 1 && o.which == 1);
        b = make_bank(3, 2, 3, 2);
        b.ped_goal[(2 * 3 + 2) * 2] = inf;
        CHECK(convert(b, o) == SCENARIO_BAD_FINITE && o.where == 2 && o.which == 4);
        b = make_bank(3, 2, 3, 2);
        b.ped_pose[(0 * 3 + 1) * 4 + 2] = b.ped_pose[(0 * 3 + 1) * 4 + 3] = 0.0;
        CHECK(convert(b, o) == SCENARIO_BAD_QUATERNION && o.where == 0 && o.which == 3);
        b = make_bank(3, 2, 3, 2);
        b.robot_pose[2] = b.robot_pose[3] = 0.0;
        CHECK(convert(b, o) == SCENARIO_BAD_QUATERNION && o.where == 0 && o.which == 0);
        b = make_bank(3, 2, 3, 2);
        b.ped_traj_len[1 * 3 + 0] = 3;
        CHECK(convert(b, o) == SCENARIO_BAD_TRAJ_LEN && o.where == 1 && o.which == 2);
        b.ped_traj_len[1 * 3 + 0] = -1;
        CHECK(convert(b, o) == SCENARIO_BAD_TRAJ_LEN);
        b = make_bank(3, 2, 3, 2);
        b.ped_traj[((size_t)0 * 3 + 2) * 6 + 4] = nan;  // inside pedestrian 2's length (2) of scenario 0 ...
        CHECK(convert(b, o) == SCENARIO_BAD_FINITE && o.where == 0 && o.which == 4);
        b = make_bank(3, 2, 3, 2);
        b.ped_traj[((size_t)0 * 3 + 1) * 6 + 4] = nan;  // ... behind pedestrian 1's length (1): not read
        CHECK(convert(b, o) == 0);
        b = make_bank(3, 2, 3, 2);
        b.obs_shape[2 * 2 + 1] = 9;
        CHECK(convert(b, o) == SCENARIO_BAD_SHAPE && o.where == 2 && o.which == 1);
        b.obs_shape[2 * 2 + 1] = IMGENV_SHAPE_LEG;
        CHECK(convert(b, o) == SCENARIO_BAD_SHAPE);
        b = make_bank(3, 2, 3, 2);
        b.obs_size[(1 * 2 + 0) * 4 + 2] = std::numeric_limits<float>::quiet_NaN();
        CHECK(convert(b, o) == SCENARIO_BAD_FINITE && o.where == 1 && o.which == 0);
        b = make_bank(3, 2, 3, 2);
        b.obs_pose[(1 * 2 + 1) * 4 + 2] = b.obs_pose[(1 * 2 + 1) * 4 + 3] = 0.0;
        CHECK(convert(b, o) == SCENARIO_BAD_QUATERNION && o.where == 1 && o.which == 1);
        b = make_bank(3, 2, 3, 2);
        b.obs_size[(0 * 2 + 0) * 4 + 2] = 1e6f;  // a circle of 10^8 x 10^8 footprint samples
        CHECK(convert(b, o) == SCENARIO_BAD_FOOTPRINT && o.where == 0 && o.which == 0);
        b.obs_size[(0 * 2 + 0) * 4 + 2] = -0.3f;
        CHECK(convert(b, o) == SCENARIO_BAD_FOOTPRINT);
        for (int c = 1; c <= 5; c++) CHECK(strlen(scenario_error_text(c)) > 3);
    }
    {   // which scenario a placement takes
        for (int n : {1, 7, 256, 300}) {
            for (uint64_t k = 0; k < 2000; k++) {
                CHECK(scenario_for_placement(IMGENV_SCENARIOS_QUEUE, 99, 5, k, n) == (int32_t)((5 + k) % (uint64_t)n));
                const int32_t d = scenario_for_placement(IMGENV_SCENARIOS_BY_PLACEMENT, 99, 5, k, n);
                CHECK(d >= 0 && d < n && d == map_for_placement(99 + k + SCENARIO_PLACEMENT_SALT, n));
                CHECK(scenario_for_placement(IMGENV_SCENARIOS_OFF, 99, 5, k, n) == -1);
            }
        }
        CHECK(scenario_for_placement(IMGENV_SCENARIOS_QUEUE, 0, ~0ull, 3, 7) == 2);  // first + n wraps modulo 2^64: (2^64 - 1 + 3) mod 2^64 = 2
        CHECK(scenario_for_placement(IMGENV_SCENARIOS_QUEUE, 0, ~0ull, 0, 7) == (int32_t)(~0ull % 7));
        CHECK(scenario_for_placement(IMGENV_SCENARIOS_QUEUE, 0, 0, 0, 0) == -1);
        CHECK(SCENARIO_PLACEMENT_SALT != 0xBB67AE8584CAA73Bull);
    }
    if (g_fail) {
        printf("%d of %d checks FAILED\n", g_fail, g_checks);
        return 1;
    }
    printf("OK %d checks\n", g_checks);
    return 0;
}
