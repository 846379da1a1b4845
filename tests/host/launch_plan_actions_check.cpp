// launch_plan_actions_check.cpp -- the shapes of the two launches around a chain (img_env_amd/csrc/launch_plan.h):
// k_actions in front of it (plan_actions_launch: one lane per local robot, whole wavefronts, no stride) and k_obs_post at its end
// (plan_tail_launch with OBS_POST_BLOCK / OBS_POST_MAX_BLOCKS: one lane per element of the rows the chain covers, capped and strided like k_stack).
// The expected values are written down from include/imgenv.h and the headers of csrc/actions.h / csrc/obs_post.h.
//   g++ -std=c++17 -I include tests/host/launch_plan_actions_check.cpp -o check && ./check
#include <stdio.h>

#include "../../img_env_amd/csrc/launch_plan.h"

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

static PlanHandle handle(int W, int Rw) {
    PlanHandle h;
    h.W = W; h.Rw = Rw; h.R = h.RL = W * Rw;
    return h;
}
static PlanChain step_chain(const PlanHandle& h) {
    PlanChain c;
    c.act_nw = h.W; c.act_ng = c.act_nl = h.RL;
    return c;
}

int main() {
    const int PV = 1 + 7 * 10;  // max_ped 10: 71 floats per row
    for (int R : {1, 256, 257}) {
        const PlanHandle h = handle(1, R);
        const unsigned blocks = R <= 256 ? 1 : 2;
        CHECK_EQ(plan_actions_launch(h).grid, blocks);
        CHECK_EQ(plan_actions_launch(h).block, 256);
        CHECK_EQ(plan_actions_launch(h).lds, 0);
        CHECK_EQ(plan_actions_launch(h).block % WAVE, 0);  // the ballot runs on whole wavefronts
        // a step and imgenv_reset cover every local robot; close_to_human alone is one lane per robot
        PlanChain c = step_chain(h);
        CHECK_EQ(plan_tail_launch(h, c, 1, OBS_POST_BLOCK, OBS_POST_MAX_BLOCKS).grid, blocks);
        CHECK_EQ(plan_tail_launch(h, c, 1, OBS_POST_BLOCK, OBS_POST_MAX_BLOCKS).block, 256);
        CHECK_EQ(plan_tail_launch(h, c, PV, OBS_POST_BLOCK, OBS_POST_MAX_BLOCKS).grid, (R * PV + 255) / 256);
        c.is_reset = true;
        CHECK_EQ(plan_tail_launch(h, c, PV, OBS_POST_BLOCK, OBS_POST_MAX_BLOCKS).grid, (R * PV + 255) / 256);
    }
    CHECK_EQ(plan_tail_launch(handle(1, 1), step_chain(handle(1, 1)), PV, OBS_POST_BLOCK, OBS_POST_MAX_BLOCKS).grid, 1);
    CHECK_EQ(plan_tail_launch(handle(1, 257), step_chain(handle(1, 257)), PV, OBS_POST_BLOCK, OBS_POST_MAX_BLOCKS).grid, 72);  // 18247 lanes
    {   // a sharded handle decodes its local rows
        PlanHandle h = handle(1, 1024);
        h.RL = 257; h.sharded = true;
        CHECK_EQ(plan_actions_launch(h).grid, 2);
    }
    {   // a listed reset chain of 2 worlds x 3 robots on a handle of 16 x 3
        const PlanHandle h = handle(16, 3);
        PlanChain c = step_chain(h);
        c.is_reset = true; c.listed = true; c.act_nw = 2; c.act_ng = c.act_nl = 6;
        CHECK_EQ(plan_tail_rows(h, c), 6);
        CHECK_EQ(plan_tail_launch(h, c, PV, OBS_POST_BLOCK, OBS_POST_MAX_BLOCKS).grid, 2);  // 6 x 71 = 426 lanes
        CHECK_EQ(plan_tail_launch(h, c, 1, OBS_POST_BLOCK, OBS_POST_MAX_BLOCKS).grid, 1);
        CHECK_EQ(plan_tail_launch(h, c, 15, OBS_POST_BLOCK, OBS_POST_MAX_BLOCKS).grid, 1);  // max_ped 2: 90 lanes
        // the step chain of the same handle covers all 48
        CHECK_EQ(plan_tail_launch(h, step_chain(h), PV, OBS_POST_BLOCK, OBS_POST_MAX_BLOCKS).grid, (48 * PV + 255) / 256);
        CHECK_EQ(plan_actions_launch(h).grid, 1);
        // a device-side chain: the count is the device's, the grid a guess that the kernel strides over
        c.n_dev = true; c.act_nw = 16; c.act_hint = 24;
        CHECK_EQ(plan_tail_rows(h, c), 24);
        CHECK_EQ(plan_tail_launch(h, c, PV, OBS_POST_BLOCK, OBS_POST_MAX_BLOCKS).grid, (24 * PV + 255) / 256);
    }
    {   // the cap: 2^19 robots x 71 elements stride over 2048 blocks; the decode has no cap
        const PlanHandle h = handle(1, 1 << 19);
        CHECK_EQ(plan_tail_launch(h, step_chain(h), PV, OBS_POST_BLOCK, OBS_POST_MAX_BLOCKS).grid, 2048);
        CHECK_EQ(plan_actions_launch(h).grid, 2048);
    }
    if (g_fail) {
        printf("%d of %d checks failed\n", g_fail, g_checks);
        return 1;
    }
    printf("OK %d checks\n", g_checks);
    return 0;
}
