// launch_plan_tracks_check.cpp -- the shape of k_tracks_install (img_env_amd/csrc/launch_plan.h: plan_tracks_install): one
// workgroup per world of a host chain, the device chain's guess of finished worlds otherwise (the workgroups stride over the count
// the device holds), and the copy of a world's tables in 8-byte words -- never a wider unit, because an odd Pw * stride leaves every
// other world's rows 8-byte aligned only.  Expected values are written down from include/imgenv.h ("track bank").
//   g++ -std=c++17 -I include tests/host/launch_plan_tracks_check.cpp -o check && ./check
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

static PlanHandle handle(int W, int Rw, int Pw) {
    PlanHandle h;
    h.W = W; h.Rw = Rw; h.Pw = Pw; h.R = h.RL = W * Rw; h.P = W * Pw;
    return h;
}

int main() {
    {   // host chains: zero worlds (nothing to launch), one world, several
        const PlanHandle h = handle(5, 2, 3);
        CHECK_EQ(plan_tracks_install(h, 0, false, 0, 5).install.grid, 0);
        CHECK_EQ(plan_tracks_install(h, -1, false, 0, 5).install.grid, 0);
        const TracksPlan one = plan_tracks_install(h, 1, false, 0, 5);
        CHECK_EQ(one.install.grid, 1);
        CHECK_EQ(one.install.block, 256);
        CHECK_EQ(one.install.block, TRACKS_BLOCK);
        CHECK_EQ(one.install.lds, 0);
        CHECK_EQ(plan_tracks_install(h, 5, false, 99, 5).install.grid, 5);  // (the hint plays no part where the host knows the list)
    }
    {   // Pw * stride odd (3 pedestrians x 5 records): 45 words of 8 bytes per table, 360 bytes -- world 1's rows start 8-byte aligned only
        const PlanHandle h = handle(5, 2, 3);
        const TracksPlan t = plan_tracks_install(h, 2, false, 0, 5);
        CHECK_EQ(t.words, 45);
        CHECK_EQ(t.words * 8 % 16, 8);
        CHECK_EQ(t.rounds, 1);
        CHECK_EQ(plan_tracks_install(h, 2, false, 0, 0).words, 0);
        CHECK_EQ(plan_tracks_install(h, 2, false, 0, 0).rounds, 0);
    }
    {   // the example of the header: 10 pedestrians of 50 records are 1500 words per table (24 KB for both), 6 rounds of 256 lanes
        const TracksPlan t = plan_tracks_install(handle(1024, 4, 10), 1, false, 0, 50);
        CHECK_EQ(t.words, 1500);
        CHECK_EQ(2 * t.words * 8, 24000);
        CHECK_EQ(t.rounds, 6);
        CHECK_EQ(plan_tracks_install(handle(1, 1, 1), 1, false, 0, 256).rounds, 3);   // 768 words: exactly three rounds
        CHECK_EQ(plan_tracks_install(handle(1, 1, 1), 1, false, 0, 86).rounds, 2);    // 258 words: one past a round
    }
    {   // the device chain: the grid is plan_dev_reset's guess, whatever n_worlds says -- min(W, max(16, 4 * last count))
        const PlanHandle h = handle(70, 1, 2);
        CHECK_EQ(plan_tracks_install(h, 0, true, 0, 4).install.grid, 16);    // 70 worlds finishing at once stride over 16 workgroups
        CHECK_EQ(plan_tracks_install(h, 0, true, 0, 4).install.grid, plan_dev_reset(h, 0, 0).guess);
        CHECK_EQ(plan_tracks_install(h, 0, true, 4, 4).install.grid, 16);
        CHECK_EQ(plan_tracks_install(h, 0, true, 5, 4).install.grid, 20);
        CHECK_EQ(plan_tracks_install(h, 0, true, 70, 4).install.grid, 70);   // never more than the handle has worlds
        CHECK_EQ(plan_tracks_install(h, 0, true, -3, 4).install.grid, 16);
        CHECK_EQ(plan_tracks_install(handle(5, 2, 3), 0, true, 0, 5).install.grid, 5);
        CHECK_EQ(plan_tracks_install(handle(1, 2, 3), 0, true, 0, 5).install.grid, 1);
        CHECK_EQ(plan_tracks_install(h, 0, true, 0, 4).install.block, 256);
    }
    if (g_fail) {
        printf("%d of %d checks FAILED\n", g_fail, g_checks);
        return 1;
    }
    printf("OK %d checks\n", g_checks);
    return 0;
}
