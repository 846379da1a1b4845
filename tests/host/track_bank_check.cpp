// track_bank_check.cpp -- the host half of imgenv_tracks_add (img_env_amd/csrc/track_bank.h: tracks_convert_set) without a device:
// one set of recorded tracks becomes what a reset stages for it.  Run over an odd Pw * stride and tracks of length 1; built with
// -fsanitize=address,undefined by tests/test_tracks_abi.py, so a write past a table or a read past a short input array fails it.
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -I include tests/host/track_bank_check.cpp -o check && ./check
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "../../img_env_amd/csrc/track_bank.h"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        g_checks++;                                                  \
        if (!(cond)) {                                               \
            g_fail++;                                                \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
        }                                                            \
    } while (0)

static bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0; }

struct Set {
    int Pw, cap;
    std::vector<double> pose, traj, traj_v;
    std::vector<int32_t> len;
};
static Set make_set(int Pw, int cap, const int* lens) {
    Set s{Pw, cap, std::vector<double>((size_t)Pw * 4), std::vector<double>((size_t)Pw * cap * 3), std::vector<double>((size_t)Pw * cap * 2),
          std::vector<int32_t>(lens, lens + Pw)};
    for (int j = 0; j < Pw; j++) {
        const double yaw = 0.3 * j - 1.0;
        s.pose[4 * j] = 1.5 + j; s.pose[4 * j + 1] = -2.25 * j; s.pose[4 * j + 2] = sin(yaw / 2); s.pose[4 * j + 3] = cos(yaw / 2);
        for (int q = 0; q < cap; q++) {  // (records behind the length hold junk that must not come through)
            const double junk = q >= lens[j] ? 1e6 : 0.0;
            double* t = &s.traj[((size_t)j * cap + q) * 3];
            t[0] = 0.1 * q + j + junk; t[1] = -0.2 * q + junk; t[2] = 0.01 * q + junk;
            double* v = &s.traj_v[((size_t)j * cap + q) * 2];
            v[0] = (q % 2 ? -0.3 : 0.4) + junk; v[1] = 0.05 * j - 0.1 * q + junk;
        }
    }
    return s;
}
static int convert(const Set& s, int stride, std::vector<double>& pose3, std::vector<double>& traj, std::vector<double>& traj_v, std::vector<int32_t>& len) {
    pose3.assign((size_t)s.Pw * 3, -7.0);
    traj.assign((size_t)s.Pw * stride * 3, -7.0);  // (exactly the size the library allocates: a write behind it is the sanitizer's)
    traj_v.assign((size_t)s.Pw * stride * 3, -7.0);
    len.assign(s.Pw, -7);
    return tracks_convert_set(s.Pw, s.cap, stride, s.pose.data(), s.traj.data(), s.traj_v.data(), s.len.data(), pose3.data(), traj.data(), traj_v.data(), len.data());
}

int main() {
    std::vector<double> pose3, traj, traj_v;
    std::vector<int32_t> len;
    {   // 3 pedestrians x 5 records (Pw * stride = 15, odd), lengths 1, 2, 5
        const int lens[3] = {1, 2, 5};
        const Set s = make_set(3, 5, lens);
        CHECK(convert(s, 5, pose3, traj, traj_v, len) == 0);
        for (int j = 0; j < 3; j++) {
            CHECK(len[j] == lens[j]);
            CHECK(same_bits(pose3[3 * j], s.pose[4 * j]) && same_bits(pose3[3 * j + 1], s.pose[4 * j + 1]));
            CHECK(same_bits(pose3[3 * j + 2], tf_yaw_from_quaternion_zw(s.pose[4 * j + 2], s.pose[4 * j + 3])));
            CHECK(fabs(pose3[3 * j + 2] - (0.3 * j - 1.0)) < 1e-12);
            for (int q = 0; q < 5; q++) {
                const double* t = &traj[((size_t)j * 5 + q) * 3];
                const double* v = &traj_v[((size_t)j * 5 + q) * 3];
                if (q < lens[j]) {
                    const double* ti = &s.traj[((size_t)j * 5 + q) * 3];
                    const double* vi = &s.traj_v[((size_t)j * 5 + q) * 2];
                    CHECK(same_bits(t[0], ti[0]) && same_bits(t[1], ti[1]) && same_bits(t[2], ti[2]));
                    CHECK(same_bits(v[0], vi[0]) && same_bits(v[1], vi[1]) && same_bits(v[2], atan2(vi[1], vi[0])));
                } else {
                    for (int e = 0; e < 3; e++) CHECK(same_bits(t[e], 0.0) && same_bits(v[e], 0.0));
                }
            }
        }
    }
    {   // cap 1 in a table of stride 2 (the handle's tables hold at least two records), every track of length 1
        const int lens[2] = {1, 1};
        const Set s = make_set(2, 1, lens);
        CHECK(convert(s, 2, pose3, traj, traj_v, len) == 0);
        for (int j = 0; j < 2; j++) {
            CHECK(same_bits(traj[((size_t)j * 2) * 3], s.traj[(size_t)j * 3]));
            CHECK(same_bits(traj_v[((size_t)j * 2) * 3 + 1], s.traj_v[(size_t)j * 2 + 1]));
            for (int e = 0; e < 3; e++) CHECK(same_bits(traj[((size_t)j * 2 + 1) * 3 + e], 0.0) && same_bits(traj_v[((size_t)j * 2 + 1) * 3 + e], 0.0));
        }
    }
    {   // refusals: a length of 0, a length beyond cap, a value that is not finite (also in a velocity), a zero quaternion
        const int lens[3] = {1, 2, 5};
        Set s = make_set(3, 5, lens);
        s.len[1] = 0;
        CHECK(convert(s, 5, pose3, traj, traj_v, len) == 2);
        s.len[1] = 6;
        CHECK(convert(s, 5, pose3, traj, traj_v, len) == 2);
        s = make_set(3, 5, lens);
        s.traj[((size_t)2 * 5 + 4) * 3 + 1] = std::numeric_limits<double>::quiet_NaN();
        CHECK(convert(s, 5, pose3, traj, traj_v, len) == -3);
        s = make_set(3, 5, lens);
        s.traj_v[0] = std::numeric_limits<double>::infinity();
        CHECK(convert(s, 5, pose3, traj, traj_v, len) == -1);
        s = make_set(3, 5, lens);
        s.traj[((size_t)0 * 5 + 3) * 3] = std::numeric_limits<double>::quiet_NaN();  // behind pedestrian 0's length: not read
        CHECK(convert(s, 5, pose3, traj, traj_v, len) == 0);
        s.pose[4 * 1 + 2] = s.pose[4 * 1 + 3] = 0.0;
        CHECK(convert(s, 5, pose3, traj, traj_v, len) == -2);
    }
    {   // the draws: in range, the salt is part of the definition, the cycle wraps
        for (int n : {1, 2, 3, 7}) {
            for (uint64_t seed = 0; seed < 1000; seed++) {
                const int32_t a = tracks_for_placement(seed, n);
                CHECK(a >= 0 && a < n && a == map_for_placement(seed + TRACKS_PLACEMENT_SALT, n));
            }
        }
        CHECK(tracks_for_placement(~0ull, 5) == map_for_placement(TRACKS_PLACEMENT_SALT - 1, 5));  // the sum wraps modulo 2^64
        const int want[7] = {0, 0, 1, 1, 2, 2, 0};
        for (int e = 0; e < 7; e++) CHECK(tracks_for_cycle((uint32_t)e, 2, 3) == want[e]);
        CHECK(tracks_for_cycle(0xFFFFFFFFu, 1, 1) == 0);
    }
    if (g_fail) {
        printf("%d of %d checks FAILED\n", g_fail, g_checks);
        return 1;
    }
    printf("OK %d checks\n", g_checks);
    return 0;
}
