// raster_pack_pose_check.cpp -- for tests/test_gpu_raster_pack.py: which poses of a disc robot the lattice rows of fp_rows.h
// certify (k_raster_pack draws those itself and hands the others to raster_robot's literal walk), and which cells the footprint
// covers there by the literal walk (Agent::draw, agent.cpp:285-327), as tests/host/fp_rows_check.cpp does it.
//   raster_pack_pose_check <radius> <res> < poses      one pose per line: x y sin(yaw / 2) cos(yaw / 2), as a robot record holds them
// Prints per pose: <1 certified | 0 not> <hash of the covered cells>
#include <stdio.h>
#include <stdlib.h>

#include <set>

#define WAVE_SZ 64
#include "../../img_env_amd/csrc/host_tables.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    double s[4] = {0.0, 0.0, (double)(float)atof(argv[1]), 0.0};
    const double res = (double)(float)atof(argv[2]);
    const Pts p = shape_circle(s[0], s[1], s[2]);
    const std::vector<FpRow> rows = build_fp_rows(p, s[1], res);
    if (rows.empty()) return 3;
    char line[512];
    while (fgets(line, sizeof(line), stdin)) {
        char* q = line;
        double v[4];
        for (double& x : v) x = strtod(q, &q);
        const Tf2 bw = tf_from_pose_sc(v[0], v[1], v[2], v[3]);
        const FpRowsPose P = fpr_pose(bw.m00, bw.m01, bw.m10, bw.m11, bw.ox, bw.oy, s[1], res);
        bool all = true;
        for (const FpRow& r : rows) {
            FpAxis ax, ay;
            all = fpr_row(P, r, ax, ay) && all;
        }
        std::set<std::pair<int, int>> cells;
        for (int k = 0; k < p.n(); k++) {
            double wx, wy;
            tf_apply(bw, p.x[k], p.y[k], wx, wy);
            cells.insert({w2m(wx, res), w2m(wy, res)});
        }
        unsigned long long hash = 1469598103934665603ull;
        for (const auto& c : cells) {
            hash = (hash ^ (unsigned long long)(unsigned)c.first) * 1099511628211ull;
            hash = (hash ^ (unsigned long long)(unsigned)c.second) * 1099511628211ull;
        }
        printf("%d %llu\n", all ? 1 : 0, hash);
    }
    return 0;
}
