// policy_check.cpp -- the host/device rules of img_env_amd/csrc/policy.h and the launch rule of launch_plan.h, compiled as plain
// C++ and walked over a simulated grid: every lane of every group of a launch of plan_policy_launch's shape runs the per-lane
// passes, the cross-lane folds are done here on arrays in the order policy.h states (xor butterfly, Hillis-Steele scan).  The
// expected values come from tests/policy_model.py through a vector file (tests/test_policy_host.py writes it):
//   PHILOX c0 c1 c2 c3 k0 k1 o0 o1 o2 o3                    (hex words)
//   DRAW g_lo g_hi draw_lo draw_hi seed_lo seed_hi second o0 o1 o2 o3
//   CAT R A G det robot_begin draw_lo draw_hi seed_lo seed_hi
//     then per row: ROW bad index s target  |  L <A words>  |  E <A words>  |  P <G words: lane sums>  |  S <G words: scan>
//   (floats as their bit patterns; L the logits, E the given e[])
//   g++ -std=c++17 -I include tests/host/policy_check.cpp -o check && ./check vectors.txt
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../img_env_amd/csrc/policy.h"

static int g_fail = 0, g_checks = 0;
#define CHECK_EQ(a, b)                                                                                     \
    do {                                                                                                   \
        g_checks++;                                                                                        \
        const long long a_ = (long long)(a), b_ = (long long)(b);                                          \
        if (a_ != b_) {                                                                                    \
            g_fail++;                                                                                      \
            if (g_fail < 40) printf("FAIL %s:%d: %s = %lld, expected %s = %lld\n", __FILE__, __LINE__, #a, a_, #b, b_); \
        }                                                                                                  \
    } while (0)

static uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// a lane's block with given e[]: what PolRegs / PolMem are to the kernel
struct GivenRow {
    const float* l;
    const float* given;
    int n;
    float at(int i) const { return l[i]; }
    float e(int i, float) const { return given[i]; }
    int count() const { return n; }
};

struct GroupResult {
    int bad, index;
    float s, target;
    std::vector<float> part, scan;
};
// one group of G lanes over one row, the folds in policy.h's order
static GroupResult run_group(const float* l, const float* e, int A, int G, float u, bool det) {
    std::vector<GivenRow> rows(G);
    std::vector<int> k0(G);
    std::vector<float> m(G), P(G), X(G);
    std::vector<int> bad(G);
    for (int j = 0; j < G; j++) {
        int n;
        pol_block(A, G, j, k0[j], n);
        rows[j] = {l + (n > 0 ? k0[j] : 0), e + (n > 0 ? k0[j] : 0), n};
        pol_lane_max(rows[j], m[j], bad[j]);
    }
    for (int d = 1; d < G; d <<= 1) {
        std::vector<float> m2(m);
        std::vector<int> b2(bad);
        for (int j = 0; j < G; j++) {
            const float y = m[j ^ d];
            m2[j] = y > m[j] ? y : m[j];
            b2[j] = bad[j] | bad[j ^ d];
        }
        m = m2; bad = b2;
    }
    for (int j = 0; j < G; j++) bad[j] |= m[j] == -INFINITY ? 1 : 0;
    GroupResult r;
    for (int j = 0; j < G; j++) P[j] = pol_lane_sum(rows[j], m[j]);
    r.part = P;
    for (int d = 1; d < G; d <<= 1) {
        std::vector<float> Q(P);
        for (int j = d; j < G; j++) Q[j] = P[j] + P[j - d];
        P = Q;
    }
    r.scan = P;
    for (int j = 0; j < G; j++) X[j] = j ? P[j - 1] : 0.0f;
    const float s = P[G - 1], log_s = logf(s), target = u * s;
    int cand = INT_MAX, last = -1;
    for (int j = 0; j < G; j++) {
        const PolLanePick pk = pol_lane_pick(rows[j], k0[j], m[j], X[j], s, log_s, target, det);
        cand = pk.cand < cand ? pk.cand : cand;  // (min / max: exact in any order)
        last = pk.last > last ? pk.last : last;
    }
    r.bad = bad[0];
    r.index = r.bad ? -1 : (cand != INT_MAX ? cand : last);
    r.s = s;
    r.target = target;
    return r;
}

static bool read_words(FILE* f, const char* tag, std::vector<uint32_t>& w, size_t n) {
    char t[16];
    if (fscanf(f, "%15s", t) != 1 || strcmp(t, tag) != 0) return false;
    w.resize(n);
    for (size_t q = 0; q < n; q++)
        if (fscanf(f, "%x", &w[q]) != 1) return false;
    return true;
}

static void launch_shapes() {
    const int As[] = {1, 16, 17, 64, 65, 256, 257, 1024, 1025, 4096}, Gs[] = {1, 1, 4, 4, 16, 16, 64, 64, 64, 64};
    for (int q = 0; q < 10; q++) {
        const int A = As[q], G = Gs[q];
        CHECK_EQ(plan_policy_group(A), G);
        CHECK_EQ(plan_policy_per_lane(A), (A + G - 1) / G);
        CHECK_EQ(plan_policy_per_lane(A) <= POL_REG, A <= 1024);  // registers up to 1024 logits, re-read beyond
        CHECK_EQ(WAVE % G, 0);                                   // a group never straddles a wavefront
        for (int R : {1, 256, 257}) {
            PlanHandle h;
            h.W = 1; h.Rw = R; h.R = h.RL = R;
            const LaunchShape s = plan_policy_launch(h, A);
            CHECK_EQ(s.block, POL_BLOCK);
            CHECK_EQ(s.block % WAVE, 0);
            CHECK_EQ(s.lds, 0);
            CHECK_EQ(s.grid, ((long long)R * G + 255) / 256);
            CHECK_EQ((long long)s.grid * s.block >= (long long)R * G, 1);
        }
        // the partition: every logit once, in order
        int next = 0;
        for (int j = 0; j < G; j++) {
            int k0, n;
            pol_block(A, G, j, k0, n);
            if (n > 0) CHECK_EQ(k0, next);
            next += n;
        }
        CHECK_EQ(next, A);
    }
    {   // the Gaussian and the values-only launch: a lane per robot; a shard launches its local rows
        PlanHandle h;
        h.W = 1; h.Rw = 1024; h.R = 1024; h.RL = 257; h.sharded = true;
        CHECK_EQ(plan_policy_launch(h, 0).grid, 2);
        CHECK_EQ(plan_policy_launch(h, 17).grid, (257 * 4 + 255) / 256);
    }
}

static void gaussian_rules() {
    const uint32_t x[4] = {0x12345678u, 0x9abcdef0u, 0, 0}, y[4] = {0x0fedcba9u, 0x87654321u, 0, 0};
    const float mean[3] = {0.25f, -1.5f, 3.0f}, ls[3] = {-0.5f, 0.0f, 1.0f};
    PolGaussRow d = pol_gauss_row(mean, ls, 3, x, y, true);  // the mode is the mean, bit for bit
    for (int c = 0; c < 3; c++) CHECK_EQ(bits(d.raw[c]), bits(mean[c] + 0.0f));
    CHECK_EQ(d.bad, 0);
    PolGaussRow s = pol_gauss_row(mean, ls, 2, x, y, false);
    CHECK_EQ(s.bad, 0);
    CHECK_EQ(bits(s.raw[2]), bits(0.0f));  // (column 2 of a two-column head is not drawn)
    float z0, z1;
    pol_box_muller(x[0], x[1], z0, z1);
    CHECK_EQ(bits(s.raw[0]), bits(mean[0] + expf(ls[0]) * z0));
    CHECK_EQ(bits(s.raw[1]), bits(mean[1] + expf(ls[1]) * z1));
    // u1 in (0, 1]: x0 = 0xffffffff gives 1, rho 0, z 0; x0 = 0 gives the largest rho, finite
    pol_box_muller(0xffffffffu, 0x40000000u, z0, z1);
    CHECK_EQ(z0 == 0.0f && z1 == 0.0f, 1);
    pol_box_muller(0u, 0u, z0, z1);
    CHECK_EQ(isfinite(z0) && z0 > 5.7f && z0 < 5.8f, 1);
    // bad rows: a mean, log_std, sigma or raw that is not finite
    const float nan_mean[3] = {NAN, 0, 0}, inf_mean[3] = {0, INFINITY, 0}, big_ls[3] = {0, 100.0f, 0}, nan_ls[3] = {0, 0, NAN};
    for (const PolGaussRow& b : {pol_gauss_row(nan_mean, ls, 3, x, y, false), pol_gauss_row(inf_mean, ls, 3, x, y, true),
                                 pol_gauss_row(mean, big_ls, 3, x, y, false), pol_gauss_row(mean, nan_ls, 3, x, y, false)}) {
        CHECK_EQ(b.bad, 1);
        CHECK_EQ(b.raw[0] == 0 && b.raw[1] == 0 && b.raw[2] == 0 && b.logp == 0 && b.entropy == 0, 1);
    }
    CHECK_EQ(pol_gauss_row(mean, nan_ls, 2, x, y, false).bad, 0);  // (a column the head does not have is not read)
    CHECK_EQ(bits(pol_clip(2.0f, -1.0f, 1.0f)), bits(1.0f));
    CHECK_EQ(bits(pol_clip(-2.0f, -1.0f, 1.0f)), bits(-1.0f));
    CHECK_EQ(bits(pol_clip(0.5f, -1.0f, 1.0f)), bits(0.5f));
    CHECK_EQ(bits(pol_u01(0xffffffffu)), bits(1.0f - 5.9604644775390625e-8f));
    CHECK_EQ(bits(pol_u01(0xffu)), bits(0.0f));
    CHECK_EQ(bits(pol_u01_open(0xffffffffu)), bits(1.0f));
    CHECK_EQ(bits(pol_u01_open(0u)), bits(5.9604644775390625e-8f));
}

int main(int argc, char** argv) {
    launch_shapes();
    gaussian_rules();
    if (argc < 2) {
        printf("usage: policy_check vectors.txt\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) {
        printf("cannot open %s\n", argv[1]);
        return 2;
    }
    char tag[16];
    int n_philox = 0, n_draw = 0, n_rows = 0;
    while (fscanf(f, "%15s", tag) == 1) {
        if (!strcmp(tag, "PHILOX")) {
            uint32_t w[10], out[4];
            for (int q = 0; q < 10; q++)
                if (fscanf(f, "%x", &w[q]) != 1) return 2;
            pol_philox(w[0], w[1], w[2], w[3], w[4], w[5], out);
            for (int q = 0; q < 4; q++) CHECK_EQ(out[q], w[6 + q]);
            n_philox++;
        } else if (!strcmp(tag, "DRAW")) {
            uint32_t w[11], out[4];
            for (int q = 0; q < 11; q++)
                if (fscanf(f, "%x", &w[q]) != 1) return 2;
            pol_draw(((uint64_t)w[1] << 32) | w[0], w[2], w[3], w[4], w[5], (int)w[6], out);
            for (int q = 0; q < 4; q++) CHECK_EQ(out[q], w[7 + q]);
            n_draw++;
        } else if (!strcmp(tag, "CAT")) {
            int R, A, G, det;
            unsigned long long g0;
            uint32_t dl, dh, sl, sh;
            if (fscanf(f, "%d %d %d %d %llu %x %x %x %x", &R, &A, &G, &det, &g0, &dl, &dh, &sl, &sh) != 9) return 2;
            CHECK_EQ(plan_policy_group(A), G);
            PlanHandle h;
            h.W = 1; h.Rw = R; h.R = h.RL = R;
            const LaunchShape shape = plan_policy_launch(h, A);
            std::vector<std::vector<uint32_t>> L(R), E(R), Pw(R), Sw(R);
            std::vector<int> want_bad(R), want_index(R);
            std::vector<uint32_t> want_s(R), want_t(R);
            for (int r = 0; r < R; r++) {
                char t[16];
                if (fscanf(f, "%15s %d %d %x %x", t, &want_bad[r], &want_index[r], &want_s[r], &want_t[r]) != 5 || strcmp(t, "ROW")) return 2;
                if (!read_words(f, "L", L[r], A) || !read_words(f, "E", E[r], A) || !read_words(f, "P", Pw[r], G) || !read_words(f, "S", Sw[r], G)) return 2;
            }
            // the simulated grid: every lane finds its row and its place in the group as the kernel does; rows are visited once,
            // by their lane 0, and the lanes behind the last row belong to no row
            std::vector<int> visits(R, 0);
            for (unsigned lane = 0; lane < shape.grid * shape.block; lane++) {
                const int r = (int)(lane / G), j = (int)(lane % G);
                if (r >= R || j != 0) continue;
                visits[r]++;
                std::vector<float> l(A), e(A);
                for (int k = 0; k < A; k++) { l[k] = from_bits(L[r][k]); e[k] = from_bits(E[r][k]); }
                uint32_t x[4];
                pol_draw(g0 + (unsigned long long)r, dl, dh, sl, sh, 0, x);
                const GroupResult got = run_group(l.data(), e.data(), A, G, pol_u01(x[0]), det != 0);
                CHECK_EQ(got.bad, want_bad[r]);
                CHECK_EQ(got.index, want_index[r]);
                if (!got.bad) {
                    CHECK_EQ(bits(got.s), want_s[r]);
                    CHECK_EQ(bits(got.target), want_t[r]);
                    for (int q = 0; q < G; q++) {
                        CHECK_EQ(bits(got.part[q]), Pw[r][q]);
                        CHECK_EQ(bits(got.scan[q]), Sw[r][q]);
                    }
                    if (got.index >= 0) CHECK_EQ(e[got.index] > 0.0f, 1);  // never a masked action
                }
                n_rows++;
            }
            for (int r = 0; r < R; r++) CHECK_EQ(visits[r], 1);
        } else {
            printf("unknown tag %s\n", tag);
            return 2;
        }
    }
    fclose(f);
    CHECK_EQ(n_philox >= 3, 1);
    CHECK_EQ(n_draw >= 1, 1);
    CHECK_EQ(n_rows >= 1, 1);
    if (g_fail) {
        printf("%d of %d checks failed\n", g_fail, g_checks);
        return 1;
    }
    printf("OK %d checks (%d philox, %d draws, %d rows)\n", g_checks, n_philox, n_draw, n_rows);
    return 0;
}
