// policy_loss_check.cpp -- the host/device rules of img_env_amd/csrc/policy_loss.h and the launch rule of launch_plan.h, compiled
// as plain C++ and walked over a simulated grid: every lane of every group of a launch of plan_policy_loss_launch's shape finds its
// row as the kernels do, the owner lane computes the row's terms, and the workgroup's fold and the final fold are done here on
// arrays in the order policy_loss.h states.  The expected values come from tests/policy_loss_model.py through a vector file
// (tests/test_policy_loss_host.py writes it), floats and doubles as their bit patterns:
//   CASE B A G clip_value clip clip_vf vf_coef ent_coef
//     per row:  ROW logp entropy r old_logp adv ret v old_v w bad | ratio pg vl kl clipped gu skip term [z0 z1 z2 sigma0 sigma1 sigma2]
//               (r: the given expf(logp - old_logp); bad: what the parameters said; A = 0 is the Gaussian launch, C = 3, whose rows
//               carry a given z and sigma: the three sums for a shared log_std ride in the records)
//     then:     REC n  <n * PLOSS_REC doubles>      the workgroups' records
//               SUM <PLOSS_REC doubles>             the final fold
//               TOT <8 stats> inv_W <3 dls> n_bad
//               per row:  VG gw grad [g gH dm0 dm1 dm2 dl0 dl1 dl2]   the value gradient for gw = w inv_W; A = 0: the Gaussian gradients
//   g++ -std=c++17 -ffp-contract=off -I include tests/host/policy_loss_check.cpp -o check && ./check vectors.txt
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../img_env_amd/csrc/policy_loss.h"

static int g_fail = 0, g_checks = 0;
#define CHECK_EQ(a, b)                                                                                     \
    do {                                                                                                   \
        g_checks++;                                                                                        \
        const long long a_ = (long long)(a), b_ = (long long)(b);                                          \
        if (a_ != b_) {                                                                                    \
            g_fail++;                                                                                      \
            if (g_fail < 40) printf("FAIL %s:%d: %s = %llx, expected %s = %llx\n", __FILE__, __LINE__, #a, a_, #b, b_); \
        }                                                                                                  \
    } while (0)

static uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static uint64_t bits64(double f) {
    uint64_t u;
    memcpy(&u, &f, 8);
    return u;
}
static bool read_f(FILE* f, float& x) {
    uint32_t u;
    if (fscanf(f, "%x", &u) != 1) return false;
    memcpy(&x, &u, 4);
    return true;
}
static bool read_d(FILE* f, double& x) {
    unsigned long long u;
    if (fscanf(f, "%llx", &u) != 1) return false;
    memcpy(&x, &u, 8);
    return true;
}

// the butterfly of a wavefront's 64 lanes, x = x + x[lane ^ d]
static void butterfly(std::vector<double>& x) {
    for (int d = 1; d < WAVE; d <<= 1) {
        std::vector<double> y(x);
        for (int l = 0; l < WAVE; l++) y[l] = x[l] + x[l ^ d];
        x = y;
    }
}

static void launch_shapes() {
    const int As[] = {0, 1, 16, 17, 64, 65, 256, 257, 1024, 1025}, Gs[] = {1, 1, 1, 4, 4, 16, 16, 64, 64, 64};
    for (int q = 0; q < 10; q++)
        for (int B : {1, 63, 65, 256, 257, 4096}) {
            const LaunchShape s = plan_policy_loss_launch(B, As[q]);
            CHECK_EQ(s.block, POL_BLOCK);
            CHECK_EQ(s.lds, 0);
            CHECK_EQ(s.grid, ((long long)B * Gs[q] + POL_BLOCK - 1) / POL_BLOCK);
            // every row has exactly one owner lane (lane j == 0 of its group) inside the grid
            CHECK_EQ((long long)(B - 1) * Gs[q] < (long long)s.grid * s.block, 1);
        }
    CHECK_EQ(POL_BLOCK % WAVE, 0);
    CHECK_EQ(PLOSS_REC, 10);
}

static void small_rules() {
    CHECK_EQ(ploss_action_index(0.0f, 3), 0);
    CHECK_EQ(ploss_action_index(2.0f, 3), 2);
    CHECK_EQ(ploss_action_index(3.0f, 3), -1);
    CHECK_EQ(ploss_action_index(-1.0f, 3), -1);
    CHECK_EQ(ploss_action_index(1.5f, 3), -1);
    CHECK_EQ(ploss_action_index(NAN, 3), -1);
    CHECK_EQ(ploss_action_index(-0.0f, 3), 0);
    CHECK_EQ(ploss_finite(1.0f), 1);
    CHECK_EQ(ploss_finite(INFINITY), 0);
    CHECK_EQ(ploss_finite(-INFINITY), 0);
    CHECK_EQ(ploss_finite(NAN), 0);
    // a masked logit's gradient is never computed; a finite one's: g (hit - p) - gH p (lp + H) with p = expf(lp)
    const float d = ploss_cat_grad(0.0f, 0.0f, logf(2.0f), logf(2.0f), 1.0f, 0.0f, true);
    CHECK_EQ(bits(d), bits(1.0f - expf(0.0f - logf(2.0f))));
    // the Gaussian row: the sampler's expressions on z = (raw - mean) / sigma
    const float mean[3] = {0.25f, -1.5f, 3.0f}, ls[3] = {-0.5f, 0.0f, 1.0f}, raw[3] = {0.5f, -1.0f, 2.0f};
    const PlossGauss g = ploss_gauss_row(mean, ls, raw, 3);
    float lp = 0.0f, H = 0.0f;
    for (int c = 0; c < 3; c++) {
        const float z = (raw[c] - mean[c]) / expf(ls[c]);
        CHECK_EQ(bits(g.z[c]), bits(z));
        lp = lp + (((-0.5f * z) * z - ls[c]) - POL_HALF_LN_2PI);
        H = H + (POL_ENT_CONST + ls[c]);
    }
    CHECK_EQ(bits(g.logp), bits(lp));
    CHECK_EQ(bits(g.entropy), bits(H));
    CHECK_EQ(g.bad, 0);
    const float nan_mean[3] = {NAN, 0, 0}, low_ls[3] = {-200.0f, 0, 0}, big_ls[3] = {0, 100.0f, 0}, inf_raw[3] = {0, 0, INFINITY};
    CHECK_EQ(ploss_gauss_row(nan_mean, ls, raw, 3).bad, 1);
    CHECK_EQ(ploss_gauss_row(mean, low_ls, raw, 3).bad, 1);  // sigma underflows to 0: z is not finite
    CHECK_EQ(ploss_gauss_row(mean, big_ls, raw, 3).bad, 1);
    CHECK_EQ(ploss_gauss_row(mean, ls, inf_raw, 3).bad, 1);
    CHECK_EQ(ploss_gauss_row(mean, ls, inf_raw, 2).bad, 0);  // (a column the head does not have is not read)
}

int main(int argc, char** argv) {
    launch_shapes();
    small_rules();
    if (argc < 2) {
        printf("usage: policy_loss_check vectors.txt\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) {
        printf("cannot open %s\n", argv[1]);
        return 2;
    }
    char tag[16];
    int n_cases = 0, n_rows = 0;
    while (fscanf(f, "%15s", tag) == 1) {
        if (strcmp(tag, "CASE")) {
            printf("unknown tag %s\n", tag);
            return 2;
        }
        int B, A, G, clip_value;
        float clip, clip_vf, vf_coef, ent_coef;
        if (fscanf(f, "%d %d %d %d", &B, &A, &G, &clip_value) != 4) return 2;
        if (!read_f(f, clip) || !read_f(f, clip_vf) || !read_f(f, vf_coef) || !read_f(f, ent_coef)) return 2;
        CHECK_EQ(plan_policy_group(A), G);
        const LaunchShape shape = plan_policy_loss_launch(B, A);
        struct Row { float logp, entropy, r, old_logp, adv, ret, v, old_v, w; int bad; float ratio, pg, vl, kl, clipped, gu; int skip; float term; float z[3], sigma[3]; };
        std::vector<Row> rows(B);
        for (int i = 0; i < B; i++) {
            Row& x = rows[i];
            if (fscanf(f, "%15s", tag) != 1 || strcmp(tag, "ROW")) return 2;
            float* in[] = {&x.logp, &x.entropy, &x.r, &x.old_logp, &x.adv, &x.ret, &x.v, &x.old_v, &x.w};
            for (float* p : in)
                if (!read_f(f, *p)) return 2;
            if (fscanf(f, "%d", &x.bad) != 1) return 2;
            float* out[] = {&x.ratio, &x.pg, &x.vl, &x.kl, &x.clipped, &x.gu};
            for (float* p : out)
                if (!read_f(f, *p)) return 2;
            if (fscanf(f, "%d", &x.skip) != 1 || !read_f(f, x.term)) return 2;
            for (int c = 0; c < 3; c++) x.z[c] = 0.0f, x.sigma[c] = 1.0f;
            if (A == 0)
                for (int c = 0; c < 6; c++)
                    if (!read_f(f, c < 3 ? x.z[c] : x.sigma[c - 3])) return 2;
        }
        // the simulated grid: a lane's row and place as in k_ploss_cat / k_ploss_gauss; the owner lane contributes
        const size_t lanes = (size_t)shape.grid * shape.block;
        std::vector<std::vector<double>> lane_acc(lanes, std::vector<double>(PLOSS_REC, 0.0));
        std::vector<int> visits(B, 0);
        for (size_t lane = 0; lane < lanes; lane++) {
            const int r = (int)(lane / G), j = (int)(lane % G);
            if (r >= B || j != 0) continue;
            visits[r]++;
            const Row& x = rows[r];
            const PlossRow t = ploss_row_terms_given(x.logp, x.bad != 0, x.r, x.old_logp, x.adv, x.ret, x.v, x.old_v, x.w, clip, clip_vf, clip_value != 0);
            const bool skip = t.bad || x.w == 0.0f;
            CHECK_EQ(skip, x.skip);
            if (!skip) {
                CHECK_EQ(bits(t.ratio), bits(x.ratio));
                CHECK_EQ(bits(t.pg), bits(x.pg));
                CHECK_EQ(bits(t.vl), bits(x.vl));
                CHECK_EQ(bits(t.kl), bits(x.kl));
                CHECK_EQ(bits(t.clipped), bits(x.clipped));
                CHECK_EQ(bits(t.gu), bits(x.gu));
                CHECK_EQ(bits(ploss_value_term(x.v, x.ret, x.old_v, clip_vf, clip_value != 0)), bits(x.term));
            }
            double acc[PLOSS_REC] = {0};
            ploss_contribute(t, x.entropy, x.w, skip, acc);
            if (A == 0)  // k_ploss_gauss
                for (int c = 0; c < 3; c++) acc[PLOSS_DLS + c] = skip ? 0.0 : (double)ploss_gauss_dls_term(t.gu, x.z[c], x.w, ent_coef);
            for (int k = 0; k < PLOSS_REC; k++) lane_acc[lane][k] = acc[k];
            n_rows++;
        }
        for (int i = 0; i < B; i++) CHECK_EQ(visits[i], 1);
        // the workgroup fold: the butterfly inside each wavefront, then the wavefronts ascending
        std::vector<std::vector<double>> rec(shape.grid, std::vector<double>(PLOSS_REC, 0.0));
        for (unsigned b = 0; b < shape.grid; b++)
            for (int k = 0; k < PLOSS_REC; k++) {
                double t = 0.0;
                for (int wv = 0; wv < POL_BLOCK / WAVE; wv++) {
                    std::vector<double> x(WAVE);
                    for (int l = 0; l < WAVE; l++) x[l] = lane_acc[(size_t)b * POL_BLOCK + wv * WAVE + l][k];
                    butterfly(x);
                    t = wv ? t + x[0] : x[0];
                }
                rec[b][k] = t;
            }
        int n_rec;
        if (fscanf(f, "%15s %d", tag, &n_rec) != 2 || strcmp(tag, "REC")) return 2;
        CHECK_EQ(n_rec, shape.grid);
        for (int b = 0; b < n_rec; b++)
            for (int k = 0; k < PLOSS_REC; k++) {
                double want;
                if (!read_d(f, want)) return 2;
                if (b < (int)shape.grid) CHECK_EQ(bits64(rec[b][k]), bits64(want));
            }
        // the final fold: lane t adds records t, t + 64, ... ascending from 0, then the butterfly
        double S[PLOSS_REC];
        for (int k = 0; k < PLOSS_REC; k++) {
            std::vector<double> x(WAVE, 0.0);
            for (int t = 0; t < WAVE; t++)
                for (unsigned q = t; q < shape.grid; q += PLOSS_FOLD_BLOCK) x[t] = x[t] + rec[q][k];
            butterfly(x);
            S[k] = x[0];
        }
        if (fscanf(f, "%15s", tag) != 1 || strcmp(tag, "SUM")) return 2;
        for (int k = 0; k < PLOSS_REC; k++) {
            double want;
            if (!read_d(f, want)) return 2;
            CHECK_EQ(bits64(S[k]), bits64(want));
        }
        const PlossTotals tot = ploss_totals(S, vf_coef, ent_coef);
        if (fscanf(f, "%15s", tag) != 1 || strcmp(tag, "TOT")) return 2;
        float want;
        for (int k = 0; k < 8; k++) {
            if (!read_f(f, want)) return 2;
            CHECK_EQ(bits(tot.stats[k]), bits(want));
        }
        if (!read_f(f, want)) return 2;
        CHECK_EQ(bits(tot.inv_W), bits(want));
        for (int c = 0; c < 3; c++) {
            if (!read_f(f, want)) return 2;
            CHECK_EQ(bits(tot.dls[c]), bits(want));
        }
        int want_bad;
        if (fscanf(f, "%d", &want_bad) != 1) return 2;
        CHECK_EQ(tot.n_bad, want_bad);
        for (int i = 0; i < B; i++) {
            float gw, grad;
            if (fscanf(f, "%15s", tag) != 1 || strcmp(tag, "VG") || !read_f(f, gw) || !read_f(f, grad)) return 2;
            const Row& x = rows[i];
            const float got = x.skip ? 0.0f : ploss_value_grad(vf_coef, gw, ploss_value_term(x.v, x.ret, x.old_v, clip_vf, clip_value != 0));
            CHECK_EQ(bits(got), bits(grad));
            if (A == 0) {  // k_ploss_grad_gauss
                float g, gH, want_d[6];
                if (!read_f(f, g) || !read_f(f, gH)) return 2;
                for (float& d : want_d)
                    if (!read_f(f, d)) return 2;
                for (int c = 0; c < 3; c++) {
                    CHECK_EQ(bits(x.skip ? 0.0f : ploss_gauss_grad_mean(g, x.z[c], x.sigma[c])), bits(want_d[c]));
                    CHECK_EQ(bits(x.skip ? 0.0f : ploss_gauss_grad_ls(g, x.z[c], gH)), bits(want_d[3 + c]));
                }
            }
        }
        n_cases++;
    }
    fclose(f);
    CHECK_EQ(n_cases >= 4, 1);
    CHECK_EQ(n_rows >= 100, 1);
    if (g_fail) {
        printf("%d of %d checks failed\n", g_fail, g_checks);
        return 1;
    }
    printf("OK %d checks (%d cases, %d rows)\n", g_checks, n_cases, n_rows);
    return 0;
}
