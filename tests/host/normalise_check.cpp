// The per-lane functions of img_env_amd/csrc/normalise.h, compiled for the host and run over a simulated grid: every workgroup of
// k_norm_part and k_norm_apply lane by lane, the folds across lanes through norm_fold (the order the device's shuffles and LDS
// step take), the turn counters as launch_views keeps them.  tests/test_normalise_plan.py writes the cases, and compares what this
// leaves after every chain bit for bit with tests/normalise_model.py.
//
//   normalise_check plan                 -> "OK NORM_BLOCK .. NORM_PER_LANE .. NORM_MAX_COLS .. NORM_MAX_BLOCKS .."
//   normalise_check run CASE RESULT      -> "OK chains N"
// CASE: i32 R Rw D K flags n_chains | f64 gamma clip_obs clip_reward eps | per chain: i32 kind training grid_part grid_apply
//   (0: the planner's), f32 vector_states [R][D], f32 state_stack [R][K][D]; a step: f64 rewards [R], u8 is_clean [R], u8 dones [R];
//   a reset: i32 mode (0 no list, 1 the host's count, 2 a device-side count) n worlds[n].
// RESULT, per chain: f64 stats [4 + 2 D] and f64 returns [R] of the words in turn, f32 norm_vector_states [R][D], f32
//   norm_state_stack [R][K][D], f64 norm_rewards [R].
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../img_env_amd/csrc/normalise.h"

static FILE* g_in;
template <typename T>
static bool take(T* p, size_t n) {
    return n == 0 || fread(p, sizeof(T), n, g_in) == n;
}
template <typename T>
static void put(FILE* out, const T* p, size_t n) {
    if (n) fwrite(p, sizeof(T), n, out);
}

template <bool RESTART>
static void run_part(const NormDev& n, unsigned grid) {
    const bool listed = RESTART && n.rows.list != nullptr;
    const size_t covered = tail_rows_count(n.rows, listed), tiles = norm_tiles(n, covered);
    for (unsigned b = 0; b < grid; b++)
        for (size_t tile = b; tile < tiles; tile += grid) {
            double x[NORM_BLOCK][NORM_PER_LANE], a[NORM_BLOCK];
            uint32_t have[NORM_BLOCK], cnt[NORM_BLOCK];
            for (uint32_t t = 0; t < NORM_BLOCK; t++) {
                have[t] = norm_part_load<RESTART>(n, listed, covered, tile, norm_lane(n.cols, t), x[t]);
                cnt[t] = (uint32_t)__builtin_popcount(have[t]);
            }
            for (int col = 0; col < n.cols; col++) {
                uint32_t cc[NORM_BLOCK];
                memcpy(cc, cnt, sizeof(cc));
                const uint32_t c = norm_fold<uint32_t>(cc, n.cols, col);
                for (uint32_t t = 0; t < NORM_BLOCK; t++) a[t] = norm_lane_sum(x[t], have[t]);
                const double mean = norm_part_mean(norm_fold<double>(a, n.cols, col), c);
                for (uint32_t t = 0; t < NORM_BLOCK; t++) a[t] = norm_lane_squares(x[t], have[t], mean);
                norm_part_store(n, tile, col, c, mean, norm_fold<double>(a, n.cols, col));
            }
        }
}

template <bool RESTART>
static void run_apply(const NormDev& n, unsigned grid) {
    const bool listed = RESTART && n.rows.list != nullptr;
    const size_t covered = tail_rows_count(n.rows, listed);
    const int rpw = plan_norm_rows_per_wave(n.cols);
    for (unsigned b = 0; b < grid; b++)
        for (uint32_t t = 0; t < NORM_BLOCK; t++) {
            const NormLane id = norm_lane(n.cols, t);
            NormTriple s = norm_stats_load(n, norm_stats_cur(n), id.col);
            if (n.update && (!RESTART || n.n_obs)) {
                s = norm_merge(s, norm_batch(n, norm_tiles(n, covered), id.col));
                if (b == 0 && (int)t < n.cols) norm_stats_store(n, id.col, s);
            }
            if (id.r >= rpw) continue;
            const double den = sqrt(s.var + n.eps);
            const size_t pass = (size_t)grid * (size_t)(NORM_WAVES * rpw);
            for (size_t m = ((size_t)b * NORM_WAVES + (size_t)id.w) * (size_t)rpw + (size_t)id.r; m < covered; m += pass)
                norm_apply_item<RESTART>(n, listed, m, id.col, s.mean, den);
        }
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "plan")) {
        // the shapes the planner gives: one workgroup per tile, capped; a tile is what four wavefronts hold NORM_PER_LANE deep
        PlanHandle h;
        PlanChain c;
        h.RL = 4096;
        h.Rw = 4;
        bool ok = plan_norm_rows_per_wave(6) == 10 && plan_norm_tile_rows(6) == 4 * 10 * NORM_PER_LANE && plan_norm_tiles(4096, 6) == 13;
        ok = ok && plan_norm_part_launch(h, c, 6).grid == 13 && plan_norm_part_launch(h, c, 6).block == NORM_BLOCK;
        ok = ok && plan_norm_apply_launch(h, c, 6).grid == (4096 + 39) / 40 && plan_norm_rows_per_wave(64) == 1 && plan_norm_rows_per_wave(1) == 64;
        h.RL = 1 << 22;
        ok = ok && plan_norm_part_launch(h, c, 1).grid == NORM_MAX_BLOCKS && plan_norm_apply_launch(h, c, 8).grid == NORM_MAX_BLOCKS;
        ok = ok && norm_half0(1) == 0 && norm_half0(2) == 1 && norm_half0(9) == 8 && norm_half0(10) == 8 && norm_half0(64) == 32 && norm_half0(8) == 4;
        if (!ok) return printf("FAIL: plan\n"), 1;
        printf("OK NORM_BLOCK %d NORM_PER_LANE %d NORM_MAX_COLS %d NORM_MAX_BLOCKS %d\n", NORM_BLOCK, NORM_PER_LANE, NORM_MAX_COLS, NORM_MAX_BLOCKS);
        return 0;
    }
    if (argc < 4 || strcmp(argv[1], "run")) return printf("usage: normalise_check plan | run CASE RESULT\n"), 2;
    g_in = fopen(argv[2], "rb");
    FILE* out = fopen(argv[3], "wb");
    if (!g_in || !out) return printf("FAIL: files\n"), 2;
    int32_t head[6];
    double par[4];
    if (!take(head, 6) || !take(par, 4)) return printf("FAIL: header\n"), 2;
    const int R = head[0], Rw = head[1], D = head[2], K = head[3], flags = head[4], n_chains = head[5];
    if (R < 1 || Rw < 1 || R % Rw || D < 1 || D + 1 > NORM_MAX_COLS || K < 0 || !(flags & 3)) return printf("FAIL: bad header\n"), 2;
    const bool obs = flags & IMGENV_NORM_OBS, rew = flags & IMGENV_NORM_REWARD;
    const size_t words = NORM_STATS_WORDS(D);
    const int cols_max = std::max(1, (obs ? D : 0) + (rew ? 1 : 0));
    const size_t tiles = std::max(plan_norm_tiles((size_t)R, cols_max), plan_norm_tiles((size_t)R, std::max(1, obs ? D : 0)));
    // exact sizes: the sanitizer build finds any index past an array's end
    std::vector<float> vs((size_t)R * D), stack((size_t)R * K * D), nvs((size_t)R * D, 0.0f), nstack((size_t)R * K * D, 0.0f);
    std::vector<double> rewards(R), stats(2 * words, 0.0), returns(2 * (size_t)R, 0.0), part(tiles * (size_t)cols_max * 2), nrew(R, 0.0);
    std::vector<uint8_t> clean(R), dones(R);
    std::vector<uint32_t> part_n(tiles);
    std::vector<int> list(R / Rw + 1);
    int n_dev = 0;
    for (int q = 0; q < 2; q++) {
        double* s = stats.data() + q * words;
        s[0] = s[1] = 1e-4;
        s[3] = 1.0;
        for (int d = 0; d < D; d++) s[4 + D + d] = 1.0;
    }
    NormDev base;
    memset(&base, 0, sizeof(base));
    base.vector_states = vs.data();
    base.state_stack = obs && K ? stack.data() : nullptr;
    base.rewards = rewards.data();
    base.is_clean = clean.data();
    base.dones = dones.data();
    base.stats = stats.data();
    base.returns = rew ? returns.data() : nullptr;
    base.part = part.data();
    base.part_n = part_n.data();
    base.norm_vector_states = obs ? nvs.data() : nullptr;
    base.norm_state_stack = obs && K ? nstack.data() : nullptr;
    base.norm_rewards = rew ? nrew.data() : nullptr;
    base.gamma = par[0]; base.clip_obs = par[1]; base.clip_reward = par[2]; base.eps = par[3];
    base.D = D;
    base.K = obs ? K : 0;
    base.n_obs = obs ? D : 0;
    uint32_t turn = 0, ret_turn = 0;
    PlanHandle ph;
    ph.RL = R;
    ph.Rw = Rw;
    ph.W = R / Rw;
    for (int q = 0; q < n_chains; q++) {
        int32_t ch[4];
        if (!take(ch, 4) || !take(vs.data(), vs.size()) || !take(stack.data(), stack.size())) return printf("FAIL: chain %d\n", q), 2;
        const bool is_reset = ch[0] != 0;
        NormDev n = base;
        PlanChain pc;
        pc.is_reset = is_reset;
        n.rows = {R, Rw, nullptr, nullptr, R / Rw};
        if (is_reset) {
            int32_t mode[2];
            if (!take(mode, 2) || mode[1] < 0 || mode[1] > R / Rw || !take(list.data(), (size_t)mode[1])) return printf("FAIL: reset %d\n", q), 2;
            if (mode[0] != 0) {
                n.rows.list = list.data();
                n.rows.n_worlds = mode[0] == 2 ? R / Rw : mode[1];  // (a device-side count wins over the host's)
                n_dev = mode[1];
                n.rows.n_dev = mode[0] == 2 ? &n_dev : nullptr;
                pc.listed = true;
                pc.n_dev = mode[0] == 2;
                pc.act_nw = n.rows.n_worlds;
                pc.act_hint = Rw;
            }
        } else if (!take(rewards.data(), (size_t)R) || !take(clean.data(), (size_t)R) || !take(dones.data(), (size_t)R)) {
            return printf("FAIL: step %d\n", q), 2;
        }
        // (launch_views' part)
        n.n_ret = !is_reset && rew ? 1 : 0;
        n.cols = std::max(1, n.n_obs + n.n_ret);
        n.update = ch[1] ? 1 : 0;
        n.turn = turn;
        n.ret_turn = ret_turn;
        const bool stats_move = n.update && (!is_reset || n.n_obs > 0);
        if (stats_move) {
            const unsigned grid = ch[2] > 0 ? (unsigned)ch[2] : plan_norm_part_launch(ph, pc, n.cols).grid;
            is_reset ? run_part<true>(n, grid) : run_part<false>(n, grid);
            turn += 1;
        }
        if (!is_reset || n.n_obs > 0 || (n.update && rew)) {
            const unsigned grid = ch[3] > 0 ? (unsigned)ch[3] : plan_norm_apply_launch(ph, pc, n.cols).grid;
            is_reset ? run_apply<true>(n, grid) : run_apply<false>(n, grid);
        }
        if (n.update && n.n_ret) ret_turn += 1;
        put(out, stats.data() + (size_t)(turn & 1) * words, words);
        put(out, returns.data() + (size_t)(ret_turn & 1) * R, (size_t)R);
        put(out, nvs.data(), nvs.size());
        put(out, nstack.data(), nstack.size());
        put(out, nrew.data(), nrew.size());
    }
    fclose(out);
    fclose(g_in);
    printf("OK chains %d\n", n_chains);
    return 0;
}
