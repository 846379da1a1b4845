// episode_log_check.cpp -- the per-row rules of the episode log (img_env_amd/csrc/episode_log.h) on the CPU, walked the way
// k_episode_log walks them: one workgroup of 1024 lanes in 16 wavefronts, a first pass that counts the open episodes of the chain, a
// second pass over chunks of 1024 covered rows with a ballot per wavefront, the wave counts, a running base -- against a plain
// sequential append.  The episodes are built by ep_accumulate itself, and the logged figures are held to what ep_fold then adds to
// a robot's (zeroed) figure sums.
//   g++ -std=c++17 -fsanitize=address,undefined tests/host/episode_log_check.cpp -o check && ./check
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../../img_env_amd/csrc/episode_log.h"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        g_checks++;                                                  \
        if (!(cond)) {                                               \
            g_fail++;                                                \
            if (g_fail < 20) printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                            \
    } while (0)

static const int BLOCK = EPLOG_BLOCK, WAVES = EPLOG_BLOCK / WAVE;

// k_episode_log, lane by lane
static void chunked_append(const EpisodesDev& e, const EpisodeLogDev& g) {
    const bool listed = e.rows.list != nullptr;
    const size_t total = tail_rows_count(e.rows, listed);
    const unsigned long long n0 = *g.n_written;
    int wave_n[WAVES];
    for (int wv = 0; wv < WAVES; wv++) wave_n[wv] = 0;
    for (size_t k0 = 0; k0 < total; k0 += BLOCK)
        for (int tid = 0; tid < BLOCK; tid++) {
            const size_t m = k0 + tid;
            if (m < total && eplog_open(e, tail_rows_row(e.rows, listed, m))) wave_n[tid / WAVE] += 1;
        }
    unsigned long long n_end = n0;
    for (int wv = 0; wv < WAVES; wv++) n_end += (unsigned long long)wave_n[wv];
    unsigned long long base = n0;
    for (size_t k0 = 0; k0 < total; k0 += BLOCK) {
        unsigned long long mask[WAVES];
        for (int wv = 0; wv < WAVES; wv++) {
            mask[wv] = 0;
            for (int lane = 0; lane < WAVE; lane++) {
                const size_t m = k0 + (size_t)wv * WAVE + lane;
                if (m < total && eplog_open(e, tail_rows_row(e.rows, listed, m))) mask[wv] |= 1ull << lane;
            }
            wave_n[wv] = __builtin_popcountll(mask[wv]);
        }
        // lanes in a scrambled order: nothing may depend on which lane stores first
        for (int t = 0; t < BLOCK; t++) {
            const int tid = (t * 389) % BLOCK, wv = tid / WAVE, lane = tid % WAVE;
            const size_t m = k0 + tid;
            if (m >= total) continue;
            const size_t row = tail_rows_row(e.rows, listed, m);
            unsigned long long before = base;
            for (int q = 0; q < wv; q++) before += (unsigned long long)wave_n[q];
            if (mask[wv] >> lane & 1ull) {
                const unsigned long long seq = before + (unsigned long long)__builtin_popcountll(mask[wv] & ((1ull << lane) - 1ull));
                if (eplog_kept(seq, n_end, g.capacity)) eplog_record(e, g, row, seq);
            }
            eplog_retag(e, g, row);
        }
        for (int wv = 0; wv < WAVES; wv++) base += (unsigned long long)wave_n[wv];
    }
    *g.n_written = n_end;
}

struct Rec {
    int32_t i[EPL_I32_ROWS];
    double f[EPL_F64_ROWS];
    unsigned long long placement;
};

struct Handle {
    int RL, Rw, W, min_steps, capacity;
    std::vector<double> f;
    std::vector<int32_t> i, codes, tags, ring_i;
    std::vector<float> actions;
    std::vector<double> rewards, ring_f;
    std::vector<uint8_t> clean;
    std::vector<unsigned long long> tag_place, ring_p, n_written;
    std::vector<int> map_cur, trk_cur, scn_world;
    std::vector<unsigned long long> scn_mark, place_serial;
    EpisodesDev e;
    EpisodeLogDev g;
    Handle(int RL_, int Rw_, int capacity_, int min_steps_) : RL(RL_), Rw(Rw_), W(RL_ / Rw_), min_steps(min_steps_), capacity(capacity_) {
        f.assign((size_t)EPF_ROWS * RL, 0.0);
        i.assign((size_t)EPI_ROWS * RL, 0);
        codes.assign(RL, 0);
        actions.assign((size_t)RL * 3, 0.f);
        rewards.assign(RL, 0.0);
        clean.assign(RL, 1);
        tags.assign((size_t)EPT_ROWS * RL, -1);
        tag_place.assign(RL, ~0ull);
        ring_i.assign((size_t)EPL_I32_ROWS * capacity, 0);
        ring_f.assign((size_t)EPL_F64_ROWS * capacity, 0.0);
        ring_p.assign(capacity, 0);
        n_written.assign(1, 0);
        map_cur.assign(W, 0); trk_cur.assign(W, 0); scn_world.assign(W, 0); scn_mark.assign(W, 0); place_serial.assign(W, 0);
        memset(&e, 0, sizeof(e));
        e.f = f.data(); e.i = i.data(); e.actions = actions.data(); e.step_rewards = rewards.data(); e.step_is_clean = clean.data();
        e.step_dones_info = codes.data(); e.dt = 0.25; e.min_steps = min_steps;
        e.rows = TailRows{RL, Rw, nullptr, nullptr, W};
        memset(&g, 0, sizeof(g));
        g.n_written = n_written.data(); g.i32 = ring_i.data(); g.f64 = ring_f.data(); g.placement = ring_p.data(); g.capacity = capacity;
        g.W = W; g.tags = tags.data(); g.tag_place = tag_place.data();
        g.map_cur = map_cur.data(); g.trk_cur = trk_cur.data(); g.scn_world = scn_world.data(); g.scn_mark = scn_mark.data();
        g.place_serial = place_serial.data();
    }
};

// one chain over `covered` rows of a handle whose rows are in random states, into a ring of `capacity`
static void run_case(int covered, int Rw, bool listed, bool count_on_device, int capacity, unsigned seed) {
    std::mt19937 rng(seed);
    const int extra_worlds = listed ? 3 : 0, W = covered / Rw + extra_worlds, RL = W * Rw;
    Handle h(RL, Rw, capacity, 3);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    // episodes of 0 .. 9 steps; a fifth of the rows have none open
    for (int r = 0; r < RL; r++) h.i[(size_t)EPI_OPEN * RL + r] = rng() % 5 != 0;
    for (int s = 0; s < 9; s++) {
        for (int r = 0; r < RL; r++) {
            h.actions[3 * r] = (float)u(rng);
            h.actions[3 * r + 1] = rng() % 4 == 0 ? 0.f : (float)u(rng);
            h.rewards[r] = u(rng);
            h.clean[r] = rng() % 7 != 0;
        }
        for (int r = 0; r < RL; r++)
            if ((int)(rng() % 10) > s) ep_accumulate(h.e, (size_t)r);
    }
    for (int r = 0; r < RL; r++) {
        h.codes[r] = (int)(rng() % 12);
        h.i[(size_t)EPI_EPISODES * RL + r] = (int)(rng() % 5);
        for (int k = 0; k < EPT_ROWS; k++) h.tags[(size_t)k * RL + r] = (int)(rng() % 50) - 2;
        h.tag_place[r] = rng();
    }
    for (int w = 0; w < W; w++) {
        h.map_cur[w] = (int)(rng() % 4); h.trk_cur[w] = (int)(rng() % 6) - 1; h.scn_world[w] = (int)(rng() % 9) - 1;
        h.place_serial[w] = rng() % 3 == 0 ? ~0ull : rng() % 100;
        h.scn_mark[w] = rng() % 2 ? h.place_serial[w] : 12345ull;
    }
    h.n_written[0] = rng() % 3 == 0 ? 0 : rng() % 10000;  // the ring is in mid-turn
    std::vector<int> list;
    int n_dev = covered / Rw;
    if (listed) {
        for (int w = 0; w < W; w++) list.push_back(w);
        std::shuffle(list.begin(), list.end(), rng);
        h.e.rows.list = list.data();
        h.e.rows.n_worlds = count_on_device ? W : covered / Rw;
        h.e.rows.n_dev = count_on_device ? &n_dev : nullptr;
    }
    CHECK(tail_rows_count(h.e.rows, listed) == (size_t)covered);
    // the straightforward version: walk the covered rows, append, keep the last `capacity`
    const unsigned long long n0 = h.n_written[0];
    std::vector<Rec> want;
    std::vector<int32_t> want_tags = h.tags;
    std::vector<unsigned long long> want_place = h.tag_place;
    std::vector<int32_t> ring_i0 = h.ring_i;
    for (int m = 0; m < covered; m++) {
        const int row = listed ? list[m / Rw] * Rw + m % Rw : m, w = row / Rw;
        if (h.i[(size_t)EPI_OPEN * RL + row]) {
            Rec r;
            const int steps = h.i[(size_t)EPI_TMP_STEPS * RL + row];
            const bool counted = steps > h.min_steps;
            const int32_t vals[EPL_I32_ROWS] = {row, w, h.codes[row], steps, h.i[(size_t)EPI_LEN * RL + row], counted ? 1 : 0,
                                                counted ? h.i[(size_t)EPI_EPISODES * RL + row] + 1 : 0, h.tags[(size_t)EPT_MAP * RL + row],
                                                h.tags[(size_t)EPT_TRACKS * RL + row], h.tags[(size_t)EPT_SCENARIO * RL + row]};
            memcpy(r.i, vals, sizeof(vals));
            r.f[EPL_RETURN] = h.f[(size_t)EPF_RETURN * RL + row];
            for (int k = 0; k < 8; k++) r.f[EPL_FIG0 + k] = 0.0;  // (counted: filled from the fold below)
            r.placement = h.tag_place[row];
            want.push_back(r);
        }
        want_tags[(size_t)EPT_MAP * RL + row] = h.map_cur[w];
        want_tags[(size_t)EPT_TRACKS * RL + row] = h.trk_cur[w];
        want_tags[(size_t)EPT_SCENARIO * RL + row] = h.scn_mark[w] == h.place_serial[w] ? h.scn_world[w] : EPLOG_SCN_DEVICE;
        want_place[row] = h.place_serial[w];
    }
    chunked_append(h.e, h.g);
    // the fold behind the log: from zeroed sums, what it adds IS the episode's figures
    for (int k = 0; k < 8; k++)
        for (int r = 0; r < RL; r++) h.f[(size_t)(EPF_FIG0 + k) * RL + r] = 0.0;
    for (int m = 0; m < covered; m++) ep_fold(h.e, tail_rows_row(h.e.rows, listed, (size_t)m));
    for (Rec& r : want)
        if (r.i[EPL_COUNTED])
            for (int k = 0; k < 8; k++) r.f[EPL_FIG0 + k] = h.f[(size_t)(EPF_FIG0 + k) * RL + r.i[EPL_ROBOT]];
    CHECK(h.n_written[0] == n0 + want.size());
    const size_t C = (size_t)capacity, first_kept = want.size() > C ? want.size() - C : 0;
    std::vector<char> touched(C, 0);
    size_t bad = 0;
    for (size_t q = first_kept; q < want.size(); q++) {
        const size_t s = (size_t)((n0 + q) % C);
        touched[s] = 1;
        for (int k = 0; k < EPL_I32_ROWS; k++) bad += h.ring_i[(size_t)k * C + s] != want[q].i[k];
        for (int k = 0; k < EPL_F64_ROWS; k++) bad += !(h.ring_f[(size_t)k * C + s] == want[q].f[k]);  // (by value: 0.0 + -0.0 is +0.0 in the sum)
        bad += h.ring_p[s] != want[q].placement;
    }
    CHECK(bad == 0);
    size_t stray = 0;  // slots no record of this chain belongs in keep what they held
    for (size_t s = 0; s < C; s++)
        if (!touched[s])
            for (int k = 0; k < EPL_I32_ROWS; k++) stray += h.ring_i[(size_t)k * C + s] != ring_i0[(size_t)k * C + s];
    CHECK(stray == 0);
    CHECK(h.tags == want_tags);
    CHECK(h.tag_place == want_place);
    // every covered row has an episode open now, the others are as they were
    size_t opened = 0;
    for (int m = 0; m < covered; m++) opened += h.i[(size_t)EPI_OPEN * RL + tail_rows_row(h.e.rows, listed, (size_t)m)] == 1;
    CHECK(opened == (size_t)covered);
}

int main() {
    unsigned seed = 1;
    for (int covered : {1, 63, 65, 1024, 1025, 2500})
        for (int capacity : {1, 7, 4096}) {
            run_case(covered, covered, false, false, capacity, seed++);  // imgenv_reset: every local robot of one world
            run_case(covered, 1, true, false, capacity, seed++);         // a listed chain, the count on the host
            run_case(covered, 1, true, true, capacity, seed++);          // ... and in device memory
            if (covered % 5 == 0) run_case(covered, 5, true, true, capacity, seed++);
        }
    {   // without banks and before the first device-side reset: map 0, tracks -1, scenario -1, placement ~0; a robot shard: world 0
        Handle h(6, 12, 4, 0);  // 6 local robots of a world of 12
        h.W = h.g.W = 1;
        h.g.map_cur = nullptr; h.g.trk_cur = nullptr; h.g.scn_world = nullptr; h.g.scn_mark = nullptr; h.g.place_serial = nullptr;
        chunked_append(h.e, h.g);  // the first reset: nothing open
        CHECK(h.n_written[0] == 0);
        for (int r = 0; r < 6; r++) ep_fold(h.e, (size_t)r);
        for (int r = 0; r < 6; r++) ep_accumulate(h.e, (size_t)r);
        chunked_append(h.e, h.g);
        CHECK(h.n_written[0] == 6);
        for (int q = 2; q < 6; q++) {  // capacity 4: records 2 .. 5 survive
            const size_t s = (size_t)q % 4;
            CHECK(h.ring_i[EPL_ROBOT * 4 + s] == q && h.ring_i[EPL_WORLD * 4 + s] == 0 && h.ring_i[EPL_MAP * 4 + s] == 0);
            CHECK(h.ring_i[EPL_TRACKS * 4 + s] == -1 && h.ring_i[EPL_SCENARIO * 4 + s] == -1 && h.ring_p[s] == ~0ull);
            CHECK(h.ring_i[EPL_STEPS * 4 + s] == 1 && h.ring_i[EPL_COUNTED * 4 + s] == 1 && h.ring_i[EPL_EPISODE * 4 + s] == 1);
        }
        // a scenario bank but no pool yet: mark ~0 == "serial" ~0, the host's scenario stands
        std::vector<int> scn(1, 3);
        std::vector<unsigned long long> mark(1, ~0ull);
        h.g.scn_world = scn.data(); h.g.scn_mark = mark.data();
        eplog_retag(h.e, h.g, 2);
        CHECK(h.tags[EPT_SCENARIO * 6 + 2] == 3);
    }
    if (g_fail) {
        printf("%d of %d checks failed\n", g_fail, g_checks);
        return 1;
    }
    printf("OK %d checks\n", g_checks);
    return 0;
}
