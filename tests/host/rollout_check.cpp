// rollout_check.cpp -- k_rollout and k_rollout_gae (img_env_amd/csrc/rollout.h) on the CPU: the header's item function, its count
// and the advantage pass's row function run over a simulated grid of blocks x lanes, on a case that tests/test_rollout_plan.py
// writes and whose result it compares with tests/rollout_model.py.
//   g++ -std=c++17 -ffp-contract=off tests/host/rollout_check.cpp -o check && ./check plan && ./check run case.bin result.bin
// (also built with -fsanitize=address,undefined: every array is an allocation of its own, so every access of the walk is bounds-checked)
//
// case.bin, little-endian: int32 RL, Rw, T, F, n_fields, n_chains; int32 row_bytes[n_fields]; the first observation (per field
// RL x row bytes); per chain int32 kind (0 step, 1 reset), then
//   step:  float actions[RL][3], double rewards[RL], uint8 dones[RL], uint8 is_clean[RL], int32 dones_info[RL]
//   reset: int32 mode (0: every local row, 1: listed, the host's count, 2: listed, the count in "device" memory), int32 n_listed,
//          int32 worlds[n_listed]
//   both:  int32 blocks (0: the planner's grid), the live arrays after the chain (per field RL x row bytes)
// then float gamma, lam, int32 has_final_values, float values[T+1][RL], final_values[F], adv[T][RL], ret[T][RL] (what adv / ret hold before).
// result.bin: per field the ring and the final array; actions, rewards, dones, is_clean, dones_info, final_idx, final_slot,
// final_row, final_n[2], adv, ret.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../img_env_amd/csrc/rollout.h"

static int g_fail = 0, g_checks = 0;
#define CHECK_EQ(a, b)                                                                                 \
    do {                                                                                               \
        g_checks++;                                                                                    \
        const long long a_ = (long long)(a), b_ = (long long)(b);                                      \
        if (a_ != b_) {                                                                                \
            g_fail++;                                                                                  \
            printf("FAIL %s:%d: %s = %lld, expected %s = %lld\n", __FILE__, __LINE__, #a, a_, #b, b_); \
        }                                                                                              \
    } while (0)

static unsigned char* room(size_t bytes) {  // 256-byte aligned and zeroed, like the library's carve-outs
    const size_t n = (bytes + 255) & ~(size_t)255;
    unsigned char* p = (unsigned char*)aligned_alloc(256, n ? n : 256);
    memset(p, 0, n ? n : 256);
    return p;
}
template <typename T>
static T* room_of(size_t count) { return (T*)room(sizeof(T) * count); }

static void get(FILE* f, void* p, size_t bytes) {
    if (bytes && fread(p, 1, bytes, f) != bytes) {
        printf("FAIL: the case file ends early\n");
        exit(2);
    }
}
static int get_i32(FILE* f) {
    int32_t v = 0;
    get(f, &v, 4);
    return v;
}

// one launch over `blocks` x ROLLOUT_BLOCK lanes, as the kernel walks it
template <bool RESTART>
static void launch(const RolloutDev& ro, unsigned blocks) {
    const bool listed = RESTART && ro.rows.list != nullptr;
    const size_t covered = tail_rows_count(ro.rows, listed);
    const uint32_t base = RESTART ? ro.final_n[ro.turn & 1] : 0u;
    const size_t total = covered * ro.chunks_per_row, stride = (size_t)blocks * ROLLOUT_BLOCK;
    for (unsigned b = 0; b < blocks; b++)
        for (unsigned lane = 0; lane < ROLLOUT_BLOCK; lane++) {
            for (size_t t = (size_t)b * ROLLOUT_BLOCK + lane; t < total; t += stride) rollout_item<RESTART>(ro, listed, base, t);
            if (RESTART && b == 0 && lane == 0) rollout_count(ro, base, covered);
        }
}

static int plan_checks() {
    // the launch shapes: rows x chunks in blocks of ROLLOUT_BLOCK; the cap is reached from ROLLOUT_BLOCK x ROLLOUT_MAX_BLOCKS chunks on
    PlanHandle h;
    h.RL = 6; h.Rw = 2; h.W = 3;
    PlanChain c;
    const uint32_t cpr = 1000;
    CHECK_EQ(plan_rollout_launch(h, c, cpr).grid, (6 * (size_t)cpr + ROLLOUT_BLOCK - 1) / ROLLOUT_BLOCK);
    CHECK_EQ(plan_rollout_launch(h, c, cpr).block, ROLLOUT_BLOCK);
    CHECK_EQ(plan_rollout_launch(h, c, cpr).lds, 0);
    c.is_reset = true; c.listed = true; c.act_nw = 2;
    CHECK_EQ(plan_rollout_launch(h, c, cpr).grid, (4 * (size_t)cpr + ROLLOUT_BLOCK - 1) / ROLLOUT_BLOCK);  // listed: Rw rows per world
    c.n_dev = true; c.act_nw = 3; c.act_hint = 2;  // the device's count: the hint, at least one world, at most every world
    CHECK_EQ(plan_rollout_launch(h, c, cpr).grid, (2 * (size_t)cpr + ROLLOUT_BLOCK - 1) / ROLLOUT_BLOCK);
    CHECK_EQ(plan_rollout_begin_launch(h, cpr).grid, (6 * (size_t)cpr + ROLLOUT_BLOCK - 1) / ROLLOUT_BLOCK);  // every local row
    PlanChain s;
    h.RL = 1024; h.Rw = 4; h.W = 256;
    CHECK_EQ(plan_rollout_launch(h, s, 256).grid, ROLLOUT_MAX_BLOCKS);      // 1024 rows x 256 chunks: exactly the cap, no stride yet
    CHECK_EQ(plan_rollout_launch(h, s, 255).grid, ROLLOUT_MAX_BLOCKS - 4);  // (1024 x 255 / 256 = 1020)
    CHECK_EQ(plan_rollout_launch(h, s, 257).grid, ROLLOUT_MAX_BLOCKS);      // beyond: the blocks stride
    CHECK_EQ(plan_rollout_launch(h, s, 100000).grid, ROLLOUT_MAX_BLOCKS);
    h.RL = 1200;
    CHECK_EQ(plan_rollout_gae_launch(h).grid, (1200 + GAE_BLOCK - 1) / GAE_BLOCK);
    CHECK_EQ(plan_rollout_gae_launch(h).block, GAE_BLOCK);
    h.RL = GAE_BLOCK * GAE_MAX_BLOCKS + 1;
    CHECK_EQ(plan_rollout_gae_launch(h).grid, GAE_MAX_BLOCKS);
    CHECK_EQ(plan_final_field(4608).unit, 16);
    CHECK_EQ(plan_final_field(1448).unit, 8);
    CHECK_EQ(plan_final_field(20).unit, 4);
    CHECK_EQ(plan_final_field(6).unit, 2);
    CHECK_EQ(plan_final_field(3).unit, 1);
    if (g_fail) {
        printf("%d of %d checks failed\n", g_fail, g_checks);
        return 1;
    }
    printf("OK %d checks ROLLOUT_BLOCK %d ROLLOUT_MAX_BLOCKS %d ROLLOUT_MAX_FIELDS %d GAE_BLOCK %d GAE_MAX_BLOCKS %d GAE_BATCH %d\n", g_checks,
           ROLLOUT_BLOCK, ROLLOUT_MAX_BLOCKS, ROLLOUT_MAX_FIELDS, GAE_BLOCK, GAE_MAX_BLOCKS, GAE_BATCH);
    return 0;
}

static int run(const char* in_path, const char* out_path) {
    FILE* f = fopen(in_path, "rb");
    if (!f) return printf("FAIL: cannot open %s\n", in_path), 2;
    const int RL = get_i32(f), Rw = get_i32(f), T = get_i32(f), F = get_i32(f), n_fields = get_i32(f), n_chains = get_i32(f);
    if (n_fields < 1 || n_fields > ROLLOUT_MAX_FIELDS || RL < 1 || Rw < 1 || RL % Rw || T < 1 || F < 1) return printf("FAIL: bad header\n"), 2;
    const size_t R = (size_t)RL;
    std::vector<size_t> row_bytes((size_t)n_fields);
    std::vector<unsigned char*> live((size_t)n_fields);
    RolloutDev ro;
    memset(&ro, 0, sizeof(ro));
    ro.n_fields = n_fields;
    for (int k = 0; k < n_fields; k++) {
        row_bytes[(size_t)k] = (size_t)get_i32(f);
        const FinalFieldPlan p = plan_final_field(row_bytes[(size_t)k]);
        live[(size_t)k] = room(R * row_bytes[(size_t)k]);
        ro.f[k] = {room((size_t)(T + 1) * R * row_bytes[(size_t)k]), room((size_t)F * row_bytes[(size_t)k]), live[(size_t)k], p.unit, p.chunks};
        ro.chunks_per_row += p.chunks;
    }
    float* act_src = room_of<float>(R * 3);
    double* rew_src = room_of<double>(R);
    uint8_t* done_src = room_of<uint8_t>(R);
    uint8_t* clean_src = room_of<uint8_t>(R);
    int32_t* info_src = room_of<int32_t>(R);
    ro.act_src = act_src; ro.rew_src = rew_src; ro.done_src = done_src; ro.clean_src = clean_src; ro.info_src = info_src;
    ro.actions = room_of<float>((size_t)T * R * 3);
    ro.rewards = room_of<float>((size_t)T * R);
    ro.dones = room_of<uint8_t>((size_t)T * R);
    ro.is_clean = room_of<uint8_t>((size_t)T * R);
    ro.dones_info = room_of<int32_t>((size_t)T * R);
    ro.final_idx = room_of<int32_t>((size_t)(T + 1) * R);
    ro.final_slot = room_of<int32_t>((size_t)F);
    ro.final_row = room_of<int32_t>((size_t)F);
    ro.final_n = room_of<uint32_t>(2);
    ro.F = F;
    PlanHandle ph;
    ph.RL = RL; ph.Rw = Rw; ph.W = RL / Rw;
    const TailRows every = {RL, Rw, nullptr, nullptr, RL / Rw};
    // imgenv_rollout_begin, the first time: the live arrays into slot 0 (the step instantiation, scalars off), final_idx -1
    for (int k = 0; k < n_fields; k++) get(f, live[(size_t)k], R * row_bytes[(size_t)k]);
    {
        RolloutDev b = ro;
        b.rewards = nullptr;
        b.n = -1;
        b.rows = every;
        launch<false>(b, plan_rollout_begin_launch(ph, ro.chunks_per_row).grid);
        memset(ro.final_idx, 0xFF, sizeof(int32_t) * (size_t)(T + 1) * R);
    }
    int n = 0;
    uint32_t turn = 0;
    for (int q = 0; q < n_chains; q++) {
        const int kind = get_i32(f);
        RolloutDev c = ro;
        c.n = n;
        c.turn = turn;
        PlanChain pc;
        std::vector<int> list;
        int n_dev = 0;
        if (kind == 0) {
            if (n >= T) return printf("FAIL: the case steps a full ring\n"), 2;
            get(f, act_src, sizeof(float) * R * 3);
            get(f, rew_src, sizeof(double) * R);
            get(f, done_src, R);
            get(f, clean_src, R);
            get(f, info_src, sizeof(int32_t) * R);
            c.rows = every;
        } else {
            const int mode = get_i32(f), n_listed = get_i32(f);
            list.resize((size_t)(RL / Rw) + 1, 0);  // (room for every world, as the library's list has; the entries behind the count are not looked at)
            for (int i = 0; i < n_listed; i++) list[(size_t)i] = get_i32(f);
            n_dev = n_listed;
            pc.is_reset = true;
            pc.listed = mode != 0;
            pc.n_dev = mode == 2;
            pc.act_nw = mode == 2 ? RL / Rw : n_listed;
            pc.act_hint = Rw;  // (a stale guess of one world: more than that strides)
            c.rows = {RL, Rw, mode ? list.data() : nullptr, mode == 2 ? &n_dev : nullptr, mode == 2 ? RL / Rw : n_listed};
        }
        const int blocks = get_i32(f);
        for (int k = 0; k < n_fields; k++) get(f, live[(size_t)k], R * row_bytes[(size_t)k]);
        const unsigned grid = blocks > 0 ? (unsigned)blocks : plan_rollout_launch(ph, pc, ro.chunks_per_row).grid;
        if (kind == 0) {
            launch<false>(c, grid);
            n++;
        } else {
            launch<true>(c, grid);
            turn++;
        }
    }
    // the advantage pass over a grid of GAE_BLOCK lanes
    float gamma = 0, lam = 0;
    get(f, &gamma, 4);
    get(f, &lam, 4);
    const int has_fv = get_i32(f);
    float* values = room_of<float>((size_t)(T + 1) * R);
    float* fv = room_of<float>((size_t)F);
    float* adv = room_of<float>((size_t)T * R);
    float* ret = room_of<float>((size_t)T * R);
    get(f, values, sizeof(float) * (size_t)(T + 1) * R);
    get(f, fv, sizeof(float) * (size_t)F);
    get(f, adv, sizeof(float) * (size_t)T * R);
    get(f, ret, sizeof(float) * (size_t)T * R);
    fclose(f);
    const RolloutGaeDev g = {ro.rewards, ro.dones, ro.is_clean, ro.dones_info, ro.final_idx, values, has_fv ? fv : nullptr, adv, ret, gamma, lam, n, F, RL};
    {
        const unsigned blocks = 2;  // (several strides)
        const size_t stride = (size_t)blocks * GAE_BLOCK;
        for (unsigned b = 0; b < blocks; b++)
            for (unsigned lane = 0; lane < GAE_BLOCK; lane++)
                for (size_t row = (size_t)b * GAE_BLOCK + lane; row < R; row += stride) rollout_gae_row(g, row);
    }
    FILE* o = fopen(out_path, "wb");
    if (!o) return printf("FAIL: cannot write %s\n", out_path), 2;
    for (int k = 0; k < n_fields; k++) {
        fwrite(ro.f[k].ring, 1, (size_t)(T + 1) * R * row_bytes[(size_t)k], o);
        fwrite(ro.f[k].fin, 1, (size_t)F * row_bytes[(size_t)k], o);
    }
    fwrite(ro.actions, 4, (size_t)T * R * 3, o);
    fwrite(ro.rewards, 4, (size_t)T * R, o);
    fwrite(ro.dones, 1, (size_t)T * R, o);
    fwrite(ro.is_clean, 1, (size_t)T * R, o);
    fwrite(ro.dones_info, 4, (size_t)T * R, o);
    fwrite(ro.final_idx, 4, (size_t)(T + 1) * R, o);
    fwrite(ro.final_slot, 4, (size_t)F, o);
    fwrite(ro.final_row, 4, (size_t)F, o);
    fwrite(ro.final_n, 4, 2, o);
    fwrite(adv, 4, (size_t)T * R, o);
    fwrite(ret, 4, (size_t)T * R, o);
    fclose(o);
    for (int k = 0; k < n_fields; k++) {
        free(ro.f[k].ring);
        free(ro.f[k].fin);
        free(live[(size_t)k]);
    }
    void* rest[] = {act_src, rew_src, done_src, clean_src, info_src, ro.actions, ro.rewards, ro.dones, ro.is_clean, ro.dones_info,
                    ro.final_idx, ro.final_slot, ro.final_row, ro.final_n, values, fv, adv, ret};
    for (void* p : rest) free(p);
    printf("OK n %d resets %u\n", n, turn);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "plan")) return plan_checks();
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    printf("usage: %s plan | run case.bin result.bin\n", argv[0]);
    return 2;
}
