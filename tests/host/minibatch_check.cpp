// minibatch_check.cpp -- the minibatch kernels (img_env_amd/csrc/minibatch.h) on the CPU: the header's flag, scatter, shuffle,
// statistics and gather functions run over a simulated grid of blocks x lanes, on a case that tests/test_minibatch_plan.py writes
// and whose result it compares with tests/minibatch_model.py.  What crosses lanes on the device -- the exclusive prefix of the
// lanes' popcounts, the scan's carry, the fold of the partial sums -- is done here lane by lane in the same order.
//   g++ -std=c++17 -ffp-contract=off tests/host/minibatch_check.cpp -o check && ./check plan && ./check run case.bin result.bin
// (also built with -fsanitize=address,undefined: every array is an allocation of its own, so every access of the walk is bounds-checked)
//
// case.bin, little-endian: int32 TR (T x R), total (n x R), ring_rows (>= TR: the rows of an obs array and of a caller's scalar), B,
// j, n_fields, n_scalars, normalise, gather_blocks (0: the planner's grid); uint32 seed_lo, seed_hi; float norm[2]; double eps;
// int32 row_bytes[n_fields]; uint8 is_clean[TR]; per field ring_rows x row bytes; float actions[TR][3], rewards[TR]; uint8
// dones[TR]; int32 dones_info[TR]; float x[TR]; per scalar float [ring_rows].
// result.bin: int32 valid_n; int32 valid[TR], order[TR]; float stats[2], the same of a second run; per field B x row bytes; float
// mb_actions[B][3], mb_rewards[B]; uint8 mb_dones[B]; int32 mb_dones_info[B], mb_index[B]; float mb_weight[B], mb_scalars[6][B].
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../img_env_amd/csrc/minibatch.h"

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

static unsigned char* room(size_t bytes) {  // 256-byte aligned and zeroed, like the library's carve-outs, but of the exact size
    void* p = nullptr;
    if (posix_memalign(&p, 256, bytes ? bytes : 1)) exit(2);
    memset(p, 0, bytes ? bytes : 1);
    return (unsigned char*)p;
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

// ---- the index: k_mb_count, k_mb_scan, k_mb_scatter
static void index_launches(const MbIndexDev& d) {
    const unsigned grid = plan_mb_index_launch(d.total).grid;
    for (unsigned tile = 0; tile < grid; tile++) {
        int total = 0;
        for (unsigned lane = 0; lane < MB_INDEX_BLOCK; lane++) total += __builtin_popcount(mb_lane_flags(d, tile, lane));
        if (tile < d.n_tiles) d.tile_count[tile] = total;
    }
    uint32_t carry = 0;
    for (uint32_t base = 0; base < d.n_tiles; base += MB_SCAN_BLOCK) {  // one round of the one workgroup
        uint32_t before = 0;
        for (uint32_t lane = 0; lane < MB_SCAN_BLOCK; lane++) {
            const uint32_t i = base + lane;
            if (i < d.n_tiles) d.tile_base[i] = (int32_t)(carry + before);
            before += i < d.n_tiles ? (uint32_t)d.tile_count[i] : 0u;
        }
        carry += before;
    }
    *d.valid_n = carry;
    for (unsigned tile = 0; tile < grid; tile++) {
        int before = 0;
        for (unsigned lane = 0; lane < MB_INDEX_BLOCK; lane++) {
            const uint32_t mask = mb_lane_flags(d, tile, lane);
            if (tile < d.n_tiles) mb_scatter16(d.valid, (size_t)d.tile_base[tile] + (size_t)before, mask, (size_t)tile * MB_TILE + (size_t)lane * MB_LANE_FLAGS);
            before += __builtin_popcount(mask);
        }
    }
}

// ---- the statistics: k_mb_stats<false>, k_mb_stats_final<false>, k_mb_stats<true>, k_mb_stats_final<true>
static void stats_launches(const MbStatsDev& s, size_t total) {
    const unsigned grid = plan_mb_stats_launch(total).grid;
    double a[MB_STATS_BLOCK];
    for (int second = 0; second < 2; second++) {
        const uint32_t V = *s.valid_n;
        for (unsigned tile = 0; tile < grid; tile++) {
            for (unsigned lane = 0; lane < MB_STATS_BLOCK; lane++) a[lane] = mb_stats_lane(s, V, second != 0, second ? s.mean[0] : 0.0, tile, lane);
            const double sum = mb_fold(a);
            if (tile < s.n_tiles) s.part[tile] = sum;
        }
        for (unsigned lane = 0; lane < MB_STATS_BLOCK; lane++) a[lane] = mb_stats_final_lane(s, lane);
        const double sum = mb_fold(a);
        if (second)
            mb_stats_norm(s, V, sum);
        else
            mb_stats_mean(s, V, sum);
    }
}

static int plan_checks() {
    CHECK_EQ(MB_TILE, MB_INDEX_BLOCK * MB_LANE_FLAGS);
    CHECK_EQ(MB_LANE_FLAGS, 16);  // one 16-byte load per lane
    CHECK_EQ(MB_MAX_SCALARS, 6);
    CHECK_EQ(plan_mb_tiles(1), 1);
    CHECK_EQ(plan_mb_tiles(MB_TILE), 1);
    CHECK_EQ(plan_mb_tiles(MB_TILE + 1), 2);
    CHECK_EQ(plan_mb_index_launch(MB_TILE + 1).grid, 2);
    CHECK_EQ(plan_mb_index_launch(90).block, MB_INDEX_BLOCK);
    CHECK_EQ(plan_mb_index_launch((size_t)1 << 31).grid, ((size_t)1 << 31) / MB_TILE);  // no cap: the scan's carry takes any count
    CHECK_EQ(plan_mb_scan_launch().grid, 1);
    CHECK_EQ(plan_mb_scan_launch().block, MB_SCAN_BLOCK);
    CHECK_EQ(plan_mb_stats_launch(MB_STATS_TILE * 3 + 1).grid, 4);
    CHECK_EQ(plan_mb_stats_final_launch().grid, 1);
    CHECK_EQ(plan_mb_shuffle_launch(90).grid, 1);
    CHECK_EQ(plan_mb_shuffle_launch(4800).grid, (4800 + MB_SHUFFLE_BLOCK - 1) / MB_SHUFFLE_BLOCK);
    CHECK_EQ(plan_mb_gather_launch(32, 100).grid, (3200 + ROLLOUT_BLOCK - 1) / ROLLOUT_BLOCK);
    CHECK_EQ(plan_mb_gather_launch(256, 1024).grid, ROLLOUT_MAX_BLOCKS);  // exactly the cap, no stride yet
    CHECK_EQ(plan_mb_gather_launch(256, 1728).grid, ROLLOUT_MAX_BLOCKS);  // ped_maps at B = 256: the blocks stride
    CHECK_EQ(plan_mb_gather_launch(256, 1728).lds, 0);
    // pi for small V under seed 0x0123456789ABCDEF (tests/test_minibatch_model.py derives these by hand)
    const MbKeys key = mb_keys(0x89ABCDEFu, 0x01234567u);
    CHECK_EQ(key.k[0], 0x4C843A19u);
    CHECK_EQ(key.k[5], 0x106103B5u);
    const int want5[5] = {1, 3, 4, 2, 0}, want3[3] = {2, 1, 0};
    for (uint32_t x = 0; x < 5; x++) CHECK_EQ(mb_perm(key, 5, x), want5[x]);
    for (uint32_t x = 0; x < 3; x++) CHECK_EQ(mb_perm(key, 3, x), want3[x]);
    CHECK_EQ(mb_perm(key, 2, 0), 0);
    CHECK_EQ(mb_perm(key, 2, 1), 1);
    CHECK_EQ(mb_perm(key, 1, 0), 0);
    if (g_fail) {
        printf("%d of %d checks failed\n", g_fail, g_checks);
        return 1;
    }
    printf("OK %d checks MB_INDEX_BLOCK %d MB_LANE_FLAGS %d MB_TILE %d MB_SCAN_BLOCK %d MB_STATS_BLOCK %d MB_STATS_PER_LANE %d MB_SHUFFLE_BLOCK %d MB_ROUNDS %d MB_MAX_SCALARS %d\n",
           g_checks, MB_INDEX_BLOCK, MB_LANE_FLAGS, MB_TILE, MB_SCAN_BLOCK, MB_STATS_BLOCK, MB_STATS_PER_LANE, MB_SHUFFLE_BLOCK, MB_ROUNDS, MB_MAX_SCALARS);
    return 0;
}

static int run(const char* in_path, const char* out_path) {
    FILE* f = fopen(in_path, "rb");
    if (!f) return printf("FAIL: cannot open %s\n", in_path), 2;
    const int TR = get_i32(f), total = get_i32(f), ring_rows = get_i32(f), B = get_i32(f), j = get_i32(f), n_fields = get_i32(f);
    const int n_scalars = get_i32(f), normalise = get_i32(f), gather_blocks = get_i32(f);
    if (TR < 1 || total < 1 || total > TR || ring_rows < TR || B < 1 || j < 0 || n_fields < 1 || n_fields > ROLLOUT_MAX_FIELDS || n_scalars < 0 ||
        n_scalars > MB_MAX_SCALARS || normalise < -1 || normalise >= n_scalars)
        return printf("FAIL: bad header\n"), 2;
    uint32_t seed[2];
    get(f, seed, 8);
    float* norm = room_of<float>(2);
    get(f, norm, 8);
    double eps = 0;
    get(f, &eps, 8);
    std::vector<size_t> row_bytes((size_t)n_fields);
    for (int k = 0; k < n_fields; k++) row_bytes[(size_t)k] = (size_t)get_i32(f);
    std::vector<void*> mine;
    auto keep = [&](auto* p) {
        mine.push_back((void*)p);
        return p;
    };
    keep(norm);
    uint8_t* clean = keep(room_of<uint8_t>((size_t)total));  // (exactly n R flags: a read past the end is a finding)
    {
        std::vector<uint8_t> all((size_t)TR);
        get(f, all.data(), (size_t)TR);
        memcpy(clean, all.data(), (size_t)total);
    }
    MbGatherDev g;
    memset(&g, 0, sizeof(g));
    g.n_fields = n_fields;
    for (int k = 0; k < n_fields; k++) {
        const FinalFieldPlan p = plan_final_field(row_bytes[(size_t)k]);
        unsigned char* ring = keep(room((size_t)ring_rows * row_bytes[(size_t)k]));
        get(f, ring, (size_t)ring_rows * row_bytes[(size_t)k]);
        g.f[k] = {ring, keep(room((size_t)B * row_bytes[(size_t)k])), p.unit, p.chunks};
        memset(g.f[k].dst, 0xAB, (size_t)B * row_bytes[(size_t)k]);  // (the gather defines every byte)
        g.chunks_per_row += p.chunks;
    }
    float* actions = keep(room_of<float>((size_t)TR * 3));
    float* rewards = keep(room_of<float>((size_t)TR));
    uint8_t* dones = keep(room_of<uint8_t>((size_t)TR));
    int32_t* info = keep(room_of<int32_t>((size_t)TR));
    float* x = keep(room_of<float>((size_t)TR));
    get(f, actions, sizeof(float) * (size_t)TR * 3);
    get(f, rewards, sizeof(float) * (size_t)TR);
    get(f, dones, (size_t)TR);
    get(f, info, sizeof(int32_t) * (size_t)TR);
    get(f, x, sizeof(float) * (size_t)TR);
    for (int s = 0; s < n_scalars; s++) {
        float* a = keep(room_of<float>((size_t)ring_rows));
        get(f, a, sizeof(float) * (size_t)ring_rows);
        g.scalars[s] = a;
    }
    fclose(f);

    const size_t tiles = plan_mb_tiles((size_t)TR);
    int32_t* valid = keep(room_of<int32_t>((size_t)TR));
    int32_t* order = keep(room_of<int32_t>((size_t)TR));
    uint32_t* valid_n = keep(room_of<uint32_t>(1));
    int32_t* tile_count = keep(room_of<int32_t>(tiles));
    int32_t* tile_base = keep(room_of<int32_t>(tiles));
    double* part = keep(room_of<double>(plan_mb_stats_tiles((size_t)TR)));
    double* mean = keep(room_of<double>(1));
    float* stats = keep(room_of<float>(4));

    const MbIndexDev d = {clean, valid, tile_count, tile_base, valid_n, (uint32_t)total, (uint32_t)plan_mb_tiles((size_t)total)};
    index_launches(d);

    for (int again = 0; again < 2; again++) {
        const MbStatsDev s = {x, valid, valid_n, part, mean, stats + 2 * again, eps, (uint32_t)plan_mb_stats_tiles((size_t)total)};
        stats_launches(s, (size_t)total);
    }

    const MbShuffleDev sh = {valid, valid_n, order, (uint32_t)TR, mb_keys(seed[0], seed[1])};
    {
        const unsigned grid = plan_mb_shuffle_launch((size_t)TR).grid;
        for (unsigned b = 0; b < grid; b++)
            for (unsigned lane = 0; lane < MB_SHUFFLE_BLOCK; lane++) {
                const size_t p = (size_t)b * MB_SHUFFLE_BLOCK + lane;
                if (p < (size_t)sh.TR) mb_shuffle_item(sh, *sh.valid_n, (uint32_t)p);
            }
    }

    g.order = order;
    g.first = (size_t)j * (size_t)B;
    g.B = (uint32_t)B;
    g.TR = (uint32_t)TR;
    g.actions = actions; g.rewards = rewards; g.dones = dones; g.dones_info = info;
    g.mb_actions = keep(room_of<float>((size_t)B * 3));
    g.mb_rewards = keep(room_of<float>((size_t)B));
    g.mb_dones = keep(room_of<uint8_t>((size_t)B));
    g.mb_dones_info = keep(room_of<int32_t>((size_t)B));
    g.mb_index = keep(room_of<int32_t>((size_t)B));
    g.mb_weight = keep(room_of<float>((size_t)B));
    g.mb_scalars = keep(room_of<float>((size_t)B * MB_MAX_SCALARS));
    g.n_scalars = n_scalars;
    g.normalise = normalise;
    g.norm = norm;
    const unsigned blocks = gather_blocks > 0 ? (unsigned)gather_blocks : plan_mb_gather_launch((size_t)B, g.chunks_per_row).grid;
    {
        const size_t items = (size_t)g.B * g.chunks_per_row, stride = (size_t)blocks * ROLLOUT_BLOCK;
        for (unsigned b = 0; b < blocks; b++)
            for (unsigned lane = 0; lane < ROLLOUT_BLOCK; lane++)
                for (size_t t = (size_t)b * ROLLOUT_BLOCK + lane; t < items; t += stride) mb_gather_item(g, t);
    }

    FILE* o = fopen(out_path, "wb");
    if (!o) return printf("FAIL: cannot write %s\n", out_path), 2;
    fwrite(valid_n, 4, 1, o);
    fwrite(valid, 4, (size_t)TR, o);
    fwrite(order, 4, (size_t)TR, o);
    fwrite(stats, 4, 4, o);
    for (int k = 0; k < n_fields; k++) fwrite(g.f[k].dst, 1, (size_t)B * row_bytes[(size_t)k], o);
    fwrite(g.mb_actions, 4, (size_t)B * 3, o);
    fwrite(g.mb_rewards, 4, (size_t)B, o);
    fwrite(g.mb_dones, 1, (size_t)B, o);
    fwrite(g.mb_dones_info, 4, (size_t)B, o);
    fwrite(g.mb_index, 4, (size_t)B, o);
    fwrite(g.mb_weight, 4, (size_t)B, o);
    fwrite(g.mb_scalars, 4, (size_t)B * MB_MAX_SCALARS, o);
    fclose(o);
    const unsigned n_valid = *valid_n, n_tiles = d.n_tiles;
    for (void* p : mine) free(p);
    printf("OK valid_n %u tiles %u gather_blocks %u\n", n_valid, n_tiles, blocks);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "plan")) return plan_checks();
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    printf("usage: %s plan | run case.bin result.bin\n", argv[0]);
    return 2;
}
