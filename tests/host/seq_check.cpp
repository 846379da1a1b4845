// seq_check.cpp -- the sequence minibatches (img_env_amd/csrc/sequences.h) on the CPU: the header's flag and gather functions and
// the minibatches' compaction and shuffle run over a simulated grid of blocks x lanes, on a case that tests/test_seq_plan.py writes
// and whose result it compares with tests/seq_model.py; and the refusals of seq_enable_plan (feature_plan.h) and the block's layout.
//   g++ -std=c++17 -ffp-contract=off tests/host/seq_check.cpp -o check && ./check plan && ./check run case.bin result.bin
// (also built with -fsanitize=address,undefined: every array is an allocation of its own -- is_clean of exactly n R bytes, seq_flag
// of exactly C R -- so every access of the walk is bounds-checked)
//
// case.bin, little-endian: int32 R, T, n, L, Bs, j, n_fields, n_scalars, normalise, gather_blocks (0: the planner's grid),
// state_bytes[2]; uint32 seed_lo, seed_hi; float norm[2]; int32 row_bytes[n_fields]; uint8 is_clean[T R]; int32 final_idx[(T+1) R];
// per field (T+1) R x row bytes; float actions[T R][3], rewards[T R]; uint8 dones[T R]; int32 dones_info[T R]; per scalar float
// [(T+1) R]; per state (T+1) R x state bytes.
// result.bin: int32 valid_n; uint8 flag[C R]; int32 valid[S], order[S] (S = C_max R); per field L Bs x row bytes; float
// mb_actions[L Bs][3], mb_rewards[L Bs]; uint8 mb_dones[L Bs]; int32 mb_dones_info[L Bs], mb_index[L Bs]; float mb_weight[L Bs];
// uint8 mb_first[L Bs]; float mb_scalars[6][L Bs]; int32 mb_seq[Bs], mb_seq_len[Bs]; per state Bs x state bytes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../img_env_amd/csrc/feature_plan.h"
#include "../../img_env_amd/csrc/sequences.h"

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
#define REFUSED(expr, code, word)                                                                         \
    do {                                                                                                  \
        msg[0] = 0;                                                                                       \
        CHECK_EQ((expr), (code));                                                                         \
        g_checks++;                                                                                       \
        if (!strstr(msg, word)) {                                                                         \
            g_fail++;                                                                                     \
            printf("FAIL %s:%d: \"%s\" lacks \"%s\"\n", __FILE__, __LINE__, msg, word);                   \
        }                                                                                                 \
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

// k_mb_count, k_mb_scan, k_mb_scatter as tests/host/minibatch_check.cpp walks them
static void index_launches(const MbIndexDev& d) {
    const unsigned grid = plan_mb_index_launch(d.total).grid;
    for (unsigned tile = 0; tile < grid; tile++) {
        int total = 0;
        for (unsigned lane = 0; lane < MB_INDEX_BLOCK; lane++) total += __builtin_popcount(mb_lane_flags(d, tile, lane));
        if (tile < d.n_tiles) d.tile_count[tile] = total;
    }
    uint32_t carry = 0;
    for (uint32_t base = 0; base < d.n_tiles; base += MB_SCAN_BLOCK) {
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

static imgenv_seq_cfg good_cfg() {
    imgenv_seq_cfg c = {};
    c.struct_size = (int32_t)sizeof(c);
    c.length = 4;
    c.batch = 8;
    c.buffers = 1;
    c.state_bytes[0] = 32;
    return c;
}

static int plan_checks() {
    CHECK_EQ(SEQ_MAX_STATES, IMGENV_SEQ_MAX_STATES);
    CHECK_EQ(plan_seq_chunks(15, 4), 4);
    CHECK_EQ(plan_seq_chunks(16, 4), 4);
    CHECK_EQ(plan_seq_chunks(1, 4), 1);
    CHECK_EQ(plan_seq_flag_launch(1).grid, 1);
    CHECK_EQ(plan_seq_flag_launch(SEQ_FLAG_BLOCK + 1).grid, 2);
    CHECK_EQ(plan_seq_flag_launch(4800).block, SEQ_FLAG_BLOCK);
    CHECK_EQ(plan_seq_gather_launch(4, 4, 100, 10).grid, (1600 + 40 + ROLLOUT_BLOCK - 1) / ROLLOUT_BLOCK);
    CHECK_EQ(plan_seq_gather_launch(16, 256, 64, 0).grid, ROLLOUT_MAX_BLOCKS);   // exactly the cap
    CHECK_EQ(plan_seq_gather_launch(4, 64, 1728, 0).grid, ROLLOUT_MAX_BLOCKS);   // ped_maps at L = 4, Bs = 64: the blocks stride
    CHECK_EQ(plan_seq_gather_launch(4, 64, 1728, 0).lds, 0);
    {   // the block: every array on a 256-byte boundary, a buffer's arrays side by side, a state of no bytes takes no room
        const size_t rows[2] = {48, 20}, st[2] = {32, 0};
        const SeqLayout l = plan_seq_layout(rows, 2, 6, 15, 4, 4, 2, st);
        CHECK_EQ(l.flag, 0);
        CHECK_EQ(l.valid, 256);               // 24 flags
        CHECK_EQ(l.order, 512);
        CHECK_EQ(l.valid_n, 768);
        CHECK_EQ(l.tile_count, 1024);
        CHECK_EQ(l.tile_base, 1280);
        CHECK_EQ(l.field[0][0], 1536);
        CHECK_EQ(l.field[1][0], 1536 + 768);  // 16 x 48
        CHECK_EQ(l.field[0][1], 1536 + 2 * 768);
        CHECK_EQ(l.field[1][1] - l.field[0][1], 512);  // 16 x 20 = 320 -> 512
        CHECK_EQ(l.scalar[1][SEQ_S_ACTIONS] - l.scalar[0][SEQ_S_ACTIONS], 256);
        CHECK_EQ(l.scalar[1][SEQ_S_SCALARS] - l.scalar[0][SEQ_S_SCALARS], 512);  // 16 x 4 x 6 = 384 -> 512
        CHECK_EQ(l.scalar[1][SEQ_S_STATE0] - l.scalar[0][SEQ_S_STATE0], 256);
        CHECK_EQ(l.scalar[0][SEQ_S_STATE1], l.total);
        CHECK_EQ(l.total % 256, 0);
    }
    // seq_enable_plan: the cfg's own refusals, the null handle, the rollout, the repeated call, the refusals that read the facts
    FeatureMsg msg;
    imgenv_seq_out out = {};
    FeatureFacts f;
    f.RL = 6;
    f.roll_on = true;
    f.roll_horizon = 15;
    f.roll_fields = IMGENV_ROLLOUT_VECTOR_STATES | IMGENV_ROLLOUT_SENSOR_MAPS;
    int want = -1;
    imgenv_seq_cfg c = good_cfg();
    CHECK_EQ(seq_enable_plan(&c, &out, &f, nullptr, &want, msg), IMGENV_OK);
    CHECK_EQ(want, f.roll_fields);
    CHECK_EQ(seq_enable_plan(&c, nullptr, &f, nullptr, &want, msg), IMGENV_OK);
    REFUSED(seq_enable_plan(nullptr, &out, &f, nullptr, &want, msg), IMGENV_EINVAL, "null");
    REFUSED(seq_enable_plan(&c, &out, nullptr, nullptr, &want, msg), IMGENV_EINVAL, "null");
    c.struct_size = 12;
    REFUSED(seq_enable_plan(&c, &out, &f, nullptr, &want, msg), IMGENV_EINVAL, "struct_size");
    c = good_cfg();
    out.struct_size = 4;
    REFUSED(seq_enable_plan(&c, &out, &f, nullptr, &want, msg), IMGENV_EINVAL, "imgenv_seq_out.struct_size");
    out.struct_size = 0;
    for (int length : {0, -1}) {
        c = good_cfg();
        c.length = length;
        REFUSED(seq_enable_plan(&c, &out, nullptr, nullptr, &want, msg), IMGENV_EINVAL, "length");
    }
    c = good_cfg();
    c.length = 16;  // above the horizon: needs the handle's facts
    REFUSED(seq_enable_plan(&c, &out, &f, nullptr, &want, msg), IMGENV_EINVAL, "horizon 15");
    c.length = 15;  // L = T
    CHECK_EQ(seq_enable_plan(&c, &out, &f, nullptr, &want, msg), IMGENV_OK);
    c = good_cfg();
    c.batch = 0;
    REFUSED(seq_enable_plan(&c, &out, nullptr, nullptr, &want, msg), IMGENV_EINVAL, "batch");
    for (int buffers : {0, 5}) {
        c = good_cfg();
        c.buffers = buffers;
        REFUSED(seq_enable_plan(&c, &out, nullptr, nullptr, &want, msg), IMGENV_EINVAL, "buffers");
    }
    for (int bits : {IMGENV_ROLLOUT_ALL + 1, -1, IMGENV_ROLLOUT_NORM_REWARDS}) {
        c = good_cfg();
        c.fields = bits;
        REFUSED(seq_enable_plan(&c, &out, nullptr, nullptr, &want, msg), IMGENV_EINVAL, "fields");
    }
    for (int bytes : {-4, 6, 65540}) {
        c = good_cfg();
        c.state_bytes[1] = bytes;
        REFUSED(seq_enable_plan(&c, &out, nullptr, nullptr, &want, msg), IMGENV_EINVAL, "state_bytes[1]");
    }
    c = good_cfg();
    c.state_bytes[0] = 65536;
    c.state_bytes[1] = 0;
    CHECK_EQ(seq_enable_plan(&c, &out, &f, nullptr, &want, msg), IMGENV_OK);
    c = good_cfg();
    c.reserved = 1;
    REFUSED(seq_enable_plan(&c, &out, nullptr, nullptr, &want, msg), IMGENV_EINVAL, "reserved");
    c = good_cfg();
    c.fields = IMGENV_ROLLOUT_NORM_STATES;
    REFUSED(seq_enable_plan(&c, &out, &f, nullptr, &want, msg), IMGENV_EINVAL, "imgenv_normalise_enable");
    c = good_cfg();
    {
        FeatureFacts none = f;
        none.roll_on = false;
        none.mb_on = false;
        REFUSED(seq_enable_plan(&c, &out, &none, nullptr, &want, msg), IMGENV_ESTATE, "before imgenv_rollout_enable");
    }
    CHECK_EQ(f.mb_on, 0);  // (accepted above without the minibatches)
    c.fields = IMGENV_ROLLOUT_LASERS;
    REFUSED(seq_enable_plan(&c, &out, &f, nullptr, &want, msg), IMGENV_EINVAL, "the rollout stores");
    c = good_cfg();
    c.fields = IMGENV_ROLLOUT_VECTOR_STATES;
    CHECK_EQ(seq_enable_plan(&c, &out, &f, nullptr, &want, msg), IMGENV_OK);
    CHECK_EQ(want, IMGENV_ROLLOUT_VECTOR_STATES);
    {   // the repeated call
        FeatureFacts on = f;
        on.seq_on = true;
        const imgenv_seq_cfg stored = good_cfg();
        c = good_cfg();
        CHECK_EQ(seq_enable_plan(&c, &out, &on, &stored, &want, msg), ENABLE_REPEAT);
        c.state_bytes[1] = 8;
        REFUSED(seq_enable_plan(&c, &out, &on, &stored, &want, msg), IMGENV_EINVAL, "already gathers sequences");
        c = good_cfg();
        c.length = 5;
        REFUSED(seq_enable_plan(&c, &out, &on, &stored, &want, msg), IMGENV_EINVAL, "already gathers sequences");
    }
    {   // C_max R beyond 2^31 - 1
        FeatureFacts big = f;
        big.RL = 1 << 20;
        big.roll_horizon = 1 << 11;
        c = good_cfg();
        c.length = 1;
        REFUSED(seq_enable_plan(&c, &out, &big, nullptr, &want, msg), IMGENV_EINVAL, "2^31");
        c.length = 2;  // 2^30 sequences
        CHECK_EQ(seq_enable_plan(&c, &out, &big, nullptr, &want, msg), IMGENV_OK);
    }
    {   // the selection: the minibatches' order under the sequences' own name
        FieldSelection s;
        ObsField ring[OBSF_COUNT] = {};
        ring[OBSF_VECTOR_STATES] = {(const void*)0x1000, 20};
        REFUSED(select_feature_fields(FIELDS_SEQ, ring, IMGENV_ROLLOUT_PED_MAPS_DRAWN, IMGENV_ROLLOUT_PED_MAPS_DRAWN, s, msg), IMGENV_EINVAL, "imgenv_seq_cfg.fields 512: no field");
        CHECK_EQ(select_feature_fields(FIELDS_SEQ, ring, IMGENV_ROLLOUT_VECTOR_STATES, 0, s, msg), IMGENV_OK);
        CHECK_EQ(s.n, 1);
        CHECK_EQ(OBS_SLOTS[OBSF_VECTOR_STATES].seq_out, offsetof(imgenv_seq_buffer, mb_vector_states));
        CHECK_EQ(OBS_SLOTS[OBSF_NORM_STATE_STACK].seq_out, offsetof(imgenv_seq_buffer, mb_norm_state_stack));
        CHECK_EQ(OBS_SLOTS[OBSF_PED_MAPS_DRAWN].seq_out, offsetof(imgenv_seq_buffer, mb_ped_maps));
        CHECK_EQ(OBS_SLOTS[OBSF_VIEW_MAPS].seq_out, OBS_NO_SLOT);
    }
    if (g_fail) {
        printf("%d of %d checks failed\n", g_fail, g_checks);
        return 1;
    }
    printf("OK %d checks SEQ_FLAG_BLOCK %d SEQ_MAX_STATES %d SEQ_MAX_STATE_BYTES %d\n", g_checks, SEQ_FLAG_BLOCK, SEQ_MAX_STATES, SEQ_MAX_STATE_BYTES);
    return 0;
}

static int run(const char* in_path, const char* out_path) {
    FILE* f = fopen(in_path, "rb");
    if (!f) return printf("FAIL: cannot open %s\n", in_path), 2;
    const int R = get_i32(f), T = get_i32(f), n = get_i32(f), L = get_i32(f), Bs = get_i32(f), j = get_i32(f), n_fields = get_i32(f);
    const int n_scalars = get_i32(f), normalise = get_i32(f), gather_blocks = get_i32(f);
    const int sb[2] = {get_i32(f), get_i32(f)};
    if (R < 1 || T < 1 || n < 1 || n > T || L < 1 || L > T || Bs < 1 || j < 0 || n_fields < 0 || n_fields > ROLLOUT_MAX_FIELDS || n_scalars < 0 ||
        n_scalars > MB_MAX_SCALARS || normalise < -1 || normalise >= n_scalars || sb[0] < 0 || sb[1] < 0 || sb[0] % 4 || sb[1] % 4)
        return printf("FAIL: bad header\n"), 2;
    uint32_t seed[2];
    get(f, seed, 8);
    float* norm = room_of<float>(2);
    get(f, norm, 8);
    std::vector<size_t> row_bytes((size_t)n_fields);
    for (int k = 0; k < n_fields; k++) row_bytes[(size_t)k] = (size_t)get_i32(f);
    std::vector<void*> mine;
    auto keep = [&](auto* p) {
        mine.push_back((void*)p);
        return p;
    };
    keep(norm);
    const size_t TR = (size_t)T * R, ring_rows = (size_t)(T + 1) * R, total_clean = (size_t)n * R;
    const size_t C = plan_seq_chunks((size_t)n, (size_t)L), S = plan_seq_chunks((size_t)T, (size_t)L) * R, CR = C * R, N = (size_t)L * Bs;
    uint8_t* clean = keep(room_of<uint8_t>(total_clean));  // (exactly n R flags: a read past the end is a finding)
    {
        std::vector<uint8_t> all(TR);
        get(f, all.data(), TR);
        memcpy(clean, all.data(), total_clean);
    }
    int32_t* final_idx = keep(room_of<int32_t>(ring_rows));
    get(f, final_idx, 4 * ring_rows);
    SeqGatherDev g;
    memset(&g, 0, sizeof(g));
    g.n_fields = n_fields;
    for (int k = 0; k < n_fields; k++) {
        const FinalFieldPlan p = plan_final_field(row_bytes[(size_t)k]);
        unsigned char* ring = keep(room(ring_rows * row_bytes[(size_t)k]));
        get(f, ring, ring_rows * row_bytes[(size_t)k]);
        g.f[k] = {ring, keep(room(N * row_bytes[(size_t)k])), p.unit, p.chunks};
        memset(g.f[k].dst, 0xAB, N * row_bytes[(size_t)k]);  // (the gather defines every byte)
        g.chunks_per_row += p.chunks;
    }
    if (n_fields == 0) g.chunks_per_row = 1;
    float* actions = keep(room_of<float>(TR * 3));
    float* rewards = keep(room_of<float>(TR));
    uint8_t* dones = keep(room_of<uint8_t>(TR));
    int32_t* info = keep(room_of<int32_t>(TR));
    get(f, actions, sizeof(float) * TR * 3);
    get(f, rewards, sizeof(float) * TR);
    get(f, dones, TR);
    get(f, info, sizeof(int32_t) * TR);
    for (int s = 0; s < n_scalars; s++) {
        float* a = keep(room_of<float>(ring_rows));
        get(f, a, sizeof(float) * ring_rows);
        g.scalars[s] = a;
    }
    for (int a = 0; a < 2; a++) {
        const FinalFieldPlan p = plan_final_field((size_t)sb[a]);
        g.st[a].unit = p.unit;
        g.st[a].chunks = sb[a] ? p.chunks : 0;
        g.state_chunks += g.st[a].chunks;
        if (!sb[a]) continue;
        unsigned char* src = keep(room(ring_rows * (size_t)sb[a]));
        get(f, src, ring_rows * (size_t)sb[a]);
        g.st[a].src = src;
        g.st[a].dst = keep(room((size_t)Bs * (size_t)sb[a]));
        memset(g.st[a].dst, 0xAB, (size_t)Bs * (size_t)sb[a]);
    }
    fclose(f);

    uint8_t* flag = keep(room_of<uint8_t>(CR));  // (exactly C R flags)
    int32_t* valid = keep(room_of<int32_t>(S));
    int32_t* order = keep(room_of<int32_t>(S));
    uint32_t* valid_n = keep(room_of<uint32_t>(1));
    const size_t tiles = plan_mb_tiles(S);
    int32_t* tile_count = keep(room_of<int32_t>(tiles));
    int32_t* tile_base = keep(room_of<int32_t>(tiles));

    const SeqFlagDev fd = {clean, flag, (uint32_t)R, (uint32_t)L, (uint32_t)n, (uint32_t)CR};
    {
        const unsigned grid = plan_seq_flag_launch(CR).grid;
        for (unsigned b = 0; b < grid; b++)
            for (unsigned lane = 0; lane < SEQ_FLAG_BLOCK; lane++) {
                const size_t q = (size_t)b * SEQ_FLAG_BLOCK + lane;
                if (q < (size_t)fd.total) seq_flag_item(fd, (uint32_t)q);
            }
    }
    const MbIndexDev d = {flag, valid, tile_count, tile_base, valid_n, (uint32_t)CR, (uint32_t)plan_mb_tiles(CR)};
    index_launches(d);
    const MbShuffleDev sh = {valid, valid_n, order, (uint32_t)S, mb_keys(seed[0], seed[1])};
    {
        const unsigned grid = plan_mb_shuffle_launch(S).grid;
        for (unsigned b = 0; b < grid; b++)
            for (unsigned lane = 0; lane < MB_SHUFFLE_BLOCK; lane++) {
                const size_t p = (size_t)b * MB_SHUFFLE_BLOCK + lane;
                if (p < (size_t)sh.TR) mb_shuffle_item(sh, *sh.valid_n, (uint32_t)p);
            }
    }

    g.order = order;
    g.first = (size_t)j * (size_t)Bs;
    g.Bs = (uint32_t)Bs; g.L = (uint32_t)L; g.R = (uint32_t)R; g.S = (uint32_t)S;
    g.n = n;
    g.actions = actions; g.rewards = rewards; g.dones = dones; g.is_clean = clean; g.dones_info = info; g.final_idx = final_idx;
    g.mb_actions = keep(room_of<float>(N * 3));
    g.mb_rewards = keep(room_of<float>(N));
    g.mb_dones = keep(room_of<uint8_t>(N));
    g.mb_dones_info = keep(room_of<int32_t>(N));
    g.mb_index = keep(room_of<int32_t>(N));
    g.mb_weight = keep(room_of<float>(N));
    g.mb_first = keep(room_of<uint8_t>(N));
    g.mb_scalars = keep(room_of<float>(N * MB_MAX_SCALARS));
    g.mb_seq = keep(room_of<int32_t>((size_t)Bs));
    g.mb_seq_len = keep(room_of<int32_t>((size_t)Bs));
    memset(g.mb_index, 0xAB, 4 * N);
    memset(g.mb_first, 0xAB, N);
    memset(g.mb_seq, 0xAB, 4 * (size_t)Bs);
    memset(g.mb_seq_len, 0xAB, 4 * (size_t)Bs);
    g.n_scalars = n_scalars;
    g.normalise = normalise;
    g.norm = norm;
    const unsigned blocks = gather_blocks > 0 ? (unsigned)gather_blocks : plan_seq_gather_launch((size_t)L, (size_t)Bs, g.chunks_per_row, g.state_chunks).grid;
    {
        const size_t items = seq_gather_items(g), stride = (size_t)blocks * ROLLOUT_BLOCK;
        for (unsigned b = 0; b < blocks; b++)
            for (unsigned lane = 0; lane < ROLLOUT_BLOCK; lane++)
                for (size_t t = (size_t)b * ROLLOUT_BLOCK + lane; t < items; t += stride) seq_gather_item(g, t);
    }

    FILE* o = fopen(out_path, "wb");
    if (!o) return printf("FAIL: cannot write %s\n", out_path), 2;
    fwrite(valid_n, 4, 1, o);
    fwrite(flag, 1, CR, o);
    fwrite(valid, 4, S, o);
    fwrite(order, 4, S, o);
    for (int k = 0; k < n_fields; k++) fwrite(g.f[k].dst, 1, N * row_bytes[(size_t)k], o);
    fwrite(g.mb_actions, 4, N * 3, o);
    fwrite(g.mb_rewards, 4, N, o);
    fwrite(g.mb_dones, 1, N, o);
    fwrite(g.mb_dones_info, 4, N, o);
    fwrite(g.mb_index, 4, N, o);
    fwrite(g.mb_weight, 4, N, o);
    fwrite(g.mb_first, 1, N, o);
    fwrite(g.mb_scalars, 4, N * MB_MAX_SCALARS, o);
    fwrite(g.mb_seq, 4, (size_t)Bs, o);
    fwrite(g.mb_seq_len, 4, (size_t)Bs, o);
    for (int a = 0; a < 2; a++)
        if (sb[a]) fwrite(g.st[a].dst, 1, (size_t)Bs * (size_t)sb[a], o);
    fclose(o);
    const unsigned n_valid = *valid_n, n_tiles = d.n_tiles;
    const size_t items = seq_gather_items(g);
    for (void* p : mine) free(p);
    printf("OK valid_n %u tiles %u gather_blocks %u items %zu\n", n_valid, n_tiles, blocks, items);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "plan")) return plan_checks();
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    printf("usage: %s plan | run case.bin result.bin\n", argv[0]);
    return 2;
}
