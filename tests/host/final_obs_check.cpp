// final_obs_check.cpp -- k_final_obs (img_env_amd/csrc/final_obs.h) on the CPU: the field-table planning of launch_plan.h
// (plan_final_field, plan_final_fields, plan_final_obs_launch) and the kernel's loop body, final_obs_item, run over a simulated
// grid of blocks x lanes for a listed chain, an unlisted one and a device-side count smaller than the grid's guess.
//   g++ -std=c++17 tests/host/final_obs_check.cpp -o check && ./check
// (also built with -fsanitize=address,undefined by tests/test_final_obs_plan.py: every access of the walk is then bounds-checked)
//
// Every byte of the final arrays is in one of three states, told apart by its value against the source byte s at the same place:
//   untouched  s ^ 0xFF   (the pattern every byte starts with)
//   written    s          (what an item leaves)
//   counted    s ^ 0x5A   (what this program turns a written byte into once it has looked at it)
// Before an item runs, the bytes a literal walk of the table expects it to write must be untouched; after it they must be written,
// and become counted.  At the end every byte of a covered row must be counted -- a second write would have turned it back into
// `written` -- and every byte of any other row untouched.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../img_env_amd/csrc/final_obs.h"

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

// the row sizes of the table: vector states of 3 and 5 floats, 15 floats, 11 doubles, 181 beams x 8, 360 beams x 8, a 48 x 48
// float16 sensor map, 3 x 48 x 48 floats of ped_maps, a one-byte flag, a stack of depth 3 of 181 beams x 8, and 6 bytes (unit 2)
static const size_t ROW_BYTES[] = {12, 20, 60, 88, 1448, 2880, 4608, 27648, 1, 3 * 1448, 6};
static const uint32_t UNITS[] = {4, 4, 4, 8, 8, 16, 16, 16, 1, 8, 2};
static const int N_FIELDS = (int)(sizeof(ROW_BYTES) / sizeof(ROW_BYTES[0]));

struct Arrays {
    int rows = 0;
    std::vector<unsigned char*> src, dst;  // 256-byte aligned, [rows][ROW_BYTES[k]]
    std::vector<uint32_t> count;
    explicit Arrays(int rows_) : rows(rows_), count((size_t)rows_) {
        uint32_t x = 12345u;
        for (int k = 0; k < N_FIELDS; k++) {
            const size_t bytes = (size_t)rows * ROW_BYTES[k], room = (bytes + 255) & ~(size_t)255;
            unsigned char* s = (unsigned char*)aligned_alloc(256, room);
            unsigned char* d = (unsigned char*)aligned_alloc(256, room);
            for (size_t b = 0; b < bytes; b++) {
                x = x * 1664525u + 1013904223u;
                s[b] = (unsigned char)(x >> 24);
                d[b] = s[b] ^ 0xFF;
            }
            src.push_back(s);
            dst.push_back(d);
        }
        for (int r = 0; r < rows; r++) count[(size_t)r] = (uint32_t)(7 * r + 3);
    }
    ~Arrays() {
        for (unsigned char* p : src) free(p);
        for (unsigned char* p : dst) free(p);
    }
};

// one launch over a grid of `blocks` x FINAL_BLOCK lanes; `covered`: the rows it must capture, in the chain's order
static void run_case(const char* name, int rows_total, const TailRows& rows, const std::vector<size_t>& covered, unsigned blocks) {
    Arrays a(rows_total);
    const FinalPlan plan = plan_final_fields(ROW_BYTES, N_FIELDS);
    FinalObsDev fo;
    memset(&fo, 0, sizeof(fo));
    fo.n_fields = plan.n_fields;
    fo.chunks_per_row = plan.chunks_per_row;
    fo.count = a.count.data();
    fo.rows = rows;
    for (int k = 0; k < N_FIELDS; k++) fo.f[k] = {a.dst[(size_t)k], a.src[(size_t)k], plan.f[k].unit, plan.f[k].chunks};
    const bool listed = rows.list != nullptr;
    const size_t cpr = plan.chunks_per_row, total = tail_rows_count(rows, listed) * cpr, stride = (size_t)blocks * FINAL_BLOCK;
    CHECK_EQ(total, covered.size() * cpr);
    std::vector<int> visits(total, 0);
    size_t not_untouched = 0, not_written = 0, items = 0;
    for (unsigned b = 0; b < blocks; b++)
        for (unsigned lane = 0; lane < FINAL_BLOCK; lane++)
            for (size_t t = (size_t)b * FINAL_BLOCK + lane; t < total; t += stride) {
                visits[t]++;
                items++;
                // the literal walk: which bytes of which field item t is to copy
                const size_t m = t / cpr, row = covered[m];
                size_t c = t % cpr;
                int k = 0;
                while (c >= ROW_BYTES[k] / UNITS[k]) {
                    c -= ROW_BYTES[k] / UNITS[k];
                    k++;
                }
                const size_t at = row * ROW_BYTES[k] + c * UNITS[k];
                unsigned char* d = a.dst[(size_t)k] + at;
                const unsigned char* s = a.src[(size_t)k] + at;
                for (uint32_t q = 0; q < UNITS[k]; q++) not_untouched += d[q] != (unsigned char)(s[q] ^ 0xFF);
                final_obs_item(fo, listed, t);
                for (uint32_t q = 0; q < UNITS[k]; q++) {
                    not_written += d[q] != s[q];
                    d[q] = s[q] ^ 0x5A;
                }
            }
    CHECK_EQ(items, total);
    size_t not_once = 0;
    for (int v : visits) not_once += v != 1;
    CHECK_EQ(not_once, 0);
    CHECK_EQ(not_untouched, 0);
    CHECK_EQ(not_written, 0);
    // the end state: covered rows counted byte for byte and their count one up, every other row as it was
    std::vector<int> is_covered((size_t)rows_total, 0);
    for (size_t r : covered) is_covered[r]++;
    size_t wrong_covered = 0, wrong_other = 0, wrong_count = 0;
    for (int r = 0; r < rows_total; r++) {
        const unsigned char want = is_covered[(size_t)r] ? 0x5A : 0xFF;
        for (int k = 0; k < N_FIELDS; k++) {
            const size_t at = (size_t)r * ROW_BYTES[k];
            for (size_t q = 0; q < ROW_BYTES[k]; q++) {
                const bool bad = a.dst[(size_t)k][at + q] != (unsigned char)(a.src[(size_t)k][at + q] ^ want);
                (is_covered[(size_t)r] ? wrong_covered : wrong_other) += bad;
            }
        }
        wrong_count += a.count[(size_t)r] != (uint32_t)(7 * r + 3 + is_covered[(size_t)r]);
    }
    CHECK_EQ(wrong_covered, 0);
    CHECK_EQ(wrong_other, 0);
    CHECK_EQ(wrong_count, 0);
    if (g_fail) printf("(case %s, %u blocks)\n", name, blocks);
}

int main() {
    // ---- the planner
    const FinalPlan plan = plan_final_fields(ROW_BYTES, N_FIELDS);
    CHECK_EQ(plan.n_fields, N_FIELDS);
    uint32_t cpr = 0;
    size_t bpr = 0;
    for (int k = 0; k < N_FIELDS; k++) {
        const FinalFieldPlan f = plan_final_field(ROW_BYTES[k]);
        CHECK_EQ(f.unit, UNITS[k]);
        CHECK_EQ(f.row_bytes, ROW_BYTES[k]);
        CHECK_EQ((size_t)f.chunks * f.unit, ROW_BYTES[k]);
        CHECK_EQ(plan.f[k].unit, f.unit);
        CHECK_EQ(plan.f[k].chunks, f.chunks);
        cpr += f.chunks;
        bpr += ROW_BYTES[k];
    }
    CHECK_EQ(plan.chunks_per_row, cpr);
    CHECK_EQ(plan.bytes_per_row, bpr);
    CHECK_EQ(plan_final_field(2).unit, 2);
    CHECK_EQ(plan_final_field(16).unit, 16);
    CHECK_EQ(plan_final_field(24).unit, 8);
    CHECK_EQ(plan_final_field(3).unit, 1);
    CHECK_EQ(N_FIELDS <= FINAL_MAX_FIELDS, 1);
    // the launch shape: rows x chunks in blocks of FINAL_BLOCK, capped at FINAL_MAX_BLOCKS
    PlanHandle h;
    h.RL = 6; h.Rw = 2; h.W = 3;
    PlanChain c;
    c.is_reset = true;
    CHECK_EQ(plan_final_obs_launch(h, c, cpr, 0).grid, (6 * (size_t)cpr + FINAL_BLOCK - 1) / FINAL_BLOCK);  // unlisted: every local row
    CHECK_EQ(plan_final_obs_launch(h, c, cpr, 0).block, FINAL_BLOCK);
    c.listed = true; c.act_nw = 2;
    CHECK_EQ(plan_final_obs_launch(h, c, cpr, 0).grid, (4 * (size_t)cpr + FINAL_BLOCK - 1) / FINAL_BLOCK);  // listed: Rw rows per world
    c.n_dev = true; c.act_nw = 3;                                                                            // the device's count: the guess, at most every world
    CHECK_EQ(plan_final_obs_launch(h, c, cpr, 16).grid, (6 * (size_t)cpr + FINAL_BLOCK - 1) / FINAL_BLOCK);
    CHECK_EQ(plan_final_obs_launch(h, c, cpr, 1).grid, (2 * (size_t)cpr + FINAL_BLOCK - 1) / FINAL_BLOCK);
    CHECK_EQ(plan_final_obs_launch(h, c, 1, 1).grid, 1);
    h.RL = 4000; h.Rw = 4; h.W = 1000;
    c.listed = false; c.n_dev = false;
    CHECK_EQ(plan_final_obs_launch(h, c, cpr, 0).grid, FINAL_MAX_BLOCKS);
    h.RL = 6; h.Rw = 2; h.W = 3;

    // ---- the walk, each case at the planner's grid and at 2 blocks (several strides)
    {   // listed: worlds 0 and 2 of 3, two robots each; world 1's rows stay
        const std::vector<int> list = {0, 2, 1};  // (the entry behind the count is not looked at)
        const TailRows r = {6, 2, list.data(), nullptr, 2};
        c.listed = true; c.n_dev = false; c.act_nw = 2;
        for (unsigned blocks : {plan_final_obs_launch(h, c, cpr, 0).grid, 2u}) run_case("listed", 6, r, {0, 1, 4, 5}, blocks);
        const std::vector<int> rev = {2, 0};
        const TailRows q = {6, 2, rev.data(), nullptr, 2};
        run_case("listed, reversed", 6, q, {4, 5, 0, 1}, 3);
    }
    {   // unlisted: every local row (imgenv_reset; a shard's local rows)
        const TailRows r = {6, 2, nullptr, nullptr, 3};
        c.listed = false; c.n_dev = false; c.act_nw = 3;
        for (unsigned blocks : {plan_final_obs_launch(h, c, cpr, 0).grid, 2u}) run_case("unlisted", 6, r, {0, 1, 2, 3, 4, 5}, blocks);
        const TailRows one = {5, 5, nullptr, nullptr, 1};
        run_case("unlisted, 5 rows", 5, one, {0, 1, 2, 3, 4}, 1);
    }
    {   // the device-side chain: the list holds room for every world, the count in device memory says one; the grid was sized for three
        const std::vector<int> list = {2, 0, 1};
        int n_dev = 1;
        const TailRows r = {6, 2, list.data(), &n_dev, 3};
        c.listed = true; c.n_dev = true; c.act_nw = 3;
        for (unsigned blocks : {plan_final_obs_launch(h, c, cpr, 16).grid, 2u}) run_case("device count 1", 6, r, {4, 5}, blocks);
        n_dev = 0;
        run_case("device count 0", 6, r, {}, plan_final_obs_launch(h, c, cpr, 16).grid);
        n_dev = 3;  // ... and more than a guess of one world: the blocks stride
        run_case("device count 3, guess 1", 6, r, {4, 5, 0, 1, 2, 3}, plan_final_obs_launch(h, c, cpr, 1).grid);
    }
    if (g_fail) {
        printf("%d of %d checks failed\n", g_fail, g_checks);
        return 1;
    }
    printf("OK %d checks FINAL_BLOCK %d FINAL_MAX_BLOCKS %d FINAL_MAX_FIELDS %d\n", g_checks, FINAL_BLOCK, FINAL_MAX_BLOCKS, FINAL_MAX_FIELDS);
    return 0;
}
