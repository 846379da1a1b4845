// tail_rows_check.cpp -- the row walk of the chain-tail kernels (img_env_amd/csrc/tail_rows.h) on the CPU: tail_rows_count /
// tail_rows_row against a literal double loop over (world in list, robot in world), and the item mapping k_stack and k_obs_post
// build on top of it (a grid-stride loop over rows x per_row items) over a simulated grid.
//   g++ -std=c++17 tests/host/tail_rows_check.cpp -o check && ./check
#include <stdio.h>

#include <vector>

#include "../../img_env_amd/csrc/tail_rows.h"

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

// the rows a launch covers, in order, by the header's two functions
static std::vector<size_t> walk(const TailRows& r, bool listed) {
    std::vector<size_t> rows;
    const size_t n = tail_rows_count(r, listed);
    for (size_t m = 0; m < n; m++) rows.push_back(tail_rows_row(r, listed, m));
    return rows;
}
// ... and written out: every local robot, or robot by robot of the first n listed worlds
static std::vector<size_t> expected(int RL, int Rw, const std::vector<int>* list, int n) {
    std::vector<size_t> rows;
    if (!list) {
        for (int i = 0; i < RL; i++) rows.push_back((size_t)i);
        return rows;
    }
    for (int q = 0; q < n; q++)
        for (int i = 0; i < Rw; i++) rows.push_back((size_t)((*list)[q] * Rw + i));
    return rows;
}
static void check_rows(const std::vector<size_t>& got, const std::vector<size_t>& want) {
    CHECK_EQ(got.size(), want.size());
    for (size_t k = 0; k < got.size() && k < want.size(); k++) CHECK_EQ(got[k], want[k]);
}

// The composition the kernels use: lane `lane` of block `b` of a grid of `blocks` x `block` takes the items t = b * block + lane,
// t + blocks * block, ...; item t is element e = t - m * per_row of the m-th covered row, m = t / per_row.  Every (row, element)
// pair of the launch must be visited exactly once.
static void check_items(const TailRows& r, bool listed, size_t per_row, int blocks, int block, size_t rows_total) {
    const size_t n_rows = tail_rows_count(r, listed), total = n_rows * per_row, stride = (size_t)blocks * block;
    std::vector<int> seen(rows_total * per_row, 0);
    size_t out_of_range = 0;
    for (int b = 0; b < blocks; b++)
        for (int lane = 0; lane < block; lane++)
            for (size_t t = (size_t)b * block + lane; t < total; t += stride) {
                const size_t m = t / per_row, e = t - m * per_row, row = tail_rows_row(r, listed, m);
                if (row >= rows_total || e >= per_row) out_of_range++;
                else seen[row * per_row + e]++;
            }
    CHECK_EQ(out_of_range, 0);
    // the covered rows once per element, every other row never
    std::vector<int> want(rows_total * per_row, 0);
    for (size_t row : walk(r, listed))
        for (size_t e = 0; e < per_row; e++) want[row * per_row + e] = 1;
    size_t wrong = 0, visited = 0;
    for (size_t k = 0; k < seen.size(); k++) {
        wrong += seen[k] != want[k];
        visited += (size_t)seen[k];
    }
    CHECK_EQ(wrong, 0);
    CHECK_EQ(visited, total);
}

int main() {
    // not listed: rows 0 .. RL-1, each exactly once (a list that is there is not looked at: a step's instantiation)
    for (int RL : {1, 5, 257}) {
        const std::vector<int> ignored = {3};
        for (const int* list : {(const int*)nullptr, ignored.data()}) {
            const TailRows r = {RL, RL, list, nullptr, 1};
            CHECK_EQ(tail_rows_count(r, false), RL);
            check_rows(walk(r, false), expected(RL, RL, nullptr, 0));
        }
    }
    {   // listed: four worlds of three robots, the list {2, 0}
        const std::vector<int> list = {2, 0, 3, 1};  // (entries behind the count are not looked at)
        TailRows r = {12, 3, list.data(), nullptr, 2};
        const std::vector<size_t> both = {6, 7, 8, 0, 1, 2};
        check_rows(walk(r, true), both);
        check_rows(walk(r, true), expected(12, 3, &list, 2));
        // the device-side chain: the counted length wins over the host's
        int n_dev = 1;
        r.n_dev = &n_dev;
        r.n_worlds = 4;
        const std::vector<size_t> first = {6, 7, 8};
        check_rows(walk(r, true), first);
        check_rows(walk(r, true), expected(12, 3, &list, 1));
        n_dev = 0;
        CHECK_EQ(tail_rows_count(r, true), 0);
        CHECK_EQ(walk(r, true).size(), 0);
        // ... and not listed it is every local robot again, whatever the count says
        check_rows(walk(r, false), expected(12, 3, nullptr, 0));
    }
    {   // one robot per world, every world listed in reverse order
        const int W = 7;
        std::vector<int> list;
        for (int k = W - 1; k >= 0; k--) list.push_back(k);
        const TailRows r = {W, 1, list.data(), nullptr, W};
        const std::vector<size_t> rows = walk(r, true);
        CHECK_EQ(rows.size(), W);
        for (int k = 0; k < W && k < (int)rows.size(); k++) CHECK_EQ(rows[k], W - 1 - k);
        check_rows(rows, expected(W, 1, &list, W));
    }
    // the item mapping on 2 blocks x 256 lanes
    for (size_t per_row : {(size_t)1, (size_t)20, (size_t)71}) {
        {   // 6 rows x 71 items (a listed chain of 2 worlds x 3 robots)
            const std::vector<int> list = {2, 0};
            const TailRows r = {12, 3, list.data(), nullptr, 2};
            check_items(r, true, per_row, 2, 256, 12);
            int n_dev = 1;
            TailRows d = r;
            d.n_dev = &n_dev;
            d.n_worlds = 4;
            check_items(d, true, per_row, 2, 256, 12);
        }
        {   // 1500 items and more: several strides of the grid's 512 lanes
            const int RL = (int)((1500 + per_row - 1) / per_row);
            const TailRows r = {RL, RL, nullptr, nullptr, 1};
            check_items(r, false, per_row, 2, 256, (size_t)RL);
            // the same rows as a listed chain over every world, in reverse
            std::vector<int> list;
            for (int k = RL - 1; k >= 0; k--) list.push_back(k);
            const TailRows l = {RL, 1, list.data(), nullptr, RL};
            check_items(l, true, per_row, 2, 256, (size_t)RL);
        }
    }
    if (g_fail) {
        printf("%d of %d checks failed\n", g_fail, g_checks);
        return 1;
    }
    printf("OK %d checks\n", g_checks);
    return 0;
}
