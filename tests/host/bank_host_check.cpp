// bank_host_check.cpp -- the host plumbing the banks share (img_env_amd/csrc/bank_host.h) without a device: the (world, id) list
// check with its messages, the draws a host-placed reset carries, the epoch search, and DevTxn over a fake device that allocates
// with malloc and fails at a chosen call.  Built with -fsanitize=address,undefined by tests/test_bank_host.py, so a block that a
// failed transaction leaks or frees twice fails the run.
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -I include tests/host/bank_host_check.cpp -o check && ./check
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../img_env_amd/csrc/bank_host.h"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        g_checks++;                                                  \
        if (!(cond)) {                                               \
            g_fail++;                                                \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
        }                                                            \
    } while (0)

// ---------------------------------------------------------------------------------------- world_list_check
static std::string refused(int W, std::vector<int32_t> worlds, const std::vector<int32_t>* ids, int n_ids, const char* what) {
    char err[64] = "(accepted)";  // (as long as the longest message needs)
    const bool ok = world_list_check(W, (int)worlds.size(), worlds.data(), ids ? ids->data() : nullptr, n_ids, what, &err);
    CHECK(ok == (strcmp(err, "(accepted)") == 0));  // err is written exactly when the list is refused
    return err;
}

static void check_world_lists() {
    const std::vector<int32_t> five{0, 1, 2, 0, 1};
    for (int W : {1, 5}) {
        char want[96];
        CHECK(refused(W, {}, nullptr, 0, "map") == "(accepted)");  // n = 0
        CHECK(refused(W, {W - 1}, nullptr, 0, nullptr) == "(accepted)");
        snprintf(want, sizeof(want), "world -1 out of range (n_worlds %d)", W);
        CHECK(refused(W, {-1}, nullptr, 0, "map") == want);
        snprintf(want, sizeof(want), "world %d out of range (n_worlds %d)", W, W);
        CHECK(refused(W, {W}, nullptr, 0, "map") == want);
        CHECK(refused(W, {0, W}, nullptr, 0, "map") == want);
        CHECK(refused(W, {0, 0}, nullptr, 0, "map") == "world 0 listed twice");  // (W = 1: the only list of two)
        // ids: -1 and n_ids, the three names; a null ids checks the worlds alone
        std::vector<int32_t> ids{-1};
        CHECK(refused(W, {0}, &ids, 3, "map") == "map -1 out of range (the handle holds 3)");
        ids = {3};
        CHECK(refused(W, {0}, &ids, 3, "track set") == "track set 3 out of range (the handle holds 3)");
        ids = {7};
        CHECK(refused(W, {0}, &ids, 7, "scenario") == "scenario 7 out of range (the handle holds 7)");
        ids = {2};
        CHECK(refused(W, {0}, &ids, 3, "map") == "(accepted)");
        CHECK(refused(W, {0}, nullptr, 0, "map") == "(accepted)");
    }
    // W = 5: a duplicate in the first two and in the last two positions, every world once, and the first bad entry names the error
    CHECK(refused(5, {3, 3, 1, 0}, nullptr, 0, "map") == "world 3 listed twice");
    CHECK(refused(5, {4, 2, 1, 1}, nullptr, 0, "map") == "world 1 listed twice");
    CHECK(refused(5, {4, 2, 0, 3, 1}, &five, 3, "map") == "(accepted)");
    const std::vector<int32_t> bad_then_dup{0, 9, 0};
    CHECK(refused(5, {2, 3, 3}, &bad_then_dup, 3, "track set") == "track set 9 out of range (the handle holds 3)");
    CHECK(refused(5, {2, 2, 3}, &bad_then_dup, 3, "track set") == "world 2 listed twice");
    CHECK(refused(5, {2, 5, 3}, &bad_then_dup, 3, "track set") == "world 5 out of range (n_worlds 5)");
}

// ---------------------------------------------------------------------------------------- the draws of host-placed resets
static void check_draws() {
    const uint64_t seeds[4] = {0, UINT64_MAX, 0x9E3779B97F4A7C15ull, 12345};
    {   // no bank, or policy KEEP: nothing chosen by the host
        const PlacementDraws d(4, seeds, 0, 0, 0);
        const ResetChoices c = d.choices();
        CHECK(!c.map_ids && !c.track_ids && !c.scn_ids);
    }
    {   // an array of seeds
        const PlacementDraws d(4, seeds, 777, 3, 5);
        const ResetChoices c = d.choices();
        CHECK(c.map_ids && c.track_ids && !c.scn_ids && d.maps.size() == 4 && d.sets.size() == 4);
        bool differ = false;
        for (int q = 0; q < 4 && c.map_ids && c.track_ids; q++) {
            CHECK(c.map_ids[q] == map_for_placement(seeds[q], 3));
            CHECK(c.track_ids[q] == tracks_for_placement(seeds[q], 5));
            differ = differ || c.map_ids[q] != c.map_ids[0];
        }
        CHECK(differ);  // (the seeds do not all draw one map: the entries are per placement)
    }
    {   // seed0 + q, wrapping past UINT64_MAX into 0
        const uint64_t seed0 = UINT64_MAX - 1;
        const PlacementDraws d(4, nullptr, seed0, 3, 5);
        const ResetChoices c = d.choices();
        const uint64_t want[4] = {UINT64_MAX - 1, UINT64_MAX, 0, 1};
        for (int q = 0; q < 4 && c.map_ids && c.track_ids; q++) {
            CHECK(c.map_ids[q] == map_for_placement(want[q], 3));
            CHECK(c.track_ids[q] == tracks_for_placement(want[q], 5));
        }
    }
    {   // one bank alone draws alone
        const PlacementDraws m(2, seeds, 0, 3, 0), t(2, seeds, 0, 0, 5);
        CHECK(m.choices().map_ids && !m.choices().track_ids && !t.choices().map_ids && t.choices().track_ids);
    }
}

// ---------------------------------------------------------------------------------------- scenario_epoch_of
// the definition, forwards: the last epoch that starts at or before the placement, epoch 0 starting at 0 whatever its slot holds
static size_t epoch_forwards(const std::vector<unsigned long long>& starts, unsigned long long serial) {
    size_t e = 0;
    for (size_t q = 1; q < starts.size(); q++)
        if (starts[q] <= serial) e = q;
    return e;
}

static void check_epochs() {
    const std::vector<unsigned long long> log{0xDEADBEEFull, 5, 5, 9}, one{0xDEADBEEFull};
    const unsigned long long serials[6] = {0, 4, 5, 8, 9, UINT64_MAX - 1};
    const size_t want[6] = {0, 0, 2, 2, 3, 3};  // (two epochs starting at 5: the later one)
    for (int q = 0; q < 6; q++) {
        CHECK(scenario_epoch_of(log.data(), log.size(), serials[q]) == want[q]);
        CHECK(scenario_epoch_of(log.data(), log.size(), serials[q]) == epoch_forwards(log, serials[q]));
        CHECK(scenario_epoch_of(one.data(), one.size(), serials[q]) == 0);
    }
}

// ---------------------------------------------------------------------------------------- DevTxn over a fake device
struct FakeApi {
    static int calls, fail_at, live;  // malloc / memset / memcpy calls so far, the one that fails (0: none), blocks not yet freed
    static const char* tick() { return ++calls == fail_at ? "fake failure" : nullptr; }
    static const char* malloc(void** p, size_t bytes) {
        if (const char* e = tick()) return e;
        *p = ::malloc(bytes);
        live++;
        return nullptr;
    }
    static const char* free(void* p) {
        ::free(p);
        live--;
        return nullptr;
    }
    static const char* memset(void* p, int byte, size_t bytes) {
        if (const char* e = tick()) return e;
        ::memset(p, byte, bytes);
        return nullptr;
    }
    static const char* memcpy(void* dst, const void* src, size_t bytes, bool) {
        if (const char* e = tick()) return e;
        ::memcpy(dst, src, bytes);
        return nullptr;
    }
};
int FakeApi::calls = 0, FakeApi::fail_at = 0, FakeApi::live = 0;

// three rooms, two uploads, one copy: nine calls of the Api, the mallocs being calls 1, 3 and 5
static const int RECIPE_CALLS = 9;
struct Recipe {
    int32_t* a = nullptr;
    double* b = nullptr;
    unsigned char* c = nullptr;
    bool step[6];
};
static void run_recipe(DevTxn<FakeApi>& txn, Recipe& r) {
    static const int32_t src_a[3] = {7, -8, 9};
    static const double src_b[2] = {0.5, -2.0};
    r.step[0] = txn.room(&r.a, 3, 0);
    r.step[1] = txn.room(&r.b, 4, 0xFF);
    r.step[2] = txn.room(&r.c, 0, 0x11);  // (no elements: one)
    r.step[3] = txn.put(r.a, src_a, sizeof(src_a));
    r.step[4] = txn.put(r.b, src_b, sizeof(src_b));
    r.step[5] = txn.copy(r.b + 2, r.b, 8);
}

static void check_transactions() {
    int sentinel = 0;
    for (int j = 1; j <= RECIPE_CALLS; j++) {  // the j-th call of the Api fails
        std::vector<void*> owner{&sentinel};
        FakeApi::calls = 0, FakeApi::fail_at = j, FakeApi::live = 0;
        {
            DevTxn<FakeApi> txn;
            Recipe r;
            run_recipe(txn, r);
            const int first_bad = j <= 6 ? (j - 1) / 2 : j - 4;  // the step call j belongs to
            for (int s = 0; s < 6; s++) CHECK(r.step[s] == (s < first_bad));
            CHECK(FakeApi::calls == j);  // every call of the transaction behind the failure made nothing
            const bool was_malloc = j == 1 || j == 3 || j == 5;
            CHECK(txn.code() == (was_malloc ? IMGENV_ENOMEM : IMGENV_EDEVICE));
            CHECK(strstr(txn.error(), "fake failure") != nullptr);
            CHECK(FakeApi::live == (j <= 6 ? j / 2 : 3));  // (the blocks it got: its own until it dies)
        }
        CHECK(FakeApi::live == 0);
        CHECK(owner.size() == 1 && owner[0] == &sentinel);
    }
    {   // nothing fails: the recipe's blocks become the owner's, filled as asked, and the destructor frees nothing
        std::vector<void*> owner{&sentinel};
        FakeApi::calls = 0, FakeApi::fail_at = 0, FakeApi::live = 0;
        Recipe r;
        {
            DevTxn<FakeApi> txn;
            run_recipe(txn, r);
            for (int s = 0; s < 6; s++) CHECK(r.step[s]);
            CHECK(txn.code() == IMGENV_OK && FakeApi::calls == RECIPE_CALLS);
            CHECK(txn.put(r.a, nullptr, 0) && txn.copy(r.a, nullptr, 0) && FakeApi::calls == RECIPE_CALLS);  // (no bytes: no call)
            txn.commit(owner);
        }
        CHECK(FakeApi::live == 3);
        CHECK(owner.size() == 4 && owner[0] == &sentinel && owner[1] == r.a && owner[2] == r.b && owner[3] == r.c);
        CHECK(r.a[0] == 7 && r.a[1] == -8 && r.a[2] == 9);
        CHECK(r.b[0] == 0.5 && r.b[1] == -2.0 && r.b[2] == 0.5);
        unsigned char ff[8];
        memset(ff, 0xFF, 8);
        CHECK(memcmp(r.b + 3, ff, 8) == 0 && r.c[0] == 0x11);
        for (size_t q = 1; q < owner.size(); q++) (void)FakeApi::free(owner[q]);
        CHECK(FakeApi::live == 0);
    }
}

int main() {
    check_world_lists();
    check_draws();
    check_epochs();
    check_transactions();
    if (g_fail) {
        printf("%d of %d checks failed\n", g_fail, g_checks);
        return 1;
    }
    printf("OK %d checks\n", g_checks);
    return 0;
}
