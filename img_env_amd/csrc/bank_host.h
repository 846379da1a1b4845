// bank_host.h -- the host plumbing the per-world banks (map_bank.h, track_bank.h, scenario_bank.h) and the enable paths beside them
// share: the validation of a (world, id) list, the choices a host-placed reset carries down to its launches, the epoch a device-side
// placement falls into, and the all-or-nothing allocation of device blocks.  Plain C++17, no HIP: tests/host/bank_host_check.cpp
// runs all of it under the sanitizers without a device.
#pragma once
#include <stdio.h>

#include <string>
#include <vector>

#include "../../include/imgenv.h"
#include "track_bank.h"

// The one validation of a (world, id) list: world in [0, W), no world twice and, where `ids` is given, id in [0, n_ids) -- entry by
// entry, so the first bad entry names the error in *err.  The caller applies nothing before this has passed.
template <size_t N>
static inline bool world_list_check(int W, int n, const int32_t* worlds, const int32_t* ids, int n_ids, const char* what, char (*err)[N]) {
    std::vector<char> seen((size_t)(W > 0 ? W : 0), 0);
    for (int q = 0; q < n; q++) {
        const int k = worlds[q];
        if (k < 0 || k >= W) return snprintf(*err, N, "world %d out of range (n_worlds %d)", k, W), false;
        if (seen[k]) return snprintf(*err, N, "world %d listed twice", k), false;
        if (ids && (ids[q] < 0 || ids[q] >= n_ids)) return snprintf(*err, N, "%s %d out of range (the handle holds %d)", what, ids[q], n_ids), false;
        seen[k] = 1;
    }
    return true;
}

// What a host-placed reset has chosen for the worlds it resets, in list order; null: not chosen by the host (the device takes the
// world's `next` or what the bank's policy says).  An argument of the reset path, valid for that call alone.
struct ResetChoices {
    const int* map_ids = nullptr;
    const int* track_ids = nullptr;
    const int* scn_ids = nullptr;
};

// The draws of a reset that places n worlds from seeds (null: placement q takes seed0 + q, wrapping): under BY_PLACEMENT the seed
// also draws the map and the recorded crowd.  n_maps / n_sets: the bank's size where the handle has that bank AND its policy is
// BY_PLACEMENT, else 0 (nothing drawn).  Owns what choices() points at.
struct PlacementDraws {
    std::vector<int> maps, sets;
    PlacementDraws(int n, const uint64_t* seeds, uint64_t seed0, int n_maps, int n_sets) {
        for (int q = 0; q < n; q++) {
            const uint64_t seed = seeds ? seeds[q] : seed0 + (uint64_t)q;
            if (n_maps > 0) maps.push_back(map_for_placement(seed, n_maps));
            if (n_sets > 0) sets.push_back(tracks_for_placement(seed, n_sets));
        }
    }
    ResetChoices choices() const { return ResetChoices{maps.empty() ? nullptr : maps.data(), sets.empty() ? nullptr : sets.data(), nullptr}; }
};

// The epoch of the scenario policy a device-side placement falls into: the last of the n_epochs (>= 1) that starts at or before
// placement number `serial` (two starting at the same count: the later one).  starts[0] is not read: epoch 0 starts at placement 0.
static inline size_t scenario_epoch_of(const unsigned long long* starts, size_t n_epochs, unsigned long long serial) {
    size_t e = n_epochs - 1;
    while (e > 0 && starts[e] > serial) e--;
    return e;
}

// The one all-or-nothing allocation of device blocks: a call allocates and fills everything it needs through one transaction and
// changes the handle only after commit().  After the first failure every later call is a no-op that returns false; the destructor
// of an uncommitted transaction frees every block it got.  Api: four static functions that return nullptr or the error's text --
// malloc(void**, bytes), free(void*), memset(void*, byte, bytes), memcpy(dst, src, bytes, bool from_device).
template <typename Api>
class DevTxn {
public:
    DevTxn() = default;
    DevTxn(const DevTxn&) = delete;
    DevTxn& operator=(const DevTxn&) = delete;
    ~DevTxn() {
        for (void* p : blocks_) (void)Api::free(p);
    }
    template <typename T>
    bool room(T** out, size_t count, int fill_byte) {  // `count` elements (at least one) of T, every byte `fill_byte`
        if (code_) return false;
        const size_t bytes = sizeof(T) * (count ? count : 1);
        void* p = nullptr;
        if (const char* e = Api::malloc(&p, bytes)) return fail(IMGENV_ENOMEM, "allocation", bytes, e);
        blocks_.push_back(p);
        *out = (T*)p;
        return done("fill", bytes, Api::memset(p, fill_byte, bytes));
    }
    bool put(void* dst, const void* src, size_t bytes) { return !code_ && (!bytes || done("upload", bytes, Api::memcpy(dst, src, bytes, false))); }
    bool copy(void* dst, const void* src, size_t bytes) { return !code_ && (!bytes || done("copy", bytes, Api::memcpy(dst, src, bytes, true))); }
    void commit(std::vector<void*>& owner) {  // the blocks become the owner's (the handle's `allocs`: freed with the handle)
        owner.insert(owner.end(), blocks_.begin(), blocks_.end());
        blocks_.clear();
    }
    int code() const { return code_; }  // IMGENV_OK, IMGENV_ENOMEM (an allocation failed) or IMGENV_EDEVICE (a fill or a copy did)
    const char* error() const { return error_.c_str(); }

private:
    bool done(const char* what, size_t bytes, const char* e) { return !e || fail(IMGENV_EDEVICE, what, bytes, e); }
    bool fail(int code, const char* what, size_t bytes, const char* e) {
        code_ = code;
        error_ = std::string(what) + " of " + std::to_string(bytes) + " bytes of device memory: " + e;
        return false;
    }
    std::vector<void*> blocks_;
    std::string error_;
    int code_ = IMGENV_OK;
};
