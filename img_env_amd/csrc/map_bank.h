// map_bank.h -- several static maps in one handle (include/imgenv.h: imgenv_maps_add): the bank [n_maps][stride] of occupancy grids
// every reset starts from, which of them each world's current episode runs on (cur) and which its next reset takes (next).
//
// Both [W] arrays live in device memory, not in kernel arguments: the device-side reset chain (csrc/spawn_device.h) chooses a
// world's map inside k_respawn and the map restore behind it, in the same chain, reads the choice back -- the host never knows it.
// A handle without a bank passes null pointers and every reset takes the one map of imgenv_create, as before.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MAP_BANK_HD __host__ __device__
#else
#define MAP_BANK_HD
#endif

// The map an episode placed from `seed` runs on under IMGENV_MAPS_BY_PLACEMENT: splitmix64's finaliser over the seed, its upper
// 32 bits scaled into [0, n_maps) by multiply-shift (every map is hit by floor or ceil of 2^32 / n_maps of the 2^32 values: no
// bias beyond 2^-32).  Integers only, one definition for the host (imgenv_map_for_placement, the host-placed resets) and the
// device (k_respawn): they agree bit for bit.
MAP_BANK_HD static inline int32_t map_for_placement(uint64_t seed, int32_t n_maps) {
    if (n_maps <= 1) return 0;
    uint64_t z = seed + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (int32_t)(((z >> 32) * (uint64_t)(uint32_t)n_maps) >> 32);
}

struct MapSel {
    int* cur;             // [W] map of each world's current episode; nullptr: the handle has no bank (everything is map 0)
    int* next;            // [W] map each world's next reset starts from
    const int* ids;       // host-placed resets under BY_PLACEMENT: the maps of the worlds of this reset, in list order (page-locked), else nullptr
    size_t stride;        // bytes between two maps of the bank (the grid padded to 16)
    int n_maps;
    int by_placement;     // IMGENV_MAPS_BY_PLACEMENT: the device-side reset draws the map from the placement's seed
};

#if defined(__HIPCC__)
// next[worlds[q]] = ids[q], from page-locked host memory: the scatter of imgenv_world_maps_set and, over the track bank's `next`,
// of imgenv_world_tracks_set
__global__ void k_world_select(int* __restrict__ next, const int* __restrict__ worlds, const int* __restrict__ ids, int n) {
    const int q = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (q < n) next[worlds[q]] = ids[q];
}
#endif
