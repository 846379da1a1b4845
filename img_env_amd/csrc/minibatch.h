// minibatch.h -- a trainer's minibatches out of the rollout storage (rollout.h), on the device: which stored transitions count, a
// fresh random order over them, the statistics of a caller's array over them, and the gather of a minibatch into contiguous rows.
// k = t * R + row numbers the stored transitions, 0 <= k < n * R (n the cursor, R the local rows).
//
// Everything is the library's (imgenv_rollout_minibatch_enable; include/imgenv.h has the table):
//   valid [T R]   the k with is_clean[k] != 0, ascending;  valid_n  their count V
//   order [T R]   order[p] = valid[pi(p)] for p < V, -1 behind
//   tile_count / tile_base [tiles]   the index's scratch;  stat_part [tiles], stat_mean   the statistics'
//   mb_* per buffer   the gathered minibatch
//
// The index, three launches; the launch boundaries are the only synchronisation -- no workgroup ever waits for another:
//   k_mb_count    a workgroup per tile of MB_TILE flags, a lane per 16 flags (ONE 16-byte load; the flags behind the last whole
//                 16 byte by byte, never past n R): tile_count[tile] = the non-zero flags
//   k_mb_scan     ONE workgroup: tile_base = the exclusive prefix of tile_count, MB_SCAN_BLOCK tiles per round with a carry;
//                 valid_n = the sum
//   k_mb_scatter  the count's walk again: lane's popcount -> wave64 prefix (shuffles) -> the wavefronts' sums through LDS ->
//                 valid[tile_base + prefix ...] = the lane's set flags, ascending.  A stable compaction: deterministic.
// The statistics, four launches, float64, no atomics, every sum in a fixed order (two runs give identical bits):
//   k_mb_stats<SECOND>        a workgroup per MB_STATS_TILE positions p of the valid list: lane l adds x[valid[tile + i BLOCK + l]]
//                             (SECOND: (x - mean)^2) for i = 0 .. MB_STATS_PER_LANE - 1 with p < V, in that order; the lanes' sums
//                             fold by halves (l += l + 128, + 64, ... + 1) into stat_part[tile]
//   k_mb_stats_final<SECOND>  ONE workgroup: lane l adds stat_part[l], [l + BLOCK], ...; the same fold; mean = sum / V into
//                             stat_mean, or (SECOND) var = sum / V -- the POPULATION variance, not torch's unbiased default --
//                             and norm = ((float)mean, (float)(1 / sqrt(var + eps))); V == 0: (0, 1); var + eps == 0: (mean, 1)
// The shuffle, one launch, a lane per position p < T R: pi is a cycle-walking, unbalanced, alternating Feistel network over
//   b = max(2, bit_length(V - 1)) bits (mb_perm; include/imgenv.h has it written out), a bijection of [0, V).  V is read on the device.
// The gather, one launch: k_rollout's walk over (slot i < B, chunk c) -- chunks of 16 / 8 / 4 / 2 / 1 bytes (plan_final_field), a
//   lane per chunk, a flat grid-stride loop, the field table by value and selected with constant indices.  k = order[j B + i]
//   (-1 from T R on): k >= 0 copies chunk c of obs_<field>[k] into mb_<field>[i], k < 0 writes zeros; the lane of chunk 0 writes
//   the scalars (mb_gather_item).  No LDS, no scratch.
//
// Algorithmic bytes: index n R read twice + 4 V written; shuffle 4 V read (scattered) + 4 T R written; statistics 2 x (4 + 4) V
// read; a minibatch B x (the selected rows + 12 + 4 + 1 + 4 + 4 S) read and the same + 8 written.
//
// The per-item functions are host / device functions: tests/host/minibatch_check.cpp runs them over a simulated grid against
// tests/minibatch_model.py.  What crosses lanes -- the prefix of the popcounts, the fold of the partial sums -- is integer addition
// and mb_fold's fixed order, mirrored there lane by lane.
#pragma once
#include <math.h>
#include <stdint.h>

#include "field_rows.h"   // FieldChunk16
#include "launch_plan.h"  // MB_*, ROLLOUT_BLOCK, ROLLOUT_MAX_BLOCKS, ROLLOUT_TABLE_FIELDS
#include "rollout.h"      // ROLLOUT_UNROLL

#define MB_MAX_SCALARS 6  // (IMGENV_MB_MAX_SCALARS)

#if defined(__HIPCC__)
#define MB_WORDS(q) {q.x, q.y, q.z, q.w}
#else
#define MB_WORDS(q) {q.v[0], q.v[1], q.v[2], q.v[3]}
#endif

// ---- the index
struct MbIndexDev {
    const uint8_t* clean;  // [n][RL], 256-byte aligned
    int32_t* valid;        // [T RL]
    int32_t* tile_count;   // [tiles]
    int32_t* tile_base;
    uint32_t* valid_n;
    uint32_t total;        // n RL
    uint32_t n_tiles;      // ceil(total / MB_TILE)
};

// bit i: flag first + i is non-zero.  `first` is a multiple of 16 below `total`
TAIL_HD uint32_t mb_flags16(const uint8_t* clean, size_t total, size_t first) {
    uint32_t mask = 0;
    if (first + MB_LANE_FLAGS <= total) {
        const FieldChunk16 q = *(const FieldChunk16*)(clean + first);
        const uint32_t w[4] = MB_WORDS(q);
        ROLLOUT_UNROLL
        for (int i = 0; i < 4; i++) {
            ROLLOUT_UNROLL
            for (int b = 0; b < 4; b++) mask |= ((w[i] >> (8 * b)) & 0xffu) ? 1u << (4 * i + b) : 0u;
        }
    } else {
        for (size_t i = 0; first + i < total; i++) mask |= clean[first + i] ? 1u << i : 0u;  // (the tail: at most 15 bytes)
    }
    return mask;
}
// the flags of lane `lane` of tile `tile` (0 where the lane starts at or behind the end)
TAIL_HD uint32_t mb_lane_flags(const MbIndexDev& d, size_t tile, uint32_t lane) {
    const size_t first = tile * MB_TILE + (size_t)lane * MB_LANE_FLAGS;
    return first < d.total ? mb_flags16(d.clean, d.total, first) : 0u;
}
// the lane's set flags, ascending, from valid[at] on
TAIL_HD void mb_scatter16(int32_t* valid, size_t at, uint32_t mask, size_t first) {
    while (mask) {
        valid[at++] = (int32_t)(first + (size_t)__builtin_ctz(mask));
        mask &= mask - 1;
    }
}

// ---- the shuffle
struct MbKeys {
    uint32_t k[MB_ROUNDS];
};
TAIL_HD uint32_t mb_fmix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}
TAIL_HD MbKeys mb_keys(uint32_t seed_lo, uint32_t seed_hi) {
    MbKeys key;
    for (uint32_t r = 0; r < MB_ROUNDS; r++) key.k[r] = mb_fmix(seed_lo ^ (r * 0x9E3779B9u)) ^ seed_hi;
    return key;
}
// pi(x) for x < V: every round XORs one half with a function of the other, so the rounds are a bijection of [0, 2^b), 2^b < 2 V
// (V >= 3; 4 for V = 2), and a cycle through a point below V comes back below V: the walk ends
TAIL_HD uint32_t mb_perm(const MbKeys& key, uint32_t V, uint32_t x) {
    if (V <= 1) return x;
    const uint32_t top = V - 1;
    uint32_t b = 32u - (uint32_t)__builtin_clz(top);
    b = b < 2 ? 2 : b;
    const uint32_t hb = b / 2, ha = b - hb, mA = (1u << ha) - 1u, mB = (1u << hb) - 1u;
    do {
        uint32_t L = x >> hb, R = x & mB;
        ROLLOUT_UNROLL
        for (int r = 0; r < MB_ROUNDS; r += 2) {
            L ^= mb_fmix(R + key.k[r]) & mA;
            R ^= mb_fmix(L + key.k[r + 1]) & mB;
        }
        x = (L << hb) | R;
    } while (x >= V);
    return x;
}
struct MbShuffleDev {
    const int32_t* valid;
    const uint32_t* valid_n;
    int32_t* order;  // [T RL]
    uint32_t TR;
    MbKeys key;
};
TAIL_HD void mb_shuffle_item(const MbShuffleDev& s, uint32_t V, uint32_t p) { s.order[p] = p < V ? s.valid[mb_perm(s.key, V, p)] : -1; }

// ---- the statistics
struct MbStatsDev {
    const float* x;        // [T][RL], the caller's
    const int32_t* valid;
    const uint32_t* valid_n;
    double* part;          // [tiles]
    double* mean;          // [1]
    float* norm;           // [2]
    double eps;
    uint32_t n_tiles;      // ceil(n RL / MB_STATS_TILE)
};
// lane `lane` of tile `tile`: its MB_STATS_PER_LANE positions, in order
TAIL_HD double mb_stats_lane(const MbStatsDev& s, uint32_t V, bool second, double mean, size_t tile, uint32_t lane) {
    double acc = 0.0;
    for (int i = 0; i < MB_STATS_PER_LANE; i++) {
        const size_t p = tile * MB_STATS_TILE + (size_t)i * MB_STATS_BLOCK + lane;
        if (p >= V) break;
        double d = (double)s.x[s.valid[p]];
        if (second) {
            d = d - mean;
            d = d * d;
        }
        acc = acc + d;
    }
    return acc;
}
// lane `lane` of the reduction: the tiles' sums lane, lane + BLOCK, ...
TAIL_HD double mb_stats_final_lane(const MbStatsDev& s, uint32_t lane) {
    double acc = 0.0;
    for (size_t q = lane; q < s.n_tiles; q += MB_STATS_BLOCK) acc = acc + s.part[q];
    return acc;
}
// the fold of MB_STATS_BLOCK lane sums, as a workgroup does it round by round: a[l] += a[l + half], half = BLOCK / 2 .. 1
TAIL_HD double mb_fold(double* a) {
    for (int half = MB_STATS_BLOCK / 2; half > 0; half >>= 1)
        for (int l = 0; l < half; l++) a[l] = a[l] + a[l + half];
    return a[0];
}
TAIL_HD void mb_stats_mean(const MbStatsDev& s, uint32_t V, double sum) { s.mean[0] = V ? sum / (double)V : 0.0; }
TAIL_HD void mb_stats_norm(const MbStatsDev& s, uint32_t V, double sum) {
    if (V == 0) {
        s.norm[0] = 0.0f;
        s.norm[1] = 1.0f;
        return;
    }
    const double var = sum / (double)V, d = var + s.eps;
    s.norm[0] = (float)s.mean[0];
    s.norm[1] = d == 0.0 ? 1.0f : (float)(1.0 / sqrt(d));
}

// ---- the gather
struct MbGatherField {
    const unsigned char* ring;  // obs_<field> [T+1][RL][row bytes]
    unsigned char* dst;         // mb_<field> [B][row bytes] of the buffer in hand
    uint32_t unit, chunks;
};
struct MbGatherDev {
    MbGatherField f[ROLLOUT_TABLE_FIELDS];
    int32_t n_fields;
    uint32_t chunks_per_row;
    const int32_t* order;     // [T RL]
    size_t first;             // j B
    uint32_t B, TR;
    // the ring's [T][RL] arrays
    const float* actions;     // [.][3]
    const float* rewards;
    const uint8_t* dones;
    const int32_t* dones_info;
    // the buffer's [B] arrays
    float* mb_actions;
    float* mb_rewards;
    uint8_t* mb_dones;
    int32_t* mb_dones_info;
    int32_t* mb_index;
    float* mb_weight;
    float* mb_scalars;        // [MB_MAX_SCALARS][B]
    const float* scalars[MB_MAX_SCALARS];  // the caller's, indexed by k
    int32_t n_scalars, normalise;          // normalise: an index into scalars or -1
    const float* norm;        // [2]
};

template <typename T>
TAIL_HD void mb_gather_chunk(const unsigned char* ring, unsigned char* dst, uint32_t chunks, int32_t k, size_t i, uint32_t c) {
    T v = T{};
    if (k >= 0) v = ((const T*)ring)[(size_t)k * chunks + c];
    ((T*)dst)[i * (size_t)chunks + c] = v;
}
template <int S>
TAIL_HD void mb_gather_scalars(const MbGatherDev& g, int32_t k, size_t i) {
    if constexpr (S < MB_MAX_SCALARS) {
        if (S < g.n_scalars) {
            float v = 0.0f;
            if (k >= 0) {
                v = g.scalars[S][k];
                if (S == g.normalise) {
                    const float d = v - g.norm[0];  // (two roundings: the build has -ffp-contract=off)
                    v = d * g.norm[1];
                }
            }
            g.mb_scalars[(size_t)S * g.B + i] = v;
            mb_gather_scalars<S + 1>(g, k, i);
        }
    }
}
// item t of a launch: chunk t % chunks_per_row of slot t / chunks_per_row
TAIL_HD void mb_gather_item(const MbGatherDev& g, size_t t) {
    const size_t i = t / g.chunks_per_row;
    uint32_t c = (uint32_t)(t - i * g.chunks_per_row);
    const size_t pos = g.first + i;
    const int32_t k = pos < (size_t)g.TR ? g.order[pos] : -1;
    if (c == 0) {  // (one lane per slot)
        float v = 0.0f, w = 0.0f, beep = 0.0f, reward = 0.0f;
        uint8_t done = 0;
        int32_t info = 0;
        if (k >= 0) {
            v = g.actions[(size_t)k * 3]; w = g.actions[(size_t)k * 3 + 1]; beep = g.actions[(size_t)k * 3 + 2];
            reward = g.rewards[k];
            done = g.dones[k];
            info = g.dones_info[k];
        }
        g.mb_actions[i * 3] = v;
        g.mb_actions[i * 3 + 1] = w;
        g.mb_actions[i * 3 + 2] = beep;
        g.mb_rewards[i] = reward;
        g.mb_dones[i] = done;
        g.mb_dones_info[i] = info;
        g.mb_index[i] = k >= 0 ? k : -1;
        g.mb_weight[i] = k >= 0 ? 1.0f : 0.0f;
        mb_gather_scalars<0>(g, k, i);
    }
    if (g.n_fields == 0) return;  // (every selected field is drawn, ped_draw.h: chunks_per_row is 1, the scalars' lane)
    const MbGatherField f = field_walk(g.f, g.n_fields, c);
    field_dispatch(f.unit, [&](auto chunk) { mb_gather_chunk<typename decltype(chunk)::type>(f.ring, f.dst, f.chunks, k, i, c); });
}

#if defined(__HIPCC__)
// the exclusive prefix of `v` over the workgroup's lanes, and the workgroup's sum: shuffles inside a wavefront, `wave_sum` (LDS,
// one word per wavefront) across them.  Every lane of the workgroup calls it.
template <int BLOCK>
__device__ __forceinline__ int mb_block_prefix(int v, int* wave_sum, int& total) {
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    int inc = v;
    ROLLOUT_UNROLL
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wave_sum[wv] = inc;
    __syncthreads();
    int before = 0;
    total = 0;
    ROLLOUT_UNROLL
    for (int q = 0; q < BLOCK / 64; q++) {
        const int s = wave_sum[q];
        before += q < wv ? s : 0;
        total += s;
    }
    __syncthreads();  // (wave_sum is written again by the caller's next round)
    return before + inc - v;
}

__global__ __launch_bounds__(MB_INDEX_BLOCK) void k_mb_count(const MbIndexDev d) {
    __shared__ int wave_sum[MB_INDEX_BLOCK / 64];
    int total;
    (void)mb_block_prefix<MB_INDEX_BLOCK>(__builtin_popcount(mb_lane_flags(d, blockIdx.x, threadIdx.x)), wave_sum, total);
    if (threadIdx.x == 0 && blockIdx.x < d.n_tiles) d.tile_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(MB_SCAN_BLOCK) void k_mb_scan(const MbIndexDev d) {
    __shared__ int wave_sum[MB_SCAN_BLOCK / 64];
    uint32_t carry = 0;  // (the same in every lane)
    for (uint32_t base = 0; base < d.n_tiles; base += MB_SCAN_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        int total;
        const int before = mb_block_prefix<MB_SCAN_BLOCK>(i < d.n_tiles ? d.tile_count[i] : 0, wave_sum, total);
        if (i < d.n_tiles) d.tile_base[i] = (int32_t)(carry + (uint32_t)before);
        carry += (uint32_t)total;
    }
    if (threadIdx.x == 0) *d.valid_n = carry;
}

__global__ __launch_bounds__(MB_INDEX_BLOCK) void k_mb_scatter(const MbIndexDev d) {
    __shared__ int wave_sum[MB_INDEX_BLOCK / 64];
    const uint32_t mask = mb_lane_flags(d, blockIdx.x, threadIdx.x);
    int total;
    const int before = mb_block_prefix<MB_INDEX_BLOCK>(__builtin_popcount(mask), wave_sum, total);
    if (blockIdx.x < d.n_tiles)
        mb_scatter16(d.valid, (size_t)d.tile_base[blockIdx.x] + (size_t)before, mask, (size_t)blockIdx.x * MB_TILE + (size_t)threadIdx.x * MB_LANE_FLAGS);
}

__global__ __launch_bounds__(MB_SHUFFLE_BLOCK) void k_mb_shuffle(const MbShuffleDev s) {
    const size_t p = (size_t)blockIdx.x * MB_SHUFFLE_BLOCK + threadIdx.x;
    if (p < (size_t)s.TR) mb_shuffle_item(s, *s.valid_n, (uint32_t)p);
}

// the workgroup's fold of the lanes' sums, in mb_fold's order; the result in lane 0
__device__ __forceinline__ double mb_block_fold(double acc, double* a) {
    a[threadIdx.x] = acc;
    __syncthreads();
    for (int half = MB_STATS_BLOCK / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) a[threadIdx.x] = a[threadIdx.x] + a[threadIdx.x + half];
        __syncthreads();
    }
    return a[0];
}
template <bool SECOND>
__global__ __launch_bounds__(MB_STATS_BLOCK) void k_mb_stats(const MbStatsDev s) {
    __shared__ double a[MB_STATS_BLOCK];
    const double sum = mb_block_fold(mb_stats_lane(s, *s.valid_n, SECOND, SECOND ? s.mean[0] : 0.0, blockIdx.x, threadIdx.x), a);
    if (threadIdx.x == 0 && blockIdx.x < s.n_tiles) s.part[blockIdx.x] = sum;
}
template <bool SECOND>
__global__ __launch_bounds__(MB_STATS_BLOCK) void k_mb_stats_final(const MbStatsDev s) {
    __shared__ double a[MB_STATS_BLOCK];
    const double sum = mb_block_fold(mb_stats_final_lane(s, threadIdx.x), a);
    if (threadIdx.x == 0) {
        if (SECOND)
            mb_stats_norm(s, *s.valid_n, sum);
        else
            mb_stats_mean(s, *s.valid_n, sum);
    }
}

__global__ __launch_bounds__(ROLLOUT_BLOCK) void k_rollout_gather(const MbGatherDev g) {
    const size_t total = (size_t)g.B * g.chunks_per_row, stride = (size_t)gridDim.x * ROLLOUT_BLOCK;
    for (size_t t = (size_t)blockIdx.x * ROLLOUT_BLOCK + threadIdx.x; t < total; t += stride) mb_gather_item(g, t);
}
#endif
