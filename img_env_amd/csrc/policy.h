// policy.h -- the policy head of the action side (include/imgenv.h: imgenv_policy_enable): what a network emits for every local
// robot -- logits over the YAML's discrete_actions, or a mean and a log-std over its continuous_actions -- becomes, in ONE launch
// in front of the step, the sampled action with its log-probability and entropy, the float32 (v, w, beep) row and the masked
// `speeds` that k_actions (actions.h) would have written for it, and, where the rollout window keeps them, the action / log-prob /
// value columns of the window's slot.  A sibling of k_actions: same outputs, same ordering contract, same n_bad ballot.
//
// Random numbers: Philox4x32-10, stateless.  counter = (g lo, g hi, draw lo, draw hi) with g = robot_begin + r the GLOBAL robot
// number, key = (seed lo, seed hi): a robot shard draws what the whole world draws, and nothing is kept between calls.  The third
// Gaussian column takes a second block whose counter has draw hi ^ 0x80000000.  u = float(x >> 8) * 2^-24 is exact and in [0, 1).
//
// Categorical, k_policy_cat<G>: a group of G lanes per robot (launch_plan.h: plan_policy_group), lane j owns the logits
// [j * per, min((j + 1) * per, A)), per = ceil(A / G); it keeps them in registers while per <= POL_REG and re-reads them beyond.
// Float32 throughout, no contraction.  The order of every operation is fixed, so two runs and tests/policy_model.py agree bit for
// bit given the same e[]:
//   m        the row's maximum (NaNs skipped): lane maximum, then an xor butterfly over the group -- exact in any order
//   bad      a NaN, a +inf, or m == -inf (no finite logit): actions (0, 0, 0), index -1, logp 0, entropy 0, counted in n_bad
//   e_k      = l_k == -inf ? 0 : expf(l_k - m)                 (a masked action; an e_k that underflows to 0 counts as masked)
//   part_j   = ((0 + e_k0) + e_k0+1) + ...                     the lane's block, ascending
//   P_j      inclusive scan of part over the group, Hillis-Steele: for d = 1, 2, 4, ... < G: P_j = j >= d ? P_j + P_(j-d) : P_j
//   s        = P_(G-1);  X_j = j ? P_(j-1) : 0;  target = u * s
//   c_k      = (...((X_j + e_k0) + e_k0+1) ...) + e_k           the inclusive cumulative sum, restarted from X_j in every lane
//   index    the smallest k with e_k > 0 and c_k > target; none (u * s rounded to s, or the lanes' restarts fell short): the
//            largest k with e_k > 0.  DETERMINISTIC: the smallest k with l_k == m.  A masked action is never chosen.
//   logp     = (l_index - m) - logf(s)
//   entropy  = 0 - H, H = the lanes' sums ((0 + t_k0) + ...) of t_k = (e_k / s) * ((l_k - m) - logf(s)) over e_k > 0, ascending,
//            folded by an xor butterfly: for d = 1, 2, 4, ... < G: H_j = H_j + H_(j ^ d) (commutative: every lane holds the same bits)
// then the table row of `index` and the masked speeds exactly as k_actions does it.  No LDS, no atomics but n_bad's.
//
// Gaussian, k_policy_gauss: one lane per robot, C = 2 or 3 independent normals.  sigma = expf(log_std); Box-Muller on the first
// block: u1 = float((x0 >> 8) + 1) * 2^-24 in (0, 1], u2 = float(x1 >> 8) * 2^-24, rho = sqrtf(-2 logf(u1)), z0 = rho cosf(2 pi u2),
// z1 = rho sinf(2 pi u2) (2 pi the float32 constant); column 2 takes z0 of the second block.  raw = mean + sigma z;
// logp = sum_c ((-0.5 z z - log_std) - 0.5 ln 2 pi) of the UNCLIPPED sample, entropy = sum_c ((0.5 + 0.5 ln 2 pi) + log_std), both
// ascending from 0; DETERMINISTIC: z = 0.  A mean, log_std, sigma or raw that is not finite makes the row bad (raw 0).  actions =
// k_actions' CLIP rule on raw.
//
// The per-lane rules compile as plain C++ as well (POL_HD), for tests/host/policy_check.cpp, which walks them over a simulated
// grid; the cross-lane folds and the kernels are HIP only.
#pragma once
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "launch_plan.h"  // POL_BLOCK, POL_REG, plan_policy_group, plan_policy_per_lane

#if defined(__HIPCC__)
#define POL_HD __host__ __device__ __forceinline__
#define POL_UNROLL _Pragma("unroll")
#else
#define POL_HD inline
#define POL_UNROLL
#endif

#define POL_TWO_PI 6.2831855f          // float32(2 pi)
#define POL_HALF_LN_2PI 0.9189385f     // float32(0.5 ln 2 pi)
#define POL_ENT_CONST 1.4189385f       // float32(0.5 + 0.5 ln 2 pi)

// ---- Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85)
POL_HD void pol_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
    POL_UNROLL
    for (int round = 0; round < 10; round++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// block `second` (0 | 1) of robot g's draw
POL_HD void pol_draw(uint64_t g, uint32_t draw_lo, uint32_t draw_hi, uint32_t seed_lo, uint32_t seed_hi, int second, uint32_t (&out)[4]) {
    pol_philox((uint32_t)g, (uint32_t)(g >> 32), draw_lo, second ? draw_hi ^ 0x80000000u : draw_hi, seed_lo, seed_hi, out);
}
POL_HD float pol_u01(uint32_t x) { return (float)(x >> 8) * 5.9604644775390625e-8f; }            // [0, 1), exact
POL_HD float pol_u01_open(uint32_t x) { return (float)((x >> 8) + 1u) * 5.9604644775390625e-8f; }  // (0, 1], exact

// ---- categorical: the lane's block and its three passes
// lane j of a group of G: logits [k0, k0 + n) of a row of A
POL_HD void pol_block(int A, int G, int j, int& k0, int& n) {
    const int per = (A + G - 1) / G;
    k0 = j * per;
    n = A - k0;
    n = n < 0 ? 0 : (n > per ? per : n);
}
// a lane's logits: in registers, padded with -inf (a masked action: never bad, never chosen, adds nothing) ...
struct PolRegs {
    float l[POL_REG];
    POL_HD float at(int i) const { return l[i]; }
    POL_HD float e(int i, float m) const { return l[i] == -INFINITY ? 0.0f : expf(l[i] - m); }
    POL_HD int count() const { return POL_REG; }
    POL_HD void load(const float* p, int n) {
        POL_UNROLL
        for (int i = 0; i < POL_REG; i++) l[i] = i < n ? p[i] : -INFINITY;
    }
};
// ... or re-read from the row in every pass
struct PolMem {
    const float* p;
    int n;
    POL_HD float at(int i) const { return p[i]; }
    POL_HD float e(int i, float m) const { return p[i] == -INFINITY ? 0.0f : expf(p[i] - m); }
    POL_HD int count() const { return n; }
};
// (a row type of the host check hands out given e[] instead: everything behind e_k is IEEE arithmetic in a fixed order)

template <class Row>
POL_HD void pol_lane_max(const Row& row, float& m, int& bad) {
    m = -INFINITY;
    bad = 0;
    POL_UNROLL
    for (int i = 0; i < row.count(); i++) {
        const float l = row.at(i);
        bad |= (l != l || l == INFINITY) ? 1 : 0;
        m = l > m ? l : m;  // (a NaN compares false: skipped)
    }
}
template <class Row>
POL_HD float pol_lane_sum(const Row& row, float m) {
    float part = 0.0f;
    POL_UNROLL
    for (int i = 0; i < row.count(); i++) part = part + row.e(i, m);
    return part;
}
struct PolLanePick {
    int cand;      // the lane's first hit, INT_MAX: none
    int last;      // the lane's largest k with e_k > 0, -1: none
    float l_cand, l_last;  // their logits
    float ent;     // the lane's sum of (e_k / s) * logp_k
};
template <class Row>
POL_HD PolLanePick pol_lane_pick(const Row& row, int k0, float m, float X, float s, float log_s, float target, bool det) {
    PolLanePick r = {INT_MAX, -1, 0.0f, 0.0f, 0.0f};
    float c = X;
    POL_UNROLL
    for (int i = 0; i < row.count(); i++) {
        const float l = row.at(i);
        const float e = row.e(i, m);
        if (e > 0.0f) {
            c = c + e;
            const bool hit = det ? l == m : c > target;
            if (hit && r.cand == INT_MAX) {
                r.cand = k0 + i;
                r.l_cand = l;
            }
            r.last = k0 + i;
            r.l_last = l;
            r.ent = r.ent + (e / s) * ((l - m) - log_s);
        }
    }
    return r;
}
POL_HD float pol_cat_logp(float l, float m, float log_s) { return (l - m) - log_s; }

// ---- Gaussian: one robot's row.  x: the first Philox block, y: the second (read only where C == 3)
struct PolGaussRow {
    float raw[3];
    float logp, entropy;
    bool bad;
};
POL_HD void pol_box_muller(uint32_t x0, uint32_t x1, float& z0, float& z1) {
    const float u1 = pol_u01_open(x0), u2 = pol_u01(x1);
    const float rho = sqrtf(-2.0f * logf(u1)), ang = POL_TWO_PI * u2;
    z0 = rho * cosf(ang);
    z1 = rho * sinf(ang);
}
POL_HD PolGaussRow pol_gauss_row(const float* mean, const float* log_std, int C, const uint32_t (&x)[4], const uint32_t (&y)[4], bool det) {
    PolGaussRow o;
    float z[3] = {0.0f, 0.0f, 0.0f}, unused = 0.0f;
    if (!det) {
        pol_box_muller(x[0], x[1], z[0], z[1]);
        if (C > 2) pol_box_muller(y[0], y[1], z[2], unused);
    }
    (void)unused;
    o.logp = 0.0f;
    o.entropy = 0.0f;
    o.bad = false;
    POL_UNROLL
    for (int c = 0; c < 3; c++) {
        o.raw[c] = 0.0f;
        if (c < C) {
            const float mu = mean[c], ls = log_std[c];
            const float sigma = expf(ls);
            const float raw = mu + sigma * z[c];
            o.bad = o.bad || !isfinite(mu) || !isfinite(ls) || !isfinite(sigma) || !isfinite(raw);
            o.raw[c] = raw;
            o.logp = o.logp + (((-0.5f * z[c]) * z[c] - ls) - POL_HALF_LN_2PI);
            o.entropy = o.entropy + (POL_ENT_CONST + ls);
        }
    }
    if (o.bad) {
        o.raw[0] = o.raw[1] = o.raw[2] = 0.0f;
        o.logp = o.entropy = 0.0f;
    }
    return o;
}
// k_actions' CLIP rule on one component
POL_HD float pol_clip(float f, float lo, float hi) {
    f = f >= lo ? f : lo;
    f = f <= hi ? f : hi;
    return f;
}

// what a launch takes, by value (the pointers of the slot are the host's arithmetic: the cursor is the host's, as for k_rollout)
struct PolicyDev {
    const float* params;         // [RL][A] logits | [RL][C] means, the caller's
    const float* log_std;        // [C] or [RL][C], the caller's
    const float* values;         // [RL] or null, the caller's
    const float* table;          // [A][3] (ActionsDev::table)
    float* actions;              // [RL][3] (ActionsDev)
    float* speeds;               // [RL][2]
    int32_t* n_bad;              // [1]
    const uint8_t* clean_state;  // [RL]
    int32_t* index;              // [RL] categorical
    float* raw;                  // [RL][C] Gaussian
    float* logp;                 // [RL]
    float* entropy;              // [RL]
    float* st_raw;               // the slot's row of column 0 of pol_raw, null: this call stores nothing
    float* st_logp;              // the slot's row of pol_logp
    float* st_value;             // the slot's row of pol_value
    size_t st_col;               // floats between two columns of pol_raw: T * RL
    unsigned long long g0;       // robot_begin
    float lo[3], hi[3];          // CLIP bounds
    uint32_t seed_lo, seed_hi, draw_lo, draw_hi;
    int32_t A, C, RL;
    int32_t det, ls_per_row;
};

#if defined(__HIPCC__)
// the row is written by ONE lane of its group; its wavefront counts it once
__device__ __forceinline__ void pol_count_bad(const PolicyDev& a, bool bad_row_here) {
    // (every lane of the wavefront is here: nothing above returns)
    const unsigned long long seen = __ballot(bad_row_here);
    if (seen != 0 && (threadIdx.x & (WAVE - 1)) == 0) atomicAdd(a.n_bad, (int)__popcll(seen));
}
__device__ __forceinline__ void pol_write_actions(const PolicyDev& a, int r, float v, float w, float beep) {
    float* out = a.actions + (size_t)r * 3;
    out[0] = v; out[1] = w; out[2] = beep;
    const bool clean = a.clean_state[r] != 0;
    a.speeds[(size_t)r * 2] = clean ? v : 0.0f;
    a.speeds[(size_t)r * 2 + 1] = clean ? w : 0.0f;
}

// the cross-lane folds of a group, in the order stated at the top: m and bad (xor butterfly), the lanes' sums and their
// Hillis-Steele scan; every lane of the group leaves with the row's m, bad and s and with its own X.  k_ploss_cat
// (policy_loss.h) calls the same two functions, which is what makes its log-probabilities the sampler's bit for bit.
template <int G, class Row>
__device__ __forceinline__ void pol_group_sums(const Row& row, int j, float& m, int& bad, float& X, float& s) {
    pol_lane_max(row, m, bad);
    if constexpr (G > 1) {
        POL_UNROLL
        for (int d = 1; d < G; d <<= 1) {
            const float y = __shfl_xor(m, d, G);
            m = y > m ? y : m;
            bad |= __shfl_xor(bad, d, G);
        }
    }
    bad |= m == -INFINITY ? 1 : 0;
    float P = pol_lane_sum(row, m);
    X = 0.0f;
    if constexpr (G > 1) {
        POL_UNROLL
        for (int d = 1; d < G; d <<= 1) {
            const float t = __shfl_up(P, d, G);
            P = j >= d ? P + t : P;
        }
        X = __shfl_up(P, 1, G);
        X = j ? X : 0.0f;
        P = __shfl(P, G - 1, G);
    }
    s = P;
}
// the entropy's xor butterfly over the lanes' sums
template <int G>
__device__ __forceinline__ float pol_group_entropy(float H) {
    if constexpr (G > 1) {
        POL_UNROLL
        for (int d = 1; d < G; d <<= 1) H = H + __shfl_xor(H, d, G);
    }
    return H;
}

template <int G, class Row>
__device__ __forceinline__ void pol_cat_group(const PolicyDev& a, const Row& row, int r, int j, int k0, bool live) {
    float m, X, P;
    int bad;
    pol_group_sums<G>(row, j, m, bad, X, P);
    const float s = P, log_s = logf(s);
    uint32_t x[4];
    pol_draw(a.g0 + (unsigned long long)r, a.draw_lo, a.draw_hi, a.seed_lo, a.seed_hi, 0, x);
    const float target = pol_u01(x[0]) * s;
    const PolLanePick pk = pol_lane_pick(row, k0, m, X, s, log_s, target, a.det != 0);
    int cand = pk.cand, last = pk.last;
    if constexpr (G > 1) {
        POL_UNROLL
        for (int d = 1; d < G; d <<= 1) {
            const int oc = __shfl_xor(cand, d, G), ol = __shfl_xor(last, d, G);
            cand = oc < cand ? oc : cand;
            last = ol > last ? ol : last;
        }
    }
    const float H = pol_group_entropy<G>(pk.ent);
    const bool found = cand != INT_MAX;
    const int idx = found ? cand : last;
    bad |= idx < 0 ? 1 : 0;  // (no e_k > 0 in a row with a finite maximum: expf(0) is 1, so this cannot be -- but the table is never read at -1)
    const bool owner = found ? pk.cand == cand : (last >= 0 && pk.last == last);
    const bool writer = live && (bad ? j == 0 : owner);
    if (writer) {
        float v = 0.0f, w = 0.0f, beep = 0.0f, logp = 0.0f, ent = 0.0f;
        int index = -1;
        if (!bad) {
            const float* t = a.table + (size_t)idx * 3;
            v = t[0]; w = t[1]; beep = t[2];
            logp = pol_cat_logp(found ? pk.l_cand : pk.l_last, m, log_s);
            ent = 0.0f - H;
            index = idx;
        }
        a.index[r] = index;
        a.logp[r] = logp;
        a.entropy[r] = ent;
        pol_write_actions(a, r, v, w, beep);
        if (a.st_raw) {
            a.st_raw[r] = (float)index;
            a.st_logp[r] = logp;
            if (a.values) a.st_value[r] = a.values[r];
        }
    }
    pol_count_bad(a, writer && bad);
}

template <int G>
__global__ __launch_bounds__(POL_BLOCK) void k_policy_cat(const PolicyDev a) {
    const unsigned lane = blockIdx.x * POL_BLOCK + threadIdx.x;
    const int r = (int)(lane / G), j = (int)(lane % G);
    const bool live = r < a.RL;
    int k0, n;
    pol_block(a.A, G, j, k0, n);
    if (!live) n = 0;  // (the lanes behind the last row walk empty blocks: the folds below run on whole wavefronts)
    const float* p = a.params + (size_t)(live ? r : 0) * (size_t)a.A + (size_t)(n > 0 ? k0 : 0);
    if (G < WAVE || a.A <= WAVE * POL_REG) {
        PolRegs row;
        row.load(p, n);
        pol_cat_group<G>(a, row, r, j, k0, live);
    } else {
        const PolMem row = {p, n};
        pol_cat_group<G>(a, row, r, j, k0, live);
    }
}

__global__ __launch_bounds__(POL_BLOCK) void k_policy_gauss(const PolicyDev a) {
    const int r = (int)(blockIdx.x * POL_BLOCK + threadIdx.x);
    const bool live = r < a.RL;
    bool bad = false;
    if (live) {
        uint32_t x[4], y[4] = {0u, 0u, 0u, 0u};
        const unsigned long long g = a.g0 + (unsigned long long)r;
        pol_draw(g, a.draw_lo, a.draw_hi, a.seed_lo, a.seed_hi, 0, x);
        if (a.C > 2) pol_draw(g, a.draw_lo, a.draw_hi, a.seed_lo, a.seed_hi, 1, y);
        const float* mean = a.params + (size_t)r * a.C;
        const float* ls = a.ls_per_row ? a.log_std + (size_t)r * a.C : a.log_std;
        const PolGaussRow o = pol_gauss_row(mean, ls, a.C, x, y, a.det != 0);
        bad = o.bad;
        float act[3] = {0.0f, 0.0f, 0.0f};
        POL_UNROLL
        for (int c = 0; c < 3; c++)
            if (c < a.C) {
                a.raw[(size_t)r * a.C + c] = o.raw[c];
                act[c] = bad ? 0.0f : pol_clip(o.raw[c], a.lo[c], a.hi[c]);
                if (a.st_raw) a.st_raw[(size_t)c * a.st_col + r] = o.raw[c];
            }
        a.logp[r] = o.logp;
        a.entropy[r] = o.entropy;
        pol_write_actions(a, r, act[0], act[1], act[2]);
        if (a.st_raw) {
            a.st_logp[r] = o.logp;
            if (a.values) a.st_value[r] = a.values[r];
        }
    }
    pol_count_bad(a, bad);
}

// IMGENV_POLICY_VALUE_ONLY: values -> the slot's row of pol_value
__global__ __launch_bounds__(POL_BLOCK) void k_policy_value(const PolicyDev a) {
    const int r = (int)(blockIdx.x * POL_BLOCK + threadIdx.x);
    if (r < a.RL) a.st_value[r] = a.values[r];
}
#endif
