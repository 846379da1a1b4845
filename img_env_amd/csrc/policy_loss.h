// policy_loss.h -- PPO's loss on the device (include/imgenv.h: imgenv_policy_loss): the log-probability of every STORED action and
// the entropy under the network's NEW outputs, the clipped surrogate, the (clipped) value loss, their weighted means and the
// gradients on the network's outputs, in three launches and no atomics:
//   1. k_ploss_cat<G> / k_ploss_gauss   the rows: logp, entropy, ratio, pg, vl [B]; one float64 record per workgroup
//   2. k_ploss_fold                     one wavefront folds the records: stats, n_bad, inv_W, the shared d_log_std
//   3. k_ploss_grad_cat<G> / _gauss     d_params [B][A | C], d_log_std [B][C], d_values [B]
// No workgroup waits for another: the launches are ordered by the stream.
//
// Categorical: the sampler's group of G = plan_policy_group(A) lanes per row, its partition (pol_block), its rows (PolRegs up to
// A = 1024, PolMem beyond) and its own functions for m, the lanes' sums, the scan, s (pol_group_sums), the lanes' entropy sums
// (pol_lane_pick) and their butterfly (pol_group_entropy): logp = pol_cat_logp(l_a, m, logf(s)) and entropy = 0 - H are, for
// unchanged logits, the bits the sampler stored.  Lane 0 of the group owns the row's terms.  The stored action a is a float32 (the
// ring's pol_raw): an integer in [0, A) whose logit is not -inf, or the row is bad.
// Gaussian: one lane per row; sigma = expf(log_std), z = (raw - mean) / sigma, logp = sum_c (((-0.5 z) z - log_std) - 0.5 ln 2 pi)
// and entropy = sum_c ((0.5 + 0.5 ln 2 pi) + log_std), ascending from 0 -- the sampler's expressions.  A mean, log_std, sigma, raw
// or z that is not finite makes the row bad.
//
// The row's terms (ploss_row_terms), float32, no contraction, in this order:
//   bad     |= old_logp, adv, ret, v, (old_v with CLIP_VALUE) or w not finite
//   d        = logp - old_logp;  r = expf(d);  bad |= r not finite
//   s1       = r * adv;  rc = min(max(r, 1 - clip), 1 + clip);  s2 = rc * adv;  active = s1 <= s2;  pg = 0 - (active ? s1 : s2)
//   dv       = v - ret;  q = dv * dv
//   CLIP_VALUE: dc = v - old_v;  vc = old_v + min(max(dc, -clip_vf), clip_vf);  dvc = vc - ret;  qc = dvc * dvc;  q = qc > q ? qc : q
//   vl       = 0.5 * q;  kl = (r - 1) - d;  clipped = |r - 1| > clip
//   gu       = w * (active ? (0 - adv) * r : 0)                   the unnormalised g_i
//   skip     = bad or w == 0: every output of the row is +0, its weight counts as 0; it is COUNTED bad where bad and w != 0
// The sums are float64.  A lane's contributions are exact products of two float32: w, w pg, w vl, w H, w kl, w clipped, the bad
// count, and (Gaussian) t_c = gu (z_c z_c - 1) + (0 - ent_coef) w for c < C.  Their order is fixed:
//   workgroup  an xor butterfly inside the wavefront (x = x + x[lane ^ d], d = 1, 2, ..., 32), then the four wavefronts ascending
//              through LDS ((w0 + w1) + w2) + w3: record[blockIdx]
//   fold       lane t of one wavefront adds records t, t + 64, ... ascending from 0, then the same butterfly
//   Wm = max(W, 1);  stats[k] = (float)(S_k / Wm), loss = ((S_pg + vf_coef S_vl) - ent_coef S_H) / Wm;  inv_W = (float)(1.0 / Wm);
//   d_log_std_shared[c] = (float)(S_tc / Wm)
// The gradients, float32: gw = w inv_W, g = gu inv_W, gH = (0 - ent_coef) gw (w, gu: 0 for a skipped row, whose gradients are +0)
//   categorical  lp_k = (l_k - m) - log_s;  p_k = expf(lp_k);  d_k = g ([k == a] - p_k) - gH (p_k (lp_k + entropy));  l_k == -inf: +0
//   Gaussian     d_mean_c = (g z_c) / sigma_c;  d_log_std_c = g (z_c z_c - 1) + gH
//   values       (vf_coef gw) term, term = dv, or with CLIP_VALUE where qc > q: |dc| <= clip_vf ? dvc : 0
// The handle owns one set of row arrays, records and inv_W: two imgenv_policy_loss calls of one handle must be ordered (one stream,
// or an event between them) -- on two streams at once they race.
// Everything but expf / logf is IEEE arithmetic: tests/policy_loss_model.py restates it bit for bit, and the per-lane rules compile
// as plain C++ (POL_HD) for tests/host/policy_loss_check.cpp.
#pragma once
#include "policy.h"  // POL_HD, pol_block, PolRegs / PolMem, pol_group_sums, pol_lane_pick, pol_group_entropy, pol_cat_logp, pol_clip

#define PLOSS_FOLD_BLOCK 64  // k_ploss_fold: one wavefront
// a workgroup's record: float64 [PLOSS_REC]
enum { PLOSS_W = 0, PLOSS_PG, PLOSS_VL, PLOSS_H, PLOSS_KL, PLOSS_CLIPPED, PLOSS_BAD, PLOSS_DLS, PLOSS_REC = PLOSS_DLS + 3 };

struct PlossRow {
    float ratio, pg, vl, kl, clipped;
    float gu;      // w * (active ? (0 - adv) * r : 0)
    bool bad;
};
POL_HD bool ploss_finite(float x) { return x - x == 0.0f; }
// (r given: everything behind expf is IEEE arithmetic in a fixed order, which the host check walks with the model's r)
POL_HD PlossRow ploss_row_terms_given(float logp, bool bad, float r, float old_logp, float adv, float ret, float v, float old_v, float w,
                                      float clip, float clip_vf, bool clip_value) {
    PlossRow o;
    bad = bad || !ploss_finite(old_logp) || !ploss_finite(adv) || !ploss_finite(ret) || !ploss_finite(v) || !ploss_finite(w);
    bad = bad || (clip_value && !ploss_finite(old_v));
    const float d = logp - old_logp;
    bad = bad || !ploss_finite(r);
    const float s1 = r * adv;
    const float rc = pol_clip(r, 1.0f - clip, 1.0f + clip);
    const float s2 = rc * adv;
    const bool active = s1 <= s2;
    o.pg = 0.0f - (active ? s1 : s2);
    const float dv = v - ret;
    float q = dv * dv;
    if (clip_value) {
        const float dc = v - old_v;
        const float vc = old_v + pol_clip(dc, 0.0f - clip_vf, clip_vf);
        const float dvc = vc - ret;
        const float qc = dvc * dvc;
        q = qc > q ? qc : q;
    }
    o.vl = 0.5f * q;
    o.kl = (r - 1.0f) - d;
    o.clipped = fabsf(r - 1.0f) > clip ? 1.0f : 0.0f;
    o.gu = w * (active ? (0.0f - adv) * r : 0.0f);
    o.ratio = r;
    o.bad = bad;
    return o;
}
POL_HD PlossRow ploss_row_terms(float logp, bool bad, float old_logp, float adv, float ret, float v, float old_v, float w, float clip,
                                float clip_vf, bool clip_value) {
    return ploss_row_terms_given(logp, bad, expf(logp - old_logp), old_logp, adv, ret, v, old_v, w, clip, clip_vf, clip_value);
}
// d values[i] over (vf_coef gw)
POL_HD float ploss_value_term(float v, float ret, float old_v, float clip_vf, bool clip_value) {
    const float dv = v - ret;
    if (!clip_value) return dv;
    const float dc = v - old_v;
    const float vc = old_v + pol_clip(dc, 0.0f - clip_vf, clip_vf);
    const float dvc = vc - ret;
    if (dvc * dvc > dv * dv) return fabsf(dc) <= clip_vf ? dvc : 0.0f;
    return dv;
}
POL_HD float ploss_value_grad(float vf_coef, float gw, float term) { return (vf_coef * gw) * term; }
POL_HD float ploss_cat_grad(float l, float m, float log_s, float entropy, float g, float gH, bool hit) {
    const float lp = (l - m) - log_s;
    const float p = expf(lp);
    return g * ((hit ? 1.0f : 0.0f) - p) - gH * (p * (lp + entropy));
}
// the Gaussian head's gradients for given z and sigma, and the term the row launch adds up for a shared log_std
POL_HD float ploss_gauss_grad_mean(float g, float z, float sigma) { return (g * z) / sigma; }
POL_HD float ploss_gauss_grad_ls(float g, float z, float gH) { return g * (z * z - 1.0f) + gH; }
POL_HD float ploss_gauss_dls_term(float gu, float z, float w, float ent_coef) { return gu * (z * z - 1.0f) + (0.0f - ent_coef) * w; }
// the stored index: an integer in [0, A), or -1
POL_HD int ploss_action_index(float af, int A) { return (af >= 0.0f && af < (float)A && af == floorf(af)) ? (int)af : -1; }

struct PlossGauss {
    float z[3], sigma[3];
    float logp, entropy;
    bool bad;
};
POL_HD PlossGauss ploss_gauss_row(const float* mean, const float* log_std, const float (&raw)[3], int C) {
    PlossGauss o;
    o.logp = 0.0f;
    o.entropy = 0.0f;
    o.bad = false;
    POL_UNROLL
    for (int c = 0; c < 3; c++) {
        o.z[c] = 0.0f;
        o.sigma[c] = 1.0f;
        if (c < C) {
            const float mu = mean[c], ls = log_std[c];
            const float sigma = expf(ls);
            const float z = (raw[c] - mu) / sigma;
            o.bad = o.bad || !ploss_finite(mu) || !ploss_finite(ls) || !ploss_finite(sigma) || !ploss_finite(raw[c]) || !ploss_finite(z);
            o.z[c] = z;
            o.sigma[c] = sigma;
            o.logp = o.logp + (((-0.5f * z) * z - ls) - POL_HALF_LN_2PI);
            o.entropy = o.entropy + (POL_ENT_CONST + ls);
        }
    }
    return o;
}
// the final fold's last step: what k_ploss_fold's lane 0 writes from the sums S
struct PlossTotals {
    float stats[8];
    float inv_W;
    float dls[3];
    int32_t n_bad;
};
POL_HD PlossTotals ploss_totals(const double (&S)[PLOSS_REC], float vf_coef, float ent_coef) {
    PlossTotals o;
    const double Wm = S[PLOSS_W] > 1.0 ? S[PLOSS_W] : 1.0;
    o.stats[0] = (float)(((S[PLOSS_PG] + (double)vf_coef * S[PLOSS_VL]) - (double)ent_coef * S[PLOSS_H]) / Wm);
    o.stats[1] = (float)(S[PLOSS_PG] / Wm);
    o.stats[2] = (float)(S[PLOSS_VL] / Wm);
    o.stats[3] = (float)(S[PLOSS_H] / Wm);
    o.stats[4] = (float)(S[PLOSS_KL] / Wm);
    o.stats[5] = (float)(S[PLOSS_CLIPPED] / Wm);
    o.stats[6] = (float)S[PLOSS_W];
    o.stats[7] = 0.0f;
    o.inv_W = (float)(1.0 / Wm);
    POL_UNROLL
    for (int c = 0; c < 3; c++) o.dls[c] = (float)(S[PLOSS_DLS + c] / Wm);
    o.n_bad = (int32_t)S[PLOSS_BAD];
    return o;
}

// what the three launches take, by value
struct PlossDev {
    const float* params;      // [B][A] logits | [B][C] means, the caller's
    const float* log_std;     // [C] or [B][C]
    const float* values;      // [B]
    const float* action[3];   // [B] each
    const float* old_logp;    // [B]
    const float* old_value;   // [B], read only with clip_value
    const float* adv;
    const float* ret;
    const float* weight;
    float* logp;              // [B] row outputs
    float* entropy;
    float* ratio;
    float* pg;
    float* vl;
    float* row_m;             // [B] for the third launch: m, log_s (categorical), gu and the weight that counts (0: skipped)
    float* row_log_s;
    float* row_gu;
    float* row_w;
    double* rec;              // [n_rec][PLOSS_REC]
    float* d_params;          // [B][A | C]
    float* d_log_std;         // [B][C]
    float* d_log_std_shared;  // [C]
    float* d_values;          // [B]
    float* stats;             // [8]
    float* inv_W;             // [1]
    int32_t* n_bad;           // [1]
    float clip, clip_vf, vf_coef, ent_coef;
    int32_t A, C, B, n_rec;
    int32_t clip_value, ls_per_row;
};

// one row's terms to its [B] arrays and to the owner lane's contributions
POL_HD void ploss_contribute(const PlossRow& t, float entropy, float w, bool skip, double (&acc)[PLOSS_REC]) {
    // (selects, not branches: a skipped row's terms may be NaN, and no entry of acc is ever addressed dynamically)
    const double wd = (double)w;
    acc[PLOSS_W] = skip ? 0.0 : wd;
    acc[PLOSS_PG] = skip ? 0.0 : wd * (double)t.pg;
    acc[PLOSS_VL] = skip ? 0.0 : wd * (double)t.vl;
    acc[PLOSS_H] = skip ? 0.0 : wd * (double)entropy;
    acc[PLOSS_KL] = skip ? 0.0 : wd * (double)t.kl;
    acc[PLOSS_CLIPPED] = skip ? 0.0 : wd * (double)t.clipped;
    acc[PLOSS_BAD] = (t.bad && w != 0.0f) ? 1.0 : 0.0;
}

#if defined(__HIPCC__)
__device__ __forceinline__ void ploss_write_row(const PlossDev& a, int r, const PlossRow& t, float logp, float entropy, float w, bool skip) {
    a.logp[r] = skip ? 0.0f : logp;
    a.entropy[r] = skip ? 0.0f : entropy;
    a.ratio[r] = skip ? 0.0f : t.ratio;
    a.pg[r] = skip ? 0.0f : t.pg;
    a.vl[r] = skip ? 0.0f : t.vl;
    a.row_gu[r] = skip ? 0.0f : t.gu;
    a.row_w[r] = skip ? 0.0f : w;
}
// every lane of the workgroup is here (nothing above returns); lds: [POL_BLOCK / WAVE][PLOSS_REC]
__device__ __forceinline__ void ploss_block_fold(const PlossDev& a, double (&acc)[PLOSS_REC], double (*lds)[PLOSS_REC]) {
    POL_UNROLL
    for (int k = 0; k < PLOSS_REC; k++) {
        POL_UNROLL
        for (int d = 1; d < WAVE; d <<= 1) acc[k] = acc[k] + __shfl_xor(acc[k], d, WAVE);
    }
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    if (lane == 0) {
        POL_UNROLL
        for (int k = 0; k < PLOSS_REC; k++) lds[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < PLOSS_REC) {
        double t = lds[0][threadIdx.x];
        for (int w = 1; w < POL_BLOCK / WAVE; w++) t = t + lds[w][threadIdx.x];
        a.rec[(size_t)blockIdx.x * PLOSS_REC + threadIdx.x] = t;
    }
}

template <int G, class Row>
__device__ __forceinline__ void ploss_cat_group(const PlossDev& a, const Row& row, int r, int j, int k0, bool live, double (&acc)[PLOSS_REC]) {
    float m, X, s;
    int bad;
    pol_group_sums<G>(row, j, m, bad, X, s);
    const float log_s = logf(s);
    const PolLanePick pk = pol_lane_pick(row, k0, m, X, s, log_s, 0.0f, true);  // (its entropy sum; the pick is not used)
    const float H = pol_group_entropy<G>(pk.ent);
    if (live && j == 0) {
        const int ai = ploss_action_index(a.action[0][r], a.A);
        const float l_a = a.params[(size_t)r * (size_t)a.A + (size_t)(ai < 0 ? 0 : ai)];
        const bool bad_row = bad != 0 || ai < 0 || l_a == -INFINITY;
        const float logp = pol_cat_logp(l_a, m, log_s), entropy = 0.0f - H, w = a.weight[r];
        const PlossRow t = ploss_row_terms(logp, bad_row, a.old_logp[r], a.adv[r], a.ret[r], a.values[r], a.clip_value ? a.old_value[r] : 0.0f, w,
                                           a.clip, a.clip_vf, a.clip_value != 0);
        const bool skip = t.bad || w == 0.0f;
        ploss_write_row(a, r, t, logp, entropy, w, skip);
        a.row_m[r] = m;
        a.row_log_s[r] = log_s;
        ploss_contribute(t, entropy, w, skip, acc);
    }
}

template <int G>
__global__ __launch_bounds__(POL_BLOCK) void k_ploss_cat(const PlossDev a) {
    __shared__ double lds[POL_BLOCK / WAVE][PLOSS_REC];
    const unsigned lane = blockIdx.x * POL_BLOCK + threadIdx.x;
    const int r = (int)(lane / G), j = (int)(lane % G);
    const bool live = r < a.B;
    int k0, n;
    pol_block(a.A, G, j, k0, n);
    if (!live) n = 0;  // (the lanes behind the last row walk empty blocks: the folds run on whole wavefronts)
    const float* p = a.params + (size_t)(live ? r : 0) * (size_t)a.A + (size_t)(n > 0 ? k0 : 0);
    double acc[PLOSS_REC];
    POL_UNROLL
    for (int k = 0; k < PLOSS_REC; k++) acc[k] = 0.0;
    if (G < WAVE || a.A <= WAVE * POL_REG) {
        PolRegs row;
        row.load(p, n);
        ploss_cat_group<G>(a, row, r, j, k0, live, acc);
    } else {
        const PolMem row = {p, n};
        ploss_cat_group<G>(a, row, r, j, k0, live, acc);
    }
    ploss_block_fold(a, acc, lds);
}

__device__ __forceinline__ PlossGauss ploss_gauss_load(const PlossDev& a, int r) {
    float raw[3] = {0.0f, 0.0f, 0.0f};
    POL_UNROLL
    for (int c = 0; c < 3; c++)
        if (c < a.C) raw[c] = a.action[c][r];
    return ploss_gauss_row(a.params + (size_t)r * a.C, a.ls_per_row ? a.log_std + (size_t)r * a.C : a.log_std, raw, a.C);
}

__global__ __launch_bounds__(POL_BLOCK) void k_ploss_gauss(const PlossDev a) {
    __shared__ double lds[POL_BLOCK / WAVE][PLOSS_REC];
    const int r = (int)(blockIdx.x * POL_BLOCK + threadIdx.x);
    double acc[PLOSS_REC];
    POL_UNROLL
    for (int k = 0; k < PLOSS_REC; k++) acc[k] = 0.0;
    if (r < a.B) {
        const PlossGauss g = ploss_gauss_load(a, r);
        const float w = a.weight[r];
        const PlossRow t = ploss_row_terms(g.logp, g.bad, a.old_logp[r], a.adv[r], a.ret[r], a.values[r], a.clip_value ? a.old_value[r] : 0.0f, w,
                                           a.clip, a.clip_vf, a.clip_value != 0);
        const bool skip = t.bad || w == 0.0f;
        ploss_write_row(a, r, t, g.logp, g.entropy, w, skip);
        ploss_contribute(t, g.entropy, w, skip, acc);
        POL_UNROLL
        for (int c = 0; c < 3; c++) acc[PLOSS_DLS + c] = (skip || c >= a.C) ? 0.0 : (double)ploss_gauss_dls_term(t.gu, g.z[c], w, a.ent_coef);
    }
    ploss_block_fold(a, acc, lds);
}

__global__ __launch_bounds__(PLOSS_FOLD_BLOCK) void k_ploss_fold(const PlossDev a) {
    double acc[PLOSS_REC];
    POL_UNROLL
    for (int k = 0; k < PLOSS_REC; k++) acc[k] = 0.0;
    for (int q = (int)threadIdx.x; q < a.n_rec; q += PLOSS_FOLD_BLOCK) {
        const double* rec = a.rec + (size_t)q * PLOSS_REC;
        POL_UNROLL
        for (int k = 0; k < PLOSS_REC; k++) acc[k] = acc[k] + rec[k];
    }
    POL_UNROLL
    for (int k = 0; k < PLOSS_REC; k++) {
        POL_UNROLL
        for (int d = 1; d < WAVE; d <<= 1) acc[k] = acc[k] + __shfl_xor(acc[k], d, WAVE);
    }
    if (threadIdx.x == 0) {
        const PlossTotals o = ploss_totals(acc, a.vf_coef, a.ent_coef);
        POL_UNROLL
        for (int k = 0; k < 8; k++) a.stats[k] = o.stats[k];
        a.inv_W[0] = o.inv_W;
        a.n_bad[0] = o.n_bad;
        POL_UNROLL
        for (int c = 0; c < 3; c++)
            if (c < a.C) a.d_log_std_shared[c] = o.dls[c];
    }
}

__device__ __forceinline__ float ploss_row_value_grad(const PlossDev& a, int r, float gw, bool skip) {
    if (skip) return 0.0f;
    const float term = ploss_value_term(a.values[r], a.ret[r], a.clip_value ? a.old_value[r] : 0.0f, a.clip_vf, a.clip_value != 0);
    return ploss_value_grad(a.vf_coef, gw, term);
}

template <int G>
__global__ __launch_bounds__(POL_BLOCK) void k_ploss_grad_cat(const PlossDev a) {
    const unsigned lane = blockIdx.x * POL_BLOCK + threadIdx.x;
    const int r = (int)(lane / G), j = (int)(lane % G);
    if (r >= a.B) return;
    int k0, n;
    pol_block(a.A, G, j, k0, n);
    const float w = a.row_w[r], inv_W = a.inv_W[0];
    const bool skip = w == 0.0f;
    const float gw = w * inv_W, g = a.row_gu[r] * inv_W, gH = (0.0f - a.ent_coef) * gw;
    const float m = a.row_m[r], log_s = a.row_log_s[r], entropy = a.entropy[r];
    const int ai = skip ? -1 : ploss_action_index(a.action[0][r], a.A);
    const float* p = a.params + (size_t)r * (size_t)a.A;
    float* out = a.d_params + (size_t)r * (size_t)a.A;
    for (int i = 0; i < n; i++) {
        const int k = k0 + i;
        const float l = p[k];
        out[k] = (skip || l == -INFINITY) ? 0.0f : ploss_cat_grad(l, m, log_s, entropy, g, gH, k == ai);
    }
    if (j == 0) a.d_values[r] = ploss_row_value_grad(a, r, gw, skip);
}

__global__ __launch_bounds__(POL_BLOCK) void k_ploss_grad_gauss(const PlossDev a) {
    const int r = (int)(blockIdx.x * POL_BLOCK + threadIdx.x);
    if (r >= a.B) return;
    const float w = a.row_w[r], inv_W = a.inv_W[0];
    const bool skip = w == 0.0f;
    const float gw = w * inv_W, g = a.row_gu[r] * inv_W, gH = (0.0f - a.ent_coef) * gw;
    const PlossGauss q = ploss_gauss_load(a, r);
    POL_UNROLL
    for (int c = 0; c < 3; c++)
        if (c < a.C) {
            a.d_params[(size_t)r * a.C + c] = skip ? 0.0f : ploss_gauss_grad_mean(g, q.z[c], q.sigma[c]);
            a.d_log_std[(size_t)r * a.C + c] = skip ? 0.0f : ploss_gauss_grad_ls(g, q.z[c], gH);
        }
    a.d_values[r] = ploss_row_value_grad(a, r, gw, skip);
}
#endif
