"""PPO's loss on the device (imgenv_policy_loss, csrc/policy_loss.h) against tests/policy_loss_model.py.

Bounds, with eps = 2^-21 ("2^-21 relative per float32 operation"), margin = (A + 8) 2^-23 and the float64 truth's values:
  logp      b_lp = 2^-22 (1 + |logp|) + margin                     (test_gpu_policy.py's)
  entropy   b_H  = 2^-22 (1 + H) + margin (1 + ln A)
  ratio     d = logp - old_logp: b_d = b_lp + eps |d|;  r = expf(d): b_r = r (b_d + eps)
  pg        the branch the truth is on -- r adv: |adv| b_r + eps |pg|;  clamp(r) adv: |adv| eps rc + eps |pg|  (1 +- clip is one operation, the product one)
  d_values  = vf_coef (w / W) term: vf_coef (w / W) eps (|dv| + |dc| + |vc| + |dvc|) + 4 eps |d_values|
  vl        e_dv = eps |dv|, b_q = 2 |dv| e_dv + eps q;  e_dvc = eps (|dc| + |vc| + |dvc|), b_qc = 2 |dvc| e_dvc + eps qc;
            b_vl = 0.5 max(b_q, b_qc) + eps vl
  g         = (w / W) (-adv r): b_g = (w / W) |adv| b_r + 4 eps |g|                      ((0 - adv) r, w ., . inv_W, inv_W's rounding)
  d_logits  p_k = expf(lp_k): b_p = p_k (b_lpk + eps);  t = lp_k + H: b_t = b_lpk + b_H + eps |t|;
            d_k = g ([k == a] - p_k) - gH p_k t:
            b = b_g |hit - p| + |g| (b_p + eps |hit - p|) + eps |g (hit - p)| + |gH| (b_p |t| + p b_t) + 4 eps |gH p t| + eps |d_k|
  Gaussian  e_z = 3 eps |z| (the subtraction, expf and the division);  b_lp = sum_c |z_c| e_zc + 2 eps sum_c (z_c^2 + |log_std_c| + 1);
            b_H = eps entropy_scale;  d_mean = g z / sigma: b_g |z| / sigma + |g| e_z / sigma + 3 eps |d|;
            d_log_std = g (z^2 - 1) + gH: b_g |z^2 - 1| + |g| (2 |z| e_z + eps (z^2 + 1)) + eps |g (z^2 - 1)| + 2 eps |gH| + eps |d|;
            the shared one: the rows' bounds added up, plus B 2^-50 of the magnitudes and eps of the result
Rows whose float64 ratio lies within b_r of 1 +- clip are left out of the comparisons that depend on the surrogate's branch, rows
whose two value terms lie within b_q + b_qc of each other out of those that depend on the value branch; at most 2 % of a case's
rows.  Everything that is IEEE arithmetic given the device's own logp, entropy and ratio -- pg, vl, the value gradient, the
records' folds, stats, inv_W, n_bad -- is compared bit for bit with the float32 / float64 model, for both heads (the Gaussian's
three sums for a shared log_std excepted: they hang on the platform's expf through z).  stats is also held to the truth: the rows'
bounds weighted and added up, the clip fraction up to the edge rows' weight, plus 2^-23 of the result; kl = (r - 1) - d has
b_r + b_d + eps (|r - 1| + |d|)."""
import copy

import numpy as np
import pytest

import policy_loss_model as plm
import policy_model as pm
from scenarios import small_world
from stack_model import bits
from test_gpu_episodes import episode_cfg

pytestmark = pytest.mark.gpu
F32 = np.float32
EPS = 2.0 ** -21
TABLE8 = [[0.0, -0.9], [0.0, 0.3], [0.2, -0.6], [0.2, 0.0], [0.4, 0.6], [0.6, -0.3], [0.6, 0.0, 1], [0.6, 0.9]]
CLIP3 = [[0, 0.6], [-0.9, 0.9], [-0.6, 0.6]]
ROWS = (1, 63, 65, 257)
WIDTHS = (1, 2, 3, 16, 17, 64, 65, 257, 1025)
SCALES = (0.0, 1.0, 8.0)
SIGMAS = (0.0, 0.05, 0.5)
MAX_ROWS = 257
CLIP, CLIP_VF, VF, ENT = 0.2, 0.2, 0.5, 0.01
ROW_KEYS = ("logp", "entropy", "ratio", "pg", "vl", "d_values", "d_params")
_worlds = {}


def tiny_world(R):
    if R not in _worlds:
        _worlds[R] = small_world(R, 0, seed=11, grid_size=480, clearance=0.7)
    return _worlds[R]


def table_of(A):
    rng = np.random.default_rng(A)
    return np.stack([rng.uniform(0, 0.6, A), rng.uniform(-0.9, 0.9, A), rng.integers(0, 2, A)], axis=1).astype(F32).tolist()


def categorical_world(A, R=1, max_rows=MAX_ROWS):
    from img_env_amd.world import World
    grid, params, layout = tiny_world(R)
    w = World(params, grid)
    w.enable_actions(discrete_actions=table_of(A), act_dim=3)
    w.enable_policy("categorical", 7)
    w.enable_policy_loss(max_rows)
    w.reset(layout)
    return w


def gaussian_world(C, max_rows=MAX_ROWS):
    from img_env_amd.world import World
    grid, params, layout = tiny_world(1)
    w = World(params, grid)
    w.enable_actions(continuous_actions=CLIP3, act_dim=C)
    w.enable_policy("gaussian", 7)
    w.enable_policy_loss(max_rows)
    w.reset(layout)
    return w


def same(got, want, where):
    g, w = np.asarray(got), np.asarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (where, g.dtype, w.dtype, g.shape, w.shape)
    eq = (g == w) if g.dtype.itemsize == 1 else (bits(g) == bits(w))
    assert eq.all(), "%s differs at %s (%d of %d)" % (where, np.argwhere(~eq)[0].tolist(), (~eq).sum(), eq.size)


def run_cat(w, c, clip_vf=CLIP_VF, ent_coef=ENT, **over):
    """one call on a case of plm.make_case; every output on the host"""
    import torch
    c = dict(c, **over)
    out = w.policy_loss(c["logits"], c["values"], c["action"], c["old_logp"], c["adv"], c["ret"], c["weight"], old_value=c["old_value"],
                        clip=CLIP, clip_vf=clip_vf, vf_coef=VF, ent_coef=ent_coef)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy().copy() for k, t in out.items()}


def cat_truth(c, clip_vf=CLIP_VF, ent_coef=ENT):
    return plm.truth(c["logits"], c["action"], c["old_logp"], c["adv"], c["ret"], c["values"], c["weight"], old_value=c["old_value"],
                     clip=CLIP, clip_vf=clip_vf, vf_coef=VF, ent_coef=ent_coef)


def ratio_bounds(ref, b_lp, old_logp):
    d = ref["logp"] - old_logp.astype(np.float64)
    b_d = b_lp + EPS * np.abs(d)
    return b_d, ref["ratio"] * (b_d + EPS)


def surrogate_edge(ref, b_r):
    clip = float(F32(CLIP))
    r = ref["ratio"]
    return ~ref["skip"] & ((np.abs(r - (1 - clip)) <= b_r + EPS) | (np.abs(r - (1 + clip)) <= b_r + EPS))


def value_bounds(c, ref, clip_vf):
    v, ret, old_v = (c[k].astype(np.float64) for k in ("values", "ret", "old_value"))
    dv = v - ret
    q = dv * dv
    b_q = 2 * np.abs(dv) * EPS * np.abs(dv) + EPS * q
    if clip_vf is None:
        return 0.5 * b_q + EPS * ref["vl"], np.zeros(len(v), bool), EPS * np.abs(dv)
    cvf = float(F32(clip_vf))
    dc = v - old_v
    vc = old_v + np.clip(dc, -cvf, cvf)
    dvc = vc - ret
    qc = dvc * dvc
    b_qc = 2 * np.abs(dvc) * EPS * (np.abs(dc) + np.abs(vc) + np.abs(dvc)) + EPS * qc
    # (inside the clip range vc is v and both branches are one; at its edge the gradient jumps, beyond it the two squares compete)
    near = np.abs(np.abs(dc) - cvf) <= EPS * (np.abs(dc) + cvf)
    edge = ~ref["skip"] & (near | ((np.abs(dc) > cvf) & (np.abs(q - qc) <= b_q + b_qc)))
    return 0.5 * np.maximum(b_q, b_qc) + EPS * np.abs(ref["vl"]), edge, EPS * (np.abs(dv) + np.abs(dc) + np.abs(vc) + np.abs(dvc))


def check_ieee_parts(got, c, bad, clip_vf, ent_coef, G, where):
    """everything behind the device's own logp, entropy and ratio, bit for bit: pg, vl, the folds' first seven sums and with them
    stats, inv_W and n_bad, and d_values.  `bad`: the float64 truth's bad rows (what the parameters and the stored action say)"""
    t = plm.row_terms_f32(got["logp"], bad, c["old_logp"], c["adv"], c["ret"], c["values"], c["weight"], old_v=c["old_value"], clip=CLIP,
                          clip_vf=clip_vf, r=got["ratio"])
    z0 = lambda x: np.where(t["skip"], F32(0), x).astype(F32)  # noqa: E731
    same(got["pg"], z0(t["pg"]), where + " pg")
    same(got["vl"], z0(t["vl"]), where + " vl")
    contrib = plm.contributions(t, got["entropy"], c["weight"])
    tot = plm.totals(plm.fold_final(plm.fold_records(contrib, G)), VF, ent_coef)
    same(got["stats"], tot["stats"], where + " stats")
    same(got["inv_w"], np.array([tot["inv_W"]], F32), where + " inv_w")
    assert int(got["n_bad"][0]) == tot["n_bad"], where
    gw, g, gH = plm.scales(t, c["weight"], got["inv_w"][0], ent_coef)
    same(got["d_values"], plm.value_grad_f32(t, gw, VF), where + " d_values")
    # stats and inv_W once more, order-free: the plain float64 fold of the device's row outputs, B 2^-50 of the magnitudes, then float32
    B, W = len(c["weight"]), max(contrib[:, plm.W_].sum(), 1.0)
    vf, ec = float(F32(VF)), float(F32(ent_coef))
    plain, mag = contrib.sum(axis=0), np.abs(contrib).sum(axis=0)
    want = [(plain[plm.PG] + vf * plain[plm.VL] - ec * plain[plm.H_]) / W] + [plain[k] / W for k in (plm.PG, plm.VL, plm.H_, plm.KL, plm.CLIPPED)]
    mags = [(mag[plm.PG] + vf * mag[plm.VL] + ec * mag[plm.H_]) / W] + [mag[k] / W for k in (plm.PG, plm.VL, plm.H_, plm.KL, plm.CLIPPED)]
    for k in range(6):
        assert abs(float(got["stats"][k]) - want[k]) <= B * 2.0 ** -50 * mags[k] + 2.0 ** -24 * abs(want[k]), (where, k)
    assert abs(float(got["inv_w"][0]) - 1.0 / W) <= 2.0 ** -24 / W and got["stats"][6] == F32(plain[plm.W_]) and got["stats"][7] == 0
    return t, g, gH


def check_stats_against_truth(got, ref, c, b_r, b_d, b_H, b_vl, edge, ent_coef, where):
    """stats against the float64 truth: the rows' bounds, weighted and added up (pg and vl are continuous across their branch
    edges, so an edge row keeps its bound; the clip fraction may differ by the edge rows' weight), plus the float32 rounding of the
    result.  Returns the worst measured / bound."""
    we, W = ref["we"], ref["W"]
    adv = np.abs(c["adv"].astype(np.float64))
    d = ref["logp"] - np.where(ref["skip"], 0.0, c["old_logp"].astype(np.float64))
    b_pg = adv * b_r + EPS * np.abs(ref["pg"])
    b_kl = b_r + b_d + EPS * (np.abs(ref["ratio"] - 1) + np.abs(d))
    mean = lambda b: float((we * np.where(ref["skip"], 0.0, b)).sum() / W)  # noqa: E731
    b = [0.0, mean(b_pg), mean(b_vl), mean(b_H), mean(b_kl), float(we[edge].sum() / W)]
    b[0] = b[1] + float(F32(VF)) * b[2] + float(F32(ent_coef)) * b[3]
    worst = 0.0
    for k in range(6):
        bound = b[k] + 2.0 ** -23 * abs(ref["stats"][k]) + 1e-300
        frac = abs(float(got["stats"][k]) - ref["stats"][k]) / bound
        assert frac <= 1 or abs(float(got["stats"][k]) - ref["stats"][k]) == 0, (where, k, float(got["stats"][k]), ref["stats"][k], bound)
        worst = max(worst, frac if bound > 1e-290 else 0.0)
    assert float(got["stats"][6]) == ref["stats"][6] and got["stats"][7] == 0, where
    assert abs(float(got["inv_w"][0]) - ref["inv_W"]) <= 2.0 ** -24 * ref["inv_W"], where
    return worst


# ---- 1. categorical rows and gradients against the float64 truth; the IEEE parts bit for bit ----
@pytest.mark.parametrize("B", ROWS)
def test_categorical_against_the_truth(B):
    worst = dict(logp=0.0, entropy=0.0, ratio=0.0, pg=0.0, vl=0.0, d_params=0.0, d_values=0.0, stats=0.0)
    left_out = 0
    rng = np.random.default_rng(B)
    rows = np.arange(B)
    for A in WIDTHS:
        w = categorical_world(A)
        try:
            mg, G = pm.margin(A), pm.group(A)
            for q, (scale, sigma) in enumerate((s, g) for s in SCALES for g in SIGMAS):
                clip_vf = CLIP_VF if q % 2 == 0 else None
                c = plm.make_case(rng, B, A, scale, sigma)
                got, ref = run_cat(w, c, clip_vf), cat_truth(c, clip_vf)
                where = "B %d A %d scale %g sigma %g" % (B, A, scale, sigma)
                assert int(got["n_bad"][0]) == 0 and not ref["bad"].any(), where
                skip, keep = ref["skip"], ~ref["skip"]
                for k in ROW_KEYS:  # rows of weight 0: all-zero bits
                    assert (bits(got[k][skip]) == 0).all(), (where, k)
                b_lp = 2.0 ** -22 * (1 + np.abs(ref["logp"])) + mg
                b_H = 2.0 ** -22 * (1 + ref["entropy"]) + mg * (1 + np.log(A))
                b_d, b_r = ratio_bounds(ref, b_lp, c["old_logp"])
                edge = surrogate_edge(ref, b_r)
                b_vl, v_edge, e_term = value_bounds(c, ref, clip_vf)
                assert edge.sum() + v_edge.sum() <= 0.02 * B, (where, edge.sum(), v_edge.sum())
                left_out += int(edge.sum() + v_edge.sum())
                clip = float(F32(CLIP))
                rc = np.clip(ref["ratio"], 1 - clip, 1 + clip)
                adv = np.abs(c["adv"].astype(np.float64))
                b_pg = np.where(ref["active"], adv * b_r, adv * EPS * rc) + EPS * np.abs(ref["pg"])
                e = dict(logp=np.abs(got["logp"] - ref["logp"]) / b_lp, entropy=np.abs(got["entropy"] - ref["entropy"]) / b_H,
                         ratio=np.abs(got["ratio"] - ref["ratio"]) / np.maximum(b_r, 1e-300),
                         pg=np.where(edge, 0, np.abs(got["pg"] - ref["pg"]) / np.maximum(b_pg, 1e-300)),
                         vl=np.where(v_edge, 0, np.abs(got["vl"] - ref["vl"]) / np.maximum(b_vl, 1e-300)))
                # the gradients
                Wt = ref["W"]
                b_g = ref["we"] / Wt * adv * b_r + 4 * EPS * np.abs(ref["g"])
                truth_all = pm.categorical_truth(c["logits"])
                with np.errstate(invalid="ignore", over="ignore"):
                    p = truth_all["p"]
                    lp_all = np.where(p > 0, truth_all["logp"], 0.0)
                    b_lpk = 2.0 ** -22 * (1 + np.abs(lp_all)) + mg
                    b_p = p * (b_lpk + EPS)
                    t = lp_all + ref["entropy"][:, None]
                    b_t = b_lpk + b_H[:, None] + EPS * np.abs(t)
                    hit = (np.arange(A)[None, :] == c["action"].astype(np.int64)[:, None]).astype(np.float64)
                    g, gH = ref["g"][:, None], ref["gH"][:, None]
                    b_dl = (b_g[:, None] * np.abs(hit - p) + np.abs(g) * (b_p + EPS * np.abs(hit - p)) + EPS * np.abs(g * (hit - p))
                            + np.abs(gH) * (b_p * np.abs(t) + p * b_t) + 4 * EPS * np.abs(gH * p * t) + EPS * np.abs(ref["d_params"]))
                e_dl = np.abs(got["d_params"] - ref["d_params"]) / np.maximum(b_dl, 1e-300)
                e["d_params"] = np.where(edge[:, None] | skip[:, None], 0, e_dl).max(axis=1)
                b_dv = float(F32(VF)) * ref["we"] / Wt * e_term + 4 * EPS * np.abs(ref["d_values"])  # vf_coef (w / W) term: the term's error, four operations
                e["d_values"] = np.where(v_edge | skip, 0, np.abs(got["d_values"] - ref["d_values"]) / np.maximum(b_dv, 1e-300))
                for k, x in e.items():
                    x = np.where(skip, 0, x)
                    worst[k] = max(worst[k], float(x.max()))
                    assert (x <= 1).all(), (where, k, float(x.max()), int(np.argmax(x)))
                assert (bits(got["d_params"][~np.isfinite(c["logits"])]) == 0).all(), where  # masked logits: all-zero bits
                worst["stats"] = max(worst["stats"], check_stats_against_truth(got, ref, c, b_r, b_d, b_H, b_vl, edge, ENT, where))
                check_ieee_parts(got, c, ref["bad"], clip_vf, ENT, G, where)
                if q == 4:  # two calls: identical bits in every output
                    again = run_cat(w, c, clip_vf)
                    for k in got:
                        same(again[k], got[k], where + " second call " + k)
        finally:
            w.close()
    print("policy_loss categorical B %d: worst measured / bound: %s; %d rows left out at the branch edges"
          % (B, ", ".join("%s %.3f" % kv for kv in worst.items()), left_out))


def test_a_rows_bits_do_not_depend_on_the_batch():
    rng = np.random.default_rng(77)
    for A in (3, 17, 257, 1025):
        w = categorical_world(A)
        try:
            big = plm.make_case(rng, 257, A, 1.0, 0.5)
            small = {k: v[:65].copy() for k, v in big.items()}
            a, b = run_cat(w, big), run_cat(w, small)
            for k in ("logp", "entropy", "ratio", "pg", "vl"):
                same(b[k], a[k][:65], "A %d %s" % (A, k))
        finally:
            w.close()


# ---- 2. Gaussian ----
@pytest.mark.parametrize("C,per_row", ((2, False), (2, True), (3, False), (3, True)))
def test_gaussian_against_the_truth(C, per_row):
    import torch
    worst = dict(logp=0.0, entropy=0.0, ratio=0.0, pg=0.0, d_mean=0.0, d_log_std=0.0, d_log_std_shared=0.0, stats=0.0)
    rng = np.random.default_rng(10 * C + per_row)
    w = gaussian_world(C)
    try:
        for B in ROWS:
            for sigma in SIGMAS:
                c = plm.make_gauss_case(rng, B, C, per_row, sigma)
                clip_vf = CLIP_VF if C == 2 else None
                out = w.policy_loss(c["mean"], c["values"], list(c["action"].T.copy()), c["old_logp"], c["adv"], c["ret"], c["weight"],
                                    log_std=c["log_std"], old_value=c["old_value"], clip=CLIP, clip_vf=clip_vf, vf_coef=VF, ent_coef=ENT)
                torch.cuda.synchronize()
                got = {k: t.cpu().numpy().copy() for k, t in out.items()}
                ref = plm.truth(c["mean"], c["action"], c["old_logp"], c["adv"], c["ret"], c["values"], c["weight"], log_std=c["log_std"],
                                old_value=c["old_value"], clip=CLIP, clip_vf=clip_vf, vf_coef=VF, ent_coef=ENT)
                where = "C %d per_row %d B %d sigma %g" % (C, per_row, B, sigma)
                skip = ref["skip"]
                assert int(got["n_bad"][0]) == 0 and not ref["bad"].any(), where
                for k in ("logp", "entropy", "ratio", "pg", "vl", "d_values", "d_params", "d_log_std"):
                    assert (bits(got[k][skip]) == 0).all(), (where, k)
                z, sg = ref["z"], ref["sigma"]
                ls = np.broadcast_to(c["log_std"].astype(np.float64).reshape(-1, C), (B, C))
                e_z = 3 * EPS * np.abs(z)
                b_lp = (np.abs(z) * e_z).sum(axis=1) + 2 * EPS * (z * z + np.abs(ls) + 1).sum(axis=1)
                b_H = EPS * pm.entropy_scale(c["log_std"], B, C)
                b_d, b_r = ratio_bounds(ref, b_lp, c["old_logp"])
                edge = surrogate_edge(ref, b_r)
                assert edge.sum() <= 0.02 * B, (where, edge.sum())
                clip = float(F32(CLIP))
                rc = np.clip(ref["ratio"], 1 - clip, 1 + clip)
                adv = np.abs(c["adv"].astype(np.float64))
                b_pg = np.where(ref["active"], adv * b_r, adv * EPS * rc) + EPS * np.abs(ref["pg"])
                b_g = ref["we"] / ref["W"] * adv * b_r + 4 * EPS * np.abs(ref["g"])
                g, gH = np.abs(ref["g"])[:, None], np.abs(ref["gH"])[:, None]
                b_dm = b_g[:, None] * np.abs(z) / sg + g * e_z / sg + 3 * EPS * np.abs(ref["d_params"])
                b_dls = (b_g[:, None] * np.abs(z * z - 1) + g * (2 * np.abs(z) * e_z + EPS * (z * z + 1)) + EPS * g * np.abs(z * z - 1)
                         + 2 * EPS * gH + EPS * np.abs(ref["d_log_std"]))
                tiny = 1e-300
                e = dict(logp=np.abs(got["logp"] - ref["logp"]) / b_lp, entropy=np.abs(got["entropy"] - ref["entropy"]) / b_H,
                         ratio=np.abs(got["ratio"] - ref["ratio"]) / np.maximum(b_r, tiny),
                         pg=np.where(edge, 0, np.abs(got["pg"] - ref["pg"]) / np.maximum(b_pg, tiny)),
                         d_mean=np.where(edge[:, None], 0, np.abs(got["d_params"] - ref["d_params"]) / np.maximum(b_dm, tiny)).max(axis=1),
                         d_log_std=np.where(edge[:, None], 0, np.abs(got["d_log_std"] - ref["d_log_std"]) / np.maximum(b_dls, tiny)).max(axis=1))
                for k, x in e.items():
                    x = np.where(skip, 0, x)
                    worst[k] = max(worst[k], float(x.max()))
                    assert (x <= 1).all(), (where, k, float(x.max()), int(np.argmax(x)))
                # the shared log_std's gradient: the rows' bounds added up (an edge row: its whole magnitude)
                keep = ~skip
                row_mag = (np.abs(ref["g"])[:, None] * np.abs(z * z - 1) + np.abs(ref["gH"])[:, None])
                row_b = np.where(edge[:, None], ref["we"][:, None] / ref["W"] * (adv * ref["ratio"])[:, None] * np.abs(z * z - 1) + b_dls, b_dls)
                b_sh = row_b[keep].sum(axis=0) + B * 2.0 ** -50 * row_mag[keep].sum(axis=0) + EPS * np.abs(ref["d_log_std_shared"])
                e_sh = np.abs(got["d_log_std_shared"] - ref["d_log_std_shared"]) / np.maximum(b_sh, tiny)
                worst["d_log_std_shared"] = max(worst["d_log_std_shared"], float(e_sh.max()))
                assert (e_sh <= 1).all(), (where, e_sh)
                # stats against the truth, then the IEEE parts bit for bit from the device's own logp, entropy and ratio: pg, vl, the
                # folds of a launch with a lane per row (the first seven sums; the three for a shared log_std hang on the platform's
                # z and are held to the truth above), stats, inv_W, n_bad, d_values
                b_vl, _, _ = value_bounds(c, ref, clip_vf)
                worst["stats"] = max(worst["stats"], check_stats_against_truth(got, ref, c, b_r, b_d, b_H, b_vl, edge, ENT, where))
                check_ieee_parts(got, c, ref["bad"], clip_vf, ENT, 1, where)
                again = w.policy_loss(c["mean"], c["values"], list(c["action"].T.copy()), c["old_logp"], c["adv"], c["ret"], c["weight"],
                                      log_std=c["log_std"], old_value=c["old_value"], clip=CLIP, clip_vf=clip_vf, vf_coef=VF, ent_coef=ENT)
                torch.cuda.synchronize()
                for k, x in again.items():
                    same(x.cpu().numpy(), got[k], where + " second call " + k)
        print("policy_loss gaussian C %d per_row %d: worst measured / bound: %s" % (C, per_row, ", ".join("%s %.3f" % kv for kv in worst.items())))
    finally:
        w.close()


# ---- 3. bad rows ----
@pytest.mark.parametrize("A", (3, 17, 300))
def test_bad_rows_and_their_neighbours(A):
    B = 257
    w = categorical_world(A)
    try:
        rng = np.random.default_rng(A)
        c = plm.make_case(rng, B, A, 1.0, 0.5, zero_weight=0.0)
        clean = run_cat(w, c)
        l, a, adv = c["logits"].copy(), c["action"].copy(), c["adv"].copy()
        bad = [0, 1, 63, 64, 65, 130, 200, B - 1]
        l[0, A - 1] = np.nan                # a NaN logit
        l[1, 0] = np.inf                    # a +inf logit
        l[63, :] = -np.inf                  # an all-masked row
        a[64] = -1                          # an action of -1
        a[65] = A                           # an action of A
        a[130] = 0.5                        # a fractional action
        l[200, int(a[200])] = -np.inf       # a masked stored action
        if not np.isfinite(l[200]).any():
            l[200, (int(a[200]) + 1) % A] = 0.0
        adv[B - 1] = np.nan                 # a NaN advantage
        got = run_cat(w, c, logits=l, action=a, adv=adv)
        for k in ROW_KEYS:
            assert (bits(got[k][bad]) == 0).all(), k
        assert int(got["n_bad"][0]) == len(bad)
        ok = np.setdiff1d(np.arange(B), bad)
        for k in ("logp", "entropy", "ratio", "pg", "vl"):  # the neighbours in the same group, wavefront and workgroup
            same(got[k][ok], clean[k][ok], k)
        assert got["stats"][6] == B - len(bad) and clean["stats"][6] == B
        # the gradients scale with inv_W: the value gradient bit for bit through the model with this call's inv_W ...
        cb = dict(c, logits=l, action=a, adv=adv)
        truth_bad = cat_truth(cb)["bad"]
        assert sorted(np.flatnonzero(truth_bad).tolist()) == bad
        check_ieee_parts(got, cb, truth_bad, CLIP_VF, ENT, pm.group(A), "A %d bad rows" % A)
        # ... and d_params bit for bit against a call in which the same rows merely weigh nothing (the same W)
        wz = c["weight"].copy()
        wz[bad] = 0
        zeroed = run_cat(w, c, weight=wz)
        assert int(zeroed["n_bad"][0]) == 0  # counted per call, and only rows whose own weight was not 0
        same(got["d_params"][ok], zeroed["d_params"][ok], "d_params")
        same(got["d_values"][ok], zeroed["d_values"][ok], "d_values")
        same(got["stats"], zeroed["stats"], "stats")
        again = run_cat(w, c, logits=l, action=a, adv=adv)
        assert int(again["n_bad"][0]) == len(bad)
    finally:
        w.close()


# ---- 4. consistency with the sampler ----
@pytest.mark.parametrize("A", (3, 17, 257, 1025))
def test_unchanged_logits_give_the_samplers_logp_and_a_ratio_of_one(A):
    import torch
    R = 65
    w = categorical_world(A, R=R, max_rows=R)
    try:
        rng = np.random.default_rng(A)
        for draw, scale in enumerate((0.0, 1.0, 8.0)):
            l = torch.as_tensor(pm.make_logits(rng, R, A, scale), device="cuda")
            w.policy_sample(l, draw=draw)
            index, logp = w.policy["index"].to(torch.float32), w.policy["logp"].clone()
            t = {k: torch.as_tensor(rng.standard_normal(R).astype(F32), device="cuda") for k in ("adv", "ret", "values")}
            out = w.policy_loss(l, t["values"], index, logp, t["adv"], t["ret"], torch.ones(R, device="cuda"), clip=CLIP, vf_coef=VF, ent_coef=ENT)
            torch.cuda.synchronize()
            same(out["logp"].cpu().numpy(), logp.cpu().numpy(), "A %d logp" % A)
            same(out["entropy"].cpu().numpy(), w.policy["entropy"].cpu().numpy(), "A %d entropy" % A)
            assert (out["ratio"].cpu().numpy() == F32(1)).all()
            stats = out["stats"].cpu().numpy()
            assert stats[4] == 0 and stats[5] == 0 and int(out["n_bad"].item()) == 0
    finally:
        w.close()


# ---- 5. refusals that need a handle ----
def test_enable_and_call_refusals():
    from img_env_amd.world import World
    grid, params, layout = tiny_world(1)
    w = World(params, grid)
    try:
        w.enable_actions(discrete_actions=TABLE8)
        with pytest.raises(RuntimeError):
            w.enable_policy_loss(8)  # before enable_policy
        w.enable_policy("categorical", 1)
        with pytest.raises(RuntimeError):
            w.policy_loss(np.zeros((1, 8), F32), *[np.zeros(1, F32)] * 6)  # before enable_policy_loss
        out = w.enable_policy_loss(8)
        assert w.enable_policy_loss(8) is out and "d_log_std" not in out and out["d_params"].shape == (64,)
        with pytest.raises(ValueError):
            w.enable_policy_loss(9)  # another cfg
        z = np.zeros(4, F32)
        w.policy_loss(np.zeros((4, 8), F32), z, z, z, z, z, z)  # needs no reset and no rollout
        before, serial = w.launches(), w.policy_loss_serial
        assert serial == 1
        with pytest.raises(ValueError):
            w.policy_loss(np.zeros((9, 8), F32), *[np.zeros(9, F32)] * 6)  # rows > max_rows
        with pytest.raises(ValueError):
            w.policy_loss(np.zeros((4, 7), F32), z, z, z, z, z, z)
        with pytest.raises(ValueError):
            w.policy_loss(np.zeros((4, 8), F32), z, z, z, z, z, z, clip=-0.1)
        with pytest.raises(ValueError):
            w.policy_loss(np.zeros((4, 8), F32), z, z, z, z, z, z, clip_vf=-0.1, old_value=z)
        with pytest.raises(ValueError):
            w.policy_loss(np.zeros((4, 8), F32), z, z, z, z, z, z, clip_vf=0.2)  # no old_value
        assert w.launches() == before  # imgenv_step_launches does not count the loss's launches
        assert w.policy_loss_serial == serial  # a refused call queues nothing and counts for nothing
    finally:
        w.close()


# ---- 6. end to end ----
def test_a_ppo_iteration_end_to_end_and_the_feature_disturbs_nothing():
    import torch
    from img_env_amd.vec_env import VecImageEnv
    E, R, P, T, B = 4, 2, 2, 4, 8
    cfg = episode_cfg(R, P, discrete_action=True, discrete_actions=TABLE8)
    kw = dict(env_num=E, seed=9, device_reset=True, wrappers=True, rollout=T, minibatch=B)
    on = VecImageEnv(copy.deepcopy(cfg), policy=dict(seed=5, loss=True), **kw)
    off = VecImageEnv(copy.deepcopy(cfg), policy=dict(seed=5), **kw)
    try:
        assert off.world.policy_loss_out is None
        with pytest.raises(RuntimeError):
            off.policy_loss({}, logits=torch.zeros(1), values=torch.zeros(1))
        torch.manual_seed(0)
        s_on, s_off = on.reset(), off.reset()
        D = s_on.vector_states.shape[1]
        net = torch.nn.Linear(D, 9).to("cuda")

        def both(step):
            nonlocal s_on, s_off
            same(s_on.vector_states.cpu().numpy(), s_off.vector_states.cpu().numpy(), "step %d state" % step)
            with torch.no_grad():
                y = net(s_on.vector_states.to(torch.float32))
            logits, values = y[:, :8].contiguous(), y[:, 8].contiguous()
            s_on, r_on, d_on, i_on = on.policy_step(logits=logits, values=values)
            s_off, r_off, d_off, i_off = off.policy_step(logits=logits, values=values)
            assert on.world.launches() == off.world.launches()
            for name in ("vector_states", "sensor_maps", "lasers", "ped_maps", "rewards", "dones"):
                same(on.world.out[name].cpu().numpy(), off.world.out[name].cpu().numpy(), "step %d %s" % (step, name))
            same(i_on["policy"]["index"].cpu().numpy(), i_off["policy"]["index"].cpu().numpy(), "step %d index" % step)
        for step in range(T):
            both(step)
        with torch.no_grad():
            boot = net(s_on.vector_states.to(torch.float32))[:, 8].contiguous()
        on.policy_value(boot)
        ro = on.rollout()
        adv, ret = on.rollout_advantages(ro["pol_value"])
        scalars = dict(action=ro["pol_raw"][0], old_logp=ro["pol_logp"], old_value=ro["pol_value"], adv=adv, ret=ret)
        params = list(net.parameters())
        seen = 0
        for mb in on.rollout_minibatches(scalars, seed=3, normalise="adv"):
            x = mb["mb_vector_states"].to(torch.float32)
            y = net(x)
            logits, values = y[:, :8], y[:, 8]
            loss, info = on.policy_loss(mb, logits=logits, values=values, clip=CLIP, vf_coef=VF, ent_coef=ENT, clip_vf=CLIP_VF)
            assert loss.dim() == 0 and loss.requires_grad and set(info) >= {"loss", "approx_kl", "clip_fraction", "n_bad", "ratio", "logp"}
            net.zero_grad()
            loss.backward(retain_graph=True)
            out = on.world.policy_loss_out
            y2 = net(x)
            want = torch.autograd.grad((y2[:, :8], y2[:, 8]), params, grad_outputs=(out["d_params"][:B * 8].view(B, 8).clone(), out["d_values"][:B].clone()))
            for p, g in zip(params, want):
                assert torch.equal(p.grad, g)
            assert torch.equal(loss.detach(), info["loss"]) and int(info["n_bad"].item()) == 0
            wsum = float(mb["mb_weight"].sum().item())
            assert float(info["weight_sum"].item()) == wsum
            if wsum > 0:  # the window's own parameters: the ratio is 1 up to the network's own reproducibility
                assert abs(float(info["approx_kl"].item())) < 1e-5 and float(info["clip_fraction"].item()) == 0
                seen += 1
            on.world.policy_loss(y2[:, :8].detach(), y2[:, 8].detach(), mb["action"], mb["old_logp"], mb["adv"], mb["ret"], mb["mb_weight"])
            with pytest.raises(RuntimeError, match="later policy_loss"):
                loss.backward()  # the first call's graph: a later call -- here one made on the World directly -- has rewritten the gradients
        assert seen >= 1
        on.rollout_begin()
        off.rollout_begin()
        both(T)
    finally:
        on.close()
        off.close()
    with pytest.raises(ValueError):
        VecImageEnv(copy.deepcopy(cfg), env_num=2, seed=9, wrappers=True, policy=dict(seed=3, loss=True))  # needs minibatch=B


def test_clip_vf_with_three_gaussian_columns_is_refused():
    from img_env_amd.vec_env import VecImageEnv
    import torch
    cfg = episode_cfg(2, 2, discrete_action=False, continuous_actions=CLIP3, act_dim=3)
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=2, seed=9, device_reset=True, wrappers=True, rollout=2, minibatch=4, policy=dict(seed=5, loss=True))
    try:
        z = torch.zeros(4, device="cuda")
        mb = dict(a0=z, a1=z, a2=z, old_logp=z, adv=z, ret=z, old_value=z, mb_weight=z)
        with pytest.raises(ValueError, match="7 scalars"):
            vec.policy_loss(mb, mean=torch.zeros(4, 3, device="cuda"), log_std=torch.zeros(3, device="cuda"), values=z, clip_vf=0.2,
                            keys=dict(action=("a0", "a1", "a2")))
        mean = torch.zeros(4, 3, device="cuda", requires_grad=True)
        log_std = torch.zeros(3, device="cuda", requires_grad=True)
        loss, info = vec.policy_loss(dict(mb, mb_weight=z + 1), mean=mean, log_std=log_std, values=z, keys=dict(action=("a0", "a1", "a2")), ent_coef=0.5)
        loss.backward()
        assert mean.grad.shape == (4, 3) and torch.equal(log_std.grad, torch.full((3,), -0.5, device="cuda"))
    finally:
        vec.close()
