"""PPO's loss (csrc/policy_loss.h; include/imgenv.h: imgenv_policy_loss) in numpy, without the library:

  * ``truth``: the definition in float64 -- log-probability of the stored action and entropy under the new parameters, ratio,
    clipped surrogate, (clipped) value loss, the weighted means and the closed-form gradients, bad and weight-0 rows as zeros;
  * the float32 restatement of everything that is plain IEEE arithmetic, in the header's order: the row's terms for a given
    log-probability and ratio (``row_terms_f32``), the value gradient, the categorical and Gaussian gradients for given p / z,
    and the float64 folds -- the workgroup's butterfly and wavefront order, the final fold, the totals (``fold_records``,
    ``fold_final``, ``totals``).
"""
import numpy as np

import policy_model as pm

F32 = np.float32
REC = 10
W_, PG, VL, H_, KL, CLIPPED, BAD, DLS = 0, 1, 2, 3, 4, 5, 6, 7
BLOCK, WAVE = 256, 64


def _f64(x):
    return np.asarray(x, F32).astype(np.float64)


def _finite(*xs):
    ok = True
    for x in xs:
        ok = ok & np.isfinite(np.asarray(x, np.float64))
    return ok


def truth(params, action, old_logp, adv, ret, values, weight, log_std=None, old_value=None, clip=0.2, clip_vf=None, vf_coef=0.5,
          ent_coef=0.0):
    """float64 on the float32 inputs.  Categorical (log_std None): params [B, A] logits, action [B] the index as a float;
    Gaussian: params [B, C] means, log_std [C] or [B, C], action [B, C] raw.  Returns a dict of row arrays, stats [8], W, inv_W,
    n_bad, the gradients and the branch masks (active, use_c, inside) the GPU test's edge exclusion needs."""
    p_in = np.asarray(params, F32)
    B, n = p_in.shape
    cat = log_std is None
    old_logp, adv, ret, v, w = (_f64(x) for x in (old_logp, adv, ret, values, weight))
    clip_value = clip_vf is not None
    old_v = _f64(old_value) if clip_value else np.zeros(B)
    clip, vf_coef, ent_coef = float(F32(clip)), float(F32(vf_coef)), float(F32(ent_coef))
    cvf = float(F32(clip_vf)) if clip_value else 0.0
    rows = np.arange(B)
    with np.errstate(all="ignore"):
        if cat:
            ref = pm.categorical_truth(p_in)
            af = _f64(action)
            valid = (af >= 0) & (af < n) & (af == np.floor(af))
            a = np.where(valid, af, 0).astype(np.int64)
            bad = ref["bad"] | ~valid | (p_in[rows, a] == -np.inf)
            logp, H, prob, lp_all = ref["logp"][rows, a], ref["entropy"], ref["p"], ref["logp"]
        else:
            mu, raw = p_in.astype(np.float64), _f64(action).reshape(B, n)
            ls = np.broadcast_to(_f64(log_std).reshape(-1, n), (B, n))
            sigma = np.exp(ls)
            z = (raw - mu) / sigma
            sigma32 = sigma.astype(F32)  # (the device's sigma is a float32: one that overflows or underflows to 0 makes a bad row)
            bad = ~(_finite(mu, ls, raw, z) & np.isfinite(sigma32) & (sigma32 > 0)).all(axis=1)
            logp = (-0.5 * z * z - ls - 0.5 * np.log(2.0 * np.pi)).sum(axis=1)
            H = (0.5 + 0.5 * np.log(2.0 * np.pi) + ls).sum(axis=1)
        d = logp - old_logp
        r = np.exp(d)
        bad = bad | ~_finite(old_logp, adv, ret, v, w, r) | (clip_value & ~_finite(old_v)) | (r > np.finfo(F32).max)
        s1, rc = r * adv, np.clip(r, 1.0 - clip, 1.0 + clip)
        s2 = rc * adv
        active = s1 <= s2
        pg = -np.minimum(s1, s2)
        dv = v - ret
        q = dv * dv
        dc = v - old_v
        vc = old_v + np.clip(dc, -cvf, cvf)
        dvc = vc - ret
        qc = dvc * dvc
        use_c = clip_value & (qc > q)
        inside = np.abs(dc) <= cvf
        vl = 0.5 * np.where(use_c, qc, q)
        kl = (r - 1.0) - d
        clipped = (np.abs(r - 1.0) > clip).astype(np.float64)
        skip = bad | (w == 0)
        we = np.where(skip, 0.0, w)
        z0 = lambda x: np.where(skip, 0.0, x)  # noqa: E731
        logp, H, r, pg, vl, kl, clipped = (z0(x) for x in (logp, H, r, pg, vl, kl, clipped))
        W = max(we.sum(), 1.0)
        S = [(we * x).sum() for x in (pg, vl, H, kl, clipped)]
        stats = np.array([(S[0] + vf_coef * S[1] - ent_coef * S[2]) / W, S[0] / W, S[1] / W, S[2] / W, S[3] / W, S[4] / W, we.sum(), 0.0])
        g = we / W * np.where(active, -z0(adv) * r, 0.0)
        gH = -ent_coef * we / W
        out = dict(logp=logp, entropy=H, ratio=r, pg=pg, vl=vl, kl=kl, clipped=clipped, bad=bad, skip=skip, active=active, use_c=use_c,
                   inside=inside, W=W, inv_W=1.0 / W, stats=stats, n_bad=int((bad & (w != 0)).sum()), g=g, gH=gH, we=we,
                   q=0.5 * q, qc=0.5 * qc)
        if cat:
            onehot = (np.arange(n)[None, :] == a[:, None]).astype(np.float64)
            lnp = np.where(prob > 0, lp_all, 0.0)
            dl = g[:, None] * (onehot - prob) - gH[:, None] * prob * (lnp + H[:, None])
            out["d_params"] = np.where(skip[:, None] | (p_in == -np.inf), 0.0, dl)
        else:
            out["z"], out["sigma"] = z, sigma
            out["d_params"] = np.where(skip[:, None], 0.0, g[:, None] * z / sigma)
            out["d_log_std"] = np.where(skip[:, None], 0.0, g[:, None] * (z * z - 1.0) + gH[:, None])
            out["d_log_std_shared"] = out["d_log_std"].sum(axis=0)
        term = np.where(use_c, np.where(inside, dvc, 0.0), dv)
        out["d_values"] = np.where(skip, 0.0, vf_coef * we / W * term)
    return out


# ---- float32, the header's order ----
def _clip32(f, lo, hi):
    f = np.where(f >= lo, f, lo).astype(F32)
    return np.where(f <= hi, f, hi).astype(F32)


def row_terms_f32(logp, bad, old_logp, adv, ret, v, w, old_v=None, clip=0.2, clip_vf=None, r=None):
    """ploss_row_terms on arrays: `r` given (the platform's expf(logp - old_logp)) or numpy's; dict of float32 arrays and masks"""
    logp, old_logp, adv, ret, v, w = (np.asarray(x, F32) for x in (logp, old_logp, adv, ret, v, w))
    clip = F32(clip)
    clip_value = clip_vf is not None
    with np.errstate(all="ignore"):
        bad = np.asarray(bad, bool) | ~(np.isfinite(old_logp) & np.isfinite(adv) & np.isfinite(ret) & np.isfinite(v) & np.isfinite(w))
        if clip_value:
            old_v, cvf = np.asarray(old_v, F32), F32(clip_vf)
            bad = bad | ~np.isfinite(old_v)
        d = (logp - old_logp).astype(F32)
        r = np.exp(d).astype(F32) if r is None else np.asarray(r, F32)
        bad = bad | ~np.isfinite(r)
        s1 = (r * adv).astype(F32)
        rc = _clip32(r, F32(1) - clip, F32(1) + clip)
        s2 = (rc * adv).astype(F32)
        active = s1 <= s2
        pg = (F32(0) - np.where(active, s1, s2)).astype(F32)
        dv = (v - ret).astype(F32)
        q = (dv * dv).astype(F32)
        term = dv
        if clip_value:
            dc = (v - old_v).astype(F32)
            vc = (old_v + _clip32(dc, F32(0) - cvf, cvf)).astype(F32)
            dvc = (vc - ret).astype(F32)
            qc = (dvc * dvc).astype(F32)
            use_c = qc > q
            term = np.where(use_c, np.where(np.abs(dc) <= cvf, dvc, F32(0)), dv).astype(F32)
            q = np.where(use_c, qc, q).astype(F32)
        vl = (F32(0.5) * q).astype(F32)
        kl = ((r - F32(1)).astype(F32) - d).astype(F32)
        clipped = (np.abs((r - F32(1)).astype(F32)) > clip).astype(F32)
        gu = (w * np.where(active, ((F32(0) - adv).astype(F32) * r).astype(F32), F32(0)).astype(F32)).astype(F32)
    skip = bad | (w == 0)
    return dict(ratio=r, pg=pg, vl=vl, kl=kl, clipped=clipped, gu=gu, bad=bad, skip=skip, term=term, active=active)


def contributions(t, entropy, w, dls=None):
    """the owner lanes' float64 contributions [B, REC] (ploss_contribute; dls: the Gaussian t_c [B, C] as float32)"""
    w = np.asarray(w, F32)
    B = len(w)
    c = np.zeros((B, REC))
    wd = w.astype(np.float64)
    keep = ~t["skip"]
    with np.errstate(invalid="ignore", over="ignore"):
        prods = {k: wd * np.asarray(x, F32).astype(np.float64) for k, x in ((PG, t["pg"]), (VL, t["vl"]), (H_, entropy), (KL, t["kl"]), (CLIPPED, t["clipped"]))}
    for k, x in prods.items():
        c[keep, k] = x[keep]
    c[keep, W_] = wd[keep]
    with np.errstate(invalid="ignore"):
        c[:, BAD] = (t["bad"] & (w != 0)).astype(np.float64)
    if dls is not None:
        dls = np.asarray(dls, F32)
        c[keep, DLS:DLS + dls.shape[1]] = dls.astype(np.float64)[keep]
    return c


def _butterfly(x):
    """x [..., 64, REC] -> lane 0 of x = x + x[lane ^ d], d = 1 .. 32"""
    lanes = np.arange(WAVE)
    d = 1
    while d < WAVE:
        x = x + x[..., lanes ^ d, :]
        d *= 2
    return x[..., 0, :]


def fold_records(contrib, G):
    """the row launch's records [grid, REC]: row i's contribution sits in lane i * G of the grid"""
    B = len(contrib)
    grid = -(-B * G // BLOCK)
    lanes = np.zeros((grid * BLOCK, REC))
    lanes[np.arange(B) * G] = contrib
    waves = _butterfly(lanes.reshape(grid, BLOCK // WAVE, WAVE, REC))
    rec = waves[:, 0]
    for q in range(1, BLOCK // WAVE):
        rec = rec + waves[:, q]
    return rec


def fold_final(rec):
    """k_ploss_fold: lane t adds records t, t + 64, ... ascending from 0, then the butterfly"""
    acc = np.zeros((WAVE, REC))
    for q0 in range(0, len(rec), WAVE):
        part = rec[q0:q0 + WAVE]
        acc[:len(part)] = acc[:len(part)] + part
    return _butterfly(acc)


def totals(S, vf_coef, ent_coef):
    """ploss_totals: stats float32 [8], inv_W float32, dls float32 [3], n_bad"""
    Wm = S[W_] if S[W_] > 1.0 else 1.0
    vf, ec = float(F32(vf_coef)), float(F32(ent_coef))
    stats = np.array([((S[PG] + vf * S[VL]) - ec * S[H_]) / Wm, S[PG] / Wm, S[VL] / Wm, S[H_] / Wm, S[KL] / Wm, S[CLIPPED] / Wm, S[W_], 0.0]).astype(F32)
    return dict(stats=stats, inv_W=F32(1.0 / Wm), dls=(S[DLS:DLS + 3] / Wm).astype(F32), n_bad=int(S[BAD]))


def scales(t, w, inv_W, ent_coef):
    """gw, g, gH of the gradient launch (0 for skipped rows)"""
    w = np.where(t["skip"], F32(0), np.asarray(w, F32)).astype(F32)
    gu = np.where(t["skip"], F32(0), t["gu"]).astype(F32)
    gw = (w * F32(inv_W)).astype(F32)
    return gw, (gu * F32(inv_W)).astype(F32), ((F32(0) - F32(ent_coef)) * gw).astype(F32)


def value_grad_f32(t, gw, vf_coef):
    with np.errstate(all="ignore"):
        out = ((F32(vf_coef) * gw).astype(F32) * t["term"]).astype(F32)
    return np.where(t["skip"], F32(0), out).astype(F32)


def cat_grad_f32(logits, m, log_s, entropy, g, gH, action, skip, p=None):
    """d_params of the categorical head for given p (the platform's expf(lp)) or numpy's"""
    l = np.asarray(logits, F32)
    B, A = l.shape
    with np.errstate(all="ignore"):
        lp = ((l - np.asarray(m, F32)[:, None]).astype(F32) - np.asarray(log_s, F32)[:, None]).astype(F32)
        p = np.exp(lp).astype(F32) if p is None else np.asarray(p, F32)
        hit = (np.arange(A)[None, :] == np.asarray(action).astype(np.int64)[:, None]).astype(F32)
        a = (g[:, None] * (hit - p).astype(F32)).astype(F32)
        b = (gH[:, None] * (p * (lp + np.asarray(entropy, F32)[:, None]).astype(F32)).astype(F32)).astype(F32)
        out = (a - b).astype(F32)
    return np.where(np.asarray(skip)[:, None] | (l == -np.inf), F32(0), out).astype(F32)


def gauss_f32(mean, log_std, raw, sigma=None):
    """ploss_gauss_row: z, sigma, logp, entropy, bad for a given sigma (the platform's expf) or numpy's"""
    mu, raw = np.asarray(mean, F32), np.asarray(raw, F32)
    B, C = mu.shape
    ls = np.broadcast_to(np.asarray(log_std, F32).reshape(-1, C), (B, C))
    with np.errstate(all="ignore"):
        sigma = np.exp(ls).astype(F32) if sigma is None else np.asarray(sigma, F32)
        z = ((raw - mu).astype(F32) / sigma).astype(F32)
        bad = ~(np.isfinite(mu) & np.isfinite(ls) & np.isfinite(sigma) & np.isfinite(raw) & np.isfinite(z)).all(axis=1)
        logp, ent = np.zeros(B, F32), np.zeros(B, F32)
        for c in range(C):
            logp = (logp + ((((F32(-0.5) * z[:, c]).astype(F32) * z[:, c]).astype(F32) - ls[:, c]).astype(F32) - pm.HALF_LN_2PI).astype(F32)).astype(F32)
            ent = (ent + (pm.ENT_CONST + ls[:, c]).astype(F32)).astype(F32)
    return dict(z=z, sigma=sigma, logp=logp, entropy=ent, bad=bad)


def gauss_grads_f32(z, sigma, g, gH, skip):
    with np.errstate(all="ignore"):
        dm = ((g[:, None] * z).astype(F32) / sigma).astype(F32)
        dls = ((g[:, None] * ((z * z).astype(F32) - F32(1)).astype(F32)).astype(F32) + gH[:, None]).astype(F32)
    s = np.asarray(skip)[:, None]
    return np.where(s, F32(0), dm).astype(F32), np.where(s, F32(0), dls).astype(F32)


def gauss_dls_terms_f32(t, z, w, ent_coef):
    """t_c = gu (z z - 1) + (0 - ent_coef) w: what the row launch adds up for the shared log_std"""
    w = np.asarray(w, F32)
    with np.errstate(all="ignore"):
        ghu = ((F32(0) - F32(ent_coef)) * w).astype(F32)
        return ((t["gu"][:, None] * ((z * z).astype(F32) - F32(1)).astype(F32)).astype(F32) + ghu[:, None]).astype(F32)


# ---- test inputs ----
def make_case(rng, B, A, scale, sigma, masked=0.2, zero_weight=0.2):
    """a categorical batch: new logits, actions drawn from the old distribution (new + N(0, sigma)), its log-probabilities,
    advantages, returns, old and new values, weights with `zero_weight` of them 0"""
    l = pm.make_logits(rng, B, A, scale, masked)
    old = np.where(np.isfinite(l), l + (rng.standard_normal((B, A)) * sigma).astype(F32), l).astype(F32)
    ref = pm.categorical_truth(old)
    u = rng.random(B)
    a = np.minimum((ref["cdf"] < u[:, None]).sum(axis=1), A - 1)
    a = np.where(ref["p"][np.arange(B), a] > 0, a, np.argmax(ref["p"], axis=1))
    old_logp = ref["logp"][np.arange(B), a].astype(F32)
    ret = rng.standard_normal(B).astype(F32)
    old_v = (ret + 0.3 * rng.standard_normal(B)).astype(F32)
    v = (old_v + 0.3 * rng.standard_normal(B)).astype(F32)
    w = (rng.random(B) >= zero_weight).astype(F32)
    return dict(logits=l, action=a.astype(F32), old_logp=old_logp, adv=rng.standard_normal(B).astype(F32), ret=ret, old_value=old_v,
                values=v, weight=w)


def make_gauss_case(rng, B, C, per_row, sigma, zero_weight=0.2):
    mu = (rng.standard_normal((B, C)) * 0.5).astype(F32)
    ls = rng.uniform(-2, 0.5, (B, C) if per_row else (C,)).astype(F32)
    sd = np.exp(np.broadcast_to(ls.reshape(-1, C), (B, C)).astype(np.float64))
    raw = (mu + sd * rng.standard_normal((B, C))).astype(F32)
    new_mu = (mu + sigma * sd * rng.standard_normal((B, C))).astype(F32)
    z = (raw.astype(np.float64) - mu) / sd
    old_logp = (-0.5 * z * z - np.log(sd) - 0.5 * np.log(2 * np.pi)).sum(axis=1).astype(F32)
    ret = rng.standard_normal(B).astype(F32)
    old_v = (ret + 0.3 * rng.standard_normal(B)).astype(F32)
    v = (old_v + 0.3 * rng.standard_normal(B)).astype(F32)
    w = (rng.random(B) >= zero_weight).astype(F32)
    return dict(mean=new_mu, log_std=ls, action=raw, old_logp=old_logp, adv=rng.standard_normal(B).astype(F32), ret=ret, old_value=old_v,
                values=v, weight=w)
