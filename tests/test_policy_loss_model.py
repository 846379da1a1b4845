"""tests/policy_loss_model.py against torch.autograd of the textbook PPO loss in float64 on the CPU (categorical and Gaussian,
within 1e-12), the NaN that autograd returns for -inf logits where the closed form returns 0, known answers at the clip edges,
on both value-clip branches, for A = 1 and for all weights 0, and the float32 restatement against the truth."""
import numpy as np
import pytest

import policy_loss_model as plm
import policy_model as pm

F32 = np.float32
torch = pytest.importorskip("torch")
CLIP, CLIP_VF, VF, ENT = 0.2, 0.2, 0.5, 0.01


def textbook_categorical(c, mask_value, clip_vf=CLIP_VF):
    """loss and gradients by autograd; -inf logits stand as `mask_value`; the coefficients as the float32 the library takes"""
    CLIP, VF, ENT, clip_vf = (None if x is None else float(F32(x)) for x in (0.2, 0.5, 0.01, clip_vf))
    l = torch.tensor(np.where(np.isfinite(c["logits"]), c["logits"], mask_value).astype(np.float64), requires_grad=True)
    v = torch.tensor(c["values"].astype(np.float64), requires_grad=True)
    t = {k: torch.tensor(c[k].astype(np.float64)) for k in ("old_logp", "adv", "ret", "old_value", "weight")}
    B = l.shape[0]
    a = torch.tensor(c["action"].astype(np.int64))
    ls = torch.log_softmax(l, 1)
    p = ls.exp()
    logp = ls[torch.arange(B), a]
    H = -(p * ls).sum(1)
    r = (logp - t["old_logp"]).exp()
    pg = -torch.min(r * t["adv"], r.clamp(1 - CLIP, 1 + CLIP) * t["adv"])
    if clip_vf is None:
        vl = 0.5 * (v - t["ret"]) ** 2
    else:
        vc = t["old_value"] + (v - t["old_value"]).clamp(-clip_vf, clip_vf)
        vl = 0.5 * torch.max((v - t["ret"]) ** 2, (vc - t["ret"]) ** 2)
    W = t["weight"].sum().clamp(min=1)
    loss = (t["weight"] * (pg + VF * vl - ENT * H)).sum() / W
    loss.backward()
    return loss.item(), l.grad.numpy(), v.grad.numpy()


@pytest.mark.parametrize("A", (1, 3, 17, 65))
@pytest.mark.parametrize("clip_vf", (None, CLIP_VF))
def test_categorical_truth_equals_autograd(A, clip_vf):
    rng = np.random.default_rng(A)
    c = plm.make_case(rng, 257, A, 1.0, 0.5)
    ref = plm.truth(c["logits"], c["action"], c["old_logp"], c["adv"], c["ret"], c["values"], c["weight"], old_value=c["old_value"],
                    clip=CLIP, clip_vf=clip_vf, vf_coef=VF, ent_coef=ENT)
    loss, dl, dv = textbook_categorical(c, -1e4, clip_vf)
    assert ref["n_bad"] == 0
    assert abs(ref["stats"][0] - loss) <= 1e-12
    assert np.abs(ref["d_params"] - dl).max() <= 1e-12
    assert np.abs(ref["d_values"] - dv).max() <= 1e-12
    assert (ref["d_params"][~np.isfinite(c["logits"])] == 0).all()
    if A > 1:
        assert 0.2 < ref["stats"][5] < 0.95  # the clip fraction: both branches are populated
        if clip_vf is not None:
            assert 0.02 < (ref["use_c"] & ~ref["skip"]).mean() < 0.9


def test_autograd_returns_nan_for_masked_logits_and_the_closed_form_does_not():
    rng = np.random.default_rng(5)
    c = plm.make_case(rng, 65, 17, 1.0, 0.5)
    assert (~np.isfinite(c["logits"])).any()
    _, dl, _ = textbook_categorical(c, -np.inf)
    assert np.isnan(dl).any()
    ref = plm.truth(c["logits"], c["action"], c["old_logp"], c["adv"], c["ret"], c["values"], c["weight"], old_value=c["old_value"],
                    clip=CLIP, clip_vf=CLIP_VF, vf_coef=VF, ent_coef=ENT)
    assert np.isfinite(ref["d_params"]).all() and np.isfinite(ref["stats"]).all()


@pytest.mark.parametrize("C,per_row", ((2, False), (3, False), (2, True), (3, True)))
def test_gaussian_truth_equals_autograd(C, per_row):
    rng = np.random.default_rng(10 * C + per_row)
    c = plm.make_gauss_case(rng, 257, C, per_row, 0.5)
    clip, vf, ent = float(F32(CLIP)), float(F32(VF)), float(F32(ENT))
    ref = plm.truth(c["mean"], c["action"], c["old_logp"], c["adv"], c["ret"], c["values"], c["weight"], log_std=c["log_std"], clip=CLIP,
                    vf_coef=VF, ent_coef=ENT)
    mu = torch.tensor(c["mean"].astype(np.float64), requires_grad=True)
    ls = torch.tensor(c["log_std"].astype(np.float64), requires_grad=True)
    v = torch.tensor(c["values"].astype(np.float64), requires_grad=True)
    t = {k: torch.tensor(c[k].astype(np.float64)) for k in ("action", "old_logp", "adv", "ret", "weight")}
    z = (t["action"] - mu) / ls.exp()
    logp = (-0.5 * z * z - ls - 0.5 * np.log(2 * np.pi)).sum(1)
    H = (0.5 + 0.5 * np.log(2 * np.pi) + ls).expand(257, C).sum(1)
    r = (logp - t["old_logp"]).exp()
    pg = -torch.min(r * t["adv"], r.clamp(1 - clip, 1 + clip) * t["adv"])
    W = t["weight"].sum().clamp(min=1)
    loss = (t["weight"] * (pg + vf * 0.5 * (v - t["ret"]) ** 2 - ent * H)).sum() / W
    loss.backward()
    assert ref["n_bad"] == 0 and abs(ref["stats"][0] - loss.item()) <= 1e-12
    assert np.abs(ref["d_params"] - mu.grad.numpy()).max() <= 1e-12
    assert np.abs(ref["d_values"] - v.grad.numpy()).max() <= 1e-12
    assert np.abs(ref["d_log_std" if per_row else "d_log_std_shared"] - ls.grad.numpy()).max() <= 1e-12


def _one(logit_row, action, old_logp, adv, ret, v, w, **kw):
    return plm.truth(np.array([logit_row], F32), np.array([action], F32), np.array([old_logp], F32), np.array([adv], F32),
                     np.array([ret], F32), np.array([v], F32), np.array([w], F32), **kw)


def test_known_answers():
    # A = 1: logp 0, entropy 0, ratio exp(-old_logp), no gradient on the single logit
    ref = _one([0.7], 0, 0.0, 2.0, 1.0, 3.0, 1.0, clip=0.2, vf_coef=0.5, ent_coef=0.5)
    assert ref["logp"][0] == 0 and ref["entropy"][0] == 0 and ref["ratio"][0] == 1 and ref["d_params"][0, 0] == 0
    assert ref["stats"][0] == pytest.approx(-2.0 + 0.5 * 0.5 * 4.0, abs=1e-15) and ref["d_values"][0] == pytest.approx(0.5 * 2.0)
    # the ratio on either side of both clip edges, either sign of adv: two equal logits, old_logp chosen for the ratio
    clip = float(F32(0.2))
    for ratio, adv, active in ((0.79, 1.0, True), (0.79, -1.0, False), (0.81, 1.0, True), (0.81, -1.0, True),
                               (1.19, 1.0, True), (1.19, -1.0, True), (1.21, 1.0, False), (1.21, -1.0, True)):
        ref = _one([0.0, 0.0], 1, np.log(0.5) - np.log(ratio), adv, 0.0, 0.0, 1.0, clip=0.2, vf_coef=0.0, ent_coef=0.0)
        r = ref["ratio"][0]
        assert r == pytest.approx(ratio, rel=1e-6) and bool(ref["active"][0]) is active
        assert ref["pg"][0] == pytest.approx(-min(r * adv, min(max(r, 1 - clip), 1 + clip) * adv), abs=1e-15)
        want = -adv * r * 0.5 if active else 0.0  # d logit_1 = g (1 - p_1)
        assert ref["d_params"][0, 1] == pytest.approx(want, abs=1e-12) and ref["d_params"][0, 0] == pytest.approx(-want, abs=1e-12)
        assert ref["stats"][5] == (1.0 if abs(r - 1) > clip else 0.0)
    # both value-clip branches: old_v 0, clip_vf 0.2
    for v, ret, use_c, grad in ((0.1, 1.0, False, 0.1 - 1.0),   # inside the clip range: the plain square
                                (0.5, 1.0, True, 0.0),          # moved towards ret beyond the range: the clipped square, no gradient
                                (0.5, -1.0, False, 0.5 + 1.0)):  # moved away: the plain square is the larger
        ref = plm.truth(np.zeros((1, 2), F32), np.zeros(1, F32), np.full(1, np.log(0.5), F32), np.zeros(1, F32), np.array([ret], F32),
                        np.array([v], F32), np.ones(1, F32), old_value=np.zeros(1, F32), clip=0.2, clip_vf=0.2, vf_coef=1.0, ent_coef=0.0)
        assert bool(ref["use_c"][0]) is use_c and ref["d_values"][0] == pytest.approx(grad, abs=1e-7)
    # all weights 0: W = 1, everything 0
    rng = np.random.default_rng(2)
    c = plm.make_case(rng, 9, 5, 1.0, 0.5)
    ref = plm.truth(c["logits"], c["action"], c["old_logp"], c["adv"], c["ret"], c["values"], np.zeros(9, F32), clip=0.2)
    assert ref["W"] == 1 and (ref["stats"] == 0).all() and (ref["d_params"] == 0).all() and (ref["d_values"] == 0).all()
    assert (ref["logp"] == 0).all() and ref["n_bad"] == 0


def test_bad_rows_count_as_weight_zero():
    rng = np.random.default_rng(3)
    c = plm.make_case(rng, 16, 5, 1.0, 0.5, masked=0.0, zero_weight=0.0)
    l, a, adv, w = c["logits"].copy(), c["action"].copy(), c["adv"].copy(), c["weight"].copy()
    l[0, 1] = np.nan
    l[1, 0] = np.inf
    l[2, :] = -np.inf
    a[3], a[4], a[5] = -1, 5, 1.5
    l[6, int(a[6])] = -np.inf
    adv[7] = np.nan
    adv[8], w[8] = np.nan, 0.0  # bad, but of weight 0: not counted
    ref = plm.truth(l, a, c["old_logp"], adv, c["ret"], c["values"], w, clip=0.2)
    assert ref["bad"][:9].all() and not ref["bad"][9:].any() and ref["n_bad"] == 8
    assert (ref["d_params"][:9] == 0).all() and (ref["logp"][:9] == 0).all() and ref["stats"][6] == 7
    clean = plm.truth(c["logits"][9:], c["action"][9:], c["old_logp"][9:], c["adv"][9:], c["ret"][9:], c["values"][9:], c["weight"][9:], clip=0.2)
    assert np.array_equal(ref["d_params"][9:], clean["d_params"]) and ref["stats"][0] == clean["stats"][0]


@pytest.mark.parametrize("A", (3, 17))
def test_float32_restatement_follows_the_truth(A):
    """the float32 order on numpy's expf: rows within float32 rounding of the truth, the folds within float64 rounding of a plain
    sum, bad and weight-0 rows exactly 0"""
    rng = np.random.default_rng(A)
    B = 257
    c = plm.make_case(rng, B, A, 1.0, 0.5)
    u = np.zeros(B, F32)
    f32 = pm.categorical_f32(c["logits"], u)
    a = c["action"].astype(np.int64)
    logp = ((c["logits"][np.arange(B), a] - f32["m"]).astype(F32) - np.log(f32["s"]).astype(F32)).astype(F32)
    t = plm.row_terms_f32(logp, f32["bad"], c["old_logp"], c["adv"], c["ret"], c["values"], c["weight"], old_v=c["old_value"], clip=CLIP, clip_vf=CLIP_VF)
    ref = plm.truth(c["logits"], c["action"], c["old_logp"], c["adv"], c["ret"], c["values"], c["weight"], old_value=c["old_value"],
                    clip=CLIP, clip_vf=CLIP_VF, vf_coef=VF, ent_coef=ENT)
    keep = ~t["skip"]
    assert np.array_equal(t["skip"], ref["skip"])
    assert np.abs(t["ratio"][keep] - ref["ratio"][keep]).max() <= 1e-5 * (1 + ref["ratio"][keep].max())
    G = pm.group(A)
    contrib = plm.contributions(t, f32["entropy"], c["weight"])
    S = plm.fold_final(plm.fold_records(contrib, G))
    assert np.abs(S - contrib.sum(axis=0)).max() <= B * 2.0 ** -50 * np.abs(contrib).sum(axis=0).max()
    tot = plm.totals(S, VF, ENT)
    assert abs(float(tot["stats"][0]) - ref["stats"][0]) <= 1e-5 and tot["stats"][6] == ref["stats"][6] and tot["n_bad"] == 0
    gw, g, gH = plm.scales(t, c["weight"], tot["inv_W"], ENT)
    dv = plm.value_grad_f32(t, gw, VF)
    assert np.abs(dv - ref["d_values"]).max() <= 1e-6 and (dv[t["skip"]].view(np.uint32) == 0).all()
    dl = plm.cat_grad_f32(c["logits"], f32["m"], np.log(f32["s"]).astype(F32), f32["entropy"], g, gH, a, t["skip"])
    assert np.abs(dl - ref["d_params"]).max() <= 1e-6
    assert (dl[t["skip"]].view(np.uint32) == 0).all() and (dl[~np.isfinite(c["logits"])].view(np.uint32) == 0).all()


@pytest.mark.parametrize("C,per_row", ((2, False), (3, True)))
def test_gaussian_float32_restatement_follows_the_truth(C, per_row):
    """the Gaussian row, the three sums for a shared log_std and the gradients in the header's float32 order, on numpy's expf"""
    rng = np.random.default_rng(C)
    B = 257
    c = plm.make_gauss_case(rng, B, C, per_row, 0.5)
    ref = plm.truth(c["mean"], c["action"], c["old_logp"], c["adv"], c["ret"], c["values"], c["weight"], log_std=c["log_std"], clip=CLIP,
                    vf_coef=VF, ent_coef=ENT)
    f = plm.gauss_f32(c["mean"], c["log_std"], c["action"])
    assert not f["bad"].any() and np.abs(f["logp"] - ref["logp"])[~ref["skip"]].max() <= 1e-5
    t = plm.row_terms_f32(f["logp"], f["bad"], c["old_logp"], c["adv"], c["ret"], c["values"], c["weight"], clip=CLIP)
    assert np.array_equal(t["skip"], ref["skip"])
    contrib = plm.contributions(t, f["entropy"], c["weight"], dls=plm.gauss_dls_terms_f32(t, f["z"], c["weight"], ENT))
    tot = plm.totals(plm.fold_final(plm.fold_records(contrib, 1)), VF, ENT)
    assert abs(float(tot["stats"][0]) - ref["stats"][0]) <= 1e-5 and tot["n_bad"] == 0
    gw, g, gH = plm.scales(t, c["weight"], tot["inv_W"], ENT)
    dm, dl = plm.gauss_grads_f32(f["z"], f["sigma"], g, gH, t["skip"])
    assert np.abs(dm - ref["d_params"]).max() <= 1e-6 * (1 + np.abs(ref["d_params"]).max())
    assert np.abs(dl - ref["d_log_std"]).max() <= 1e-6 * (1 + np.abs(ref["d_log_std"]).max())
    assert np.abs(tot["dls"][:C] - ref["d_log_std_shared"]).max() <= 1e-5 and (tot["dls"][C:] == 0).all()
    assert (dm[t["skip"]].view(np.uint32) == 0).all() and (dl[t["skip"]].view(np.uint32) == 0).all()
