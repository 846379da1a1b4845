"""csrc/policy_loss.h's host/device rules and launch_plan.h's plan_policy_loss_launch on the CPU: tests/host/policy_loss_check.cpp
compiles them with g++, walks them over a simulated grid for G in {1, 4, 16, 64} and compares with vectors that
tests/policy_loss_model.py writes -- for a given ratio r, the row's terms, the owner lanes' contributions, the workgroups' records
(butterfly, then the wavefronts ascending), the final fold, the totals and the value gradient, bit for bit, bad and weight-0 rows
included; for the Gaussian launch also the three sums for a shared log_std and, for given z and sigma, its gradients.  The launch shapes, the stored action's rule and the Gaussian row's rules are asserted inside the program.  The same
program is also built once with -fsanitize=address,undefined and run directly."""
import os
import subprocess

import numpy as np

import policy_loss_model as plm
import policy_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SOURCE = os.path.join(ROOT, "tests", "host", "policy_loss_check.cpp")
FLAGS = ["-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include")]


def _hex(a):
    return " ".join("%x" % int(x) for x in np.asarray(a, F32).view(np.uint32).ravel())


def _hex64(a):
    return " ".join("%x" % int(x) for x in np.asarray(a, np.float64).view(np.uint64).ravel())


def _vectors():
    rng = np.random.default_rng(2025)
    lines = []
    shapes = [(1, 1), (5, 3), (63, 16), (65, 17), (257, 40), (70, 64), (65, 65), (257, 257), (33, 1025), (300, 0)]
    for q, (B, A) in enumerate(shapes):
        G = pm.group(A)
        clip_vf = None if q % 3 == 2 else 0.2
        clip, vf, ent = 0.2, 0.5, 0.01 * (q % 2)
        c = plm.make_case(rng, B, max(A, 2), 1.0, 0.5)
        logp = (c["old_logp"] + (rng.standard_normal(B) * 0.3).astype(F32)).astype(F32)  # any log-probability
        entropy = rng.uniform(0, 3, B).astype(F32)
        r = (np.exp(logp - c["old_logp"]).astype(F32) * (1 + rng.integers(-1, 2, B) * F32(2.0 ** -23))).astype(F32)  # any expf within an ulp
        bad, adv, w = np.zeros(B, bool), c["adv"].copy(), c["weight"].copy()
        if B >= 5:
            bad[1] = True            # what the parameters said
            adv[2] = np.nan          # a scalar that is not finite
            r[3] = np.inf            # a ratio that is not finite
            adv[4], w[4] = np.nan, 0  # bad but of weight 0: not counted
        t = plm.row_terms_f32(logp, bad, c["old_logp"], adv, c["ret"], c["values"], w, old_v=c["old_value"], clip=clip, clip_vf=clip_vf, r=r)
        z = sigma = dls = None
        if A == 0:  # the Gaussian launch: a lane per row, C = 3, any z and sigma
            z, sigma = rng.standard_normal((B, 3)).astype(F32), rng.uniform(0.1, 2.0, (B, 3)).astype(F32)
            dls = plm.gauss_dls_terms_f32(t, z, w, ent)
        contrib = plm.contributions(t, entropy, w, dls=dls)
        rec = plm.fold_records(contrib, G)
        S = plm.fold_final(rec)
        tot = plm.totals(S, vf, ent)
        gw, g, gH = plm.scales(t, w, tot["inv_W"], ent)
        grad = plm.value_grad_f32(t, gw, vf)
        lines.append("CASE %d %d %d %d %s" % (B, A, G, clip_vf is not None, _hex([clip, clip_vf or 0.0, vf, ent])))
        for i in range(B):
            lines.append("ROW %s %d %s %d %s" % (_hex([logp[i], entropy[i], r[i], c["old_logp"][i], adv[i], c["ret"][i], c["values"][i], c["old_value"][i], w[i]]),
                                                 int(bad[i]), _hex([t["ratio"][i], t["pg"][i], t["vl"][i], t["kl"][i], t["clipped"][i], t["gu"][i]]),
                                                 int(t["skip"][i]), _hex([t["term"][i]]))
                         + ("" if z is None else " " + _hex(z[i]) + " " + _hex(sigma[i])))
        lines.append("REC %d %s" % (len(rec), _hex64(rec)))
        lines.append("SUM " + _hex64(S))
        lines.append("TOT %s %s %s %d" % (_hex(tot["stats"]), _hex([tot["inv_W"]]), _hex(tot["dls"]), tot["n_bad"]))
        if z is not None:
            dm, dl = plm.gauss_grads_f32(z, sigma, g, gH, t["skip"])
        for i in range(B):
            lines.append("VG %s %s" % (_hex([gw[i]]), _hex([grad[i]]))
                         + ("" if z is None else " %s %s %s" % (_hex([g[i], gH[i]]), _hex(dm[i]), _hex(dl[i]))))
    return "\n".join(lines) + "\n"


def _run(tmp_path, name, extra):
    exe, vec = str(tmp_path / name), str(tmp_path / "vectors.txt")
    with open(vec, "w") as fh:
        fh.write(_vectors())
    subprocess.check_call(["g++"] + FLAGS + extra + [SOURCE, "-o", exe])
    out = subprocess.run([exe, vec], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr


def test_policy_loss_rules_on_a_simulated_grid(tmp_path):
    _run(tmp_path, "policy_loss_check", [])


def test_the_same_program_under_the_address_and_undefined_sanitizers(tmp_path):
    """a stand-alone program with its own main, run directly"""
    _run(tmp_path, "policy_loss_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
