"""tests/policy_model.py held to what include/imgenv.h states for the policy head: the Philox known answers, the ranges of the
uniforms, the pick's fallback, masked actions, the mode, and the float32 restatement of the kernel's order against float64 truth
within the bounds the GPU tests apply to the kernel itself (tests/test_gpu_policy.py), on the same shapes."""
import numpy as np
import pytest

import policy_model as pm

F32 = np.float32
ROWS = (1, 63, 65, 257)
WIDTHS = (1, 2, 3, 8, 16, 17, 64, 65, 257, 1025, 4096)
SCALES = (0.0, 1.0, 8.0, 30.0)


def test_philox_known_answers():
    cases = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in cases:
        assert tuple(int(x) for x in pm.philox(ctr, key)) == want
    # vectorised = one at a time; the counter is (g lo, g hi, draw lo, draw hi), the key (seed lo, seed hi)
    g = np.array([0, 5, 2 ** 32 + 7], np.uint64)
    blocks = pm.draw_block(g, draw=(3 << 32) | 9, seed=(2 << 32) | 1)
    for q, gi in enumerate(g):
        assert np.array_equal(blocks[q], pm.philox((int(gi) & pm.MASK, int(gi) >> 32, 9, 3), (1, 2)))
    second = pm.draw_block(g, draw=(3 << 32) | 9, seed=(2 << 32) | 1, second=True)
    assert np.array_equal(second[1], pm.philox((5, 0, 9, 3 ^ 0x80000000), (1, 2)))


def test_uniform_ranges_are_exact():
    x = np.array([0, 255, 256, 0xffffff00, 0xffffffff], np.uint32)
    u, v = pm.u01(x), pm.u01_open(x)
    assert u.dtype == F32 and v.dtype == F32
    assert u[0] == 0 and u[1] == 0 and u[2] == F32(2.0 ** -24) and u[-1] == F32(1 - 2.0 ** -24) and (u < 1).all()
    assert v[0] == F32(2.0 ** -24) and v[-1] == 1 and (v > 0).all() and (v <= 1).all()
    assert np.array_equal(u.astype(np.float64), (x >> 8) / 2.0 ** 24) and np.array_equal(v.astype(np.float64), ((x >> 8) + 1.0) / 2.0 ** 24)


def test_group_and_block_partition():
    want = {1: 1, 16: 1, 17: 4, 64: 4, 65: 16, 256: 16, 257: 64, 1024: 64, 1025: 64, 4096: 64}
    for A, G in want.items():
        assert pm.group(A) == G
        spans = [pm.block(A, G, j) for j in range(G)]
        covered = [k for k0, n in spans for k in range(k0, k0 + n)]
        assert covered == list(range(A))
        assert max(n for _, n in spans) <= (16 if A <= 1024 else -(-A // 64))


def test_fallback_when_nothing_exceeds_the_target():
    # u = 1 stands for "u * s rounded to s": no cumulative sum exceeds s, the largest unmasked action is taken
    l = np.array([[0.0, 1.0, -np.inf, 0.5, -np.inf, -np.inf]], F32)
    out = pm.categorical_f32(l, np.array([1.0], F32))
    assert out["target"][0] == out["s"][0] and out["index"][0] == 3
    # and in a grouped row, where the trailing lanes hold nothing
    l = np.full((1, 40), -np.inf, F32)
    l[0, [0, 7, 21]] = [0.0, 2.0, 1.0]
    assert pm.categorical_f32(l, np.array([1.0], F32))["index"][0] == 21
    assert pm.categorical_f32(l, np.array([0.0], F32))["index"][0] == 0


def test_never_a_masked_action():
    rng = np.random.default_rng(11)
    for A in (2, 3, 17, 65, 257):
        l = pm.make_logits(rng, 200, A, 8.0, masked=0.6)
        for u in (rng.random(200).astype(F32), np.zeros(200, F32), np.full(200, 1 - 2.0 ** -24, F32)):
            idx = pm.categorical_f32(l, u)["index"]
            assert (idx >= 0).all() and np.isfinite(l[np.arange(200), idx]).all()


def test_mode_takes_the_lowest_index_of_a_tie():
    l = np.array([[-1.0, 3.0, 3.0, -np.inf, 3.0]], F32)
    out = pm.categorical_f32(l, np.array([0.9], F32), deterministic=True)
    assert out["index"][0] == 1
    wide = np.zeros((1, 300), F32)
    wide[0, [70, 290]] = 5.0
    assert pm.categorical_f32(wide, np.array([0.9], F32), deterministic=True)["index"][0] == 70


def test_bad_rows():
    l = np.zeros((5, 20), F32)
    l[0, 3] = np.nan
    l[1, 19] = np.inf
    l[2, :] = -np.inf
    l[3, 5] = -np.inf
    out = pm.categorical_f32(l, np.full(5, 0.5, F32))
    assert out["bad"].tolist() == [True, True, True, False, False]
    assert out["index"][:3].tolist() == [-1, -1, -1] and (out["logp"][:3] == 0).all() and (out["entropy"][:3] == 0).all()
    g = pm.gaussian_f32(np.array([[0, 0], [np.nan, 0], [0, 0], [0, np.inf]], F32), np.array([[0, 0], [0, 0], [0, 100], [0, 0]], F32), np.ones((4, 2), F32))
    assert g["bad"].tolist() == [False, True, True, True] and (g["raw"][1:] == 0).all() and (g["logp"][1:] == 0).all()


def test_gaussian_mode_is_the_mean():
    rng = np.random.default_rng(5)
    mu = rng.standard_normal((50, 3)).astype(F32)
    ls = rng.uniform(-5, 1, (50, 3)).astype(F32)
    out = pm.gaussian_f32(mu, ls, np.zeros((50, 3), F32))
    assert np.array_equal(out["raw"], mu + F32(0))
    assert np.allclose(out["logp"], (-ls.astype(np.float64) - 0.5 * np.log(2 * np.pi)).sum(axis=1), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("A", WIDTHS)
def test_categorical_restatement_against_truth(A):
    rng = np.random.default_rng(100 + A)
    mg = pm.margin(A)
    for R in ROWS:
        for scale in SCALES:
            l = pm.make_logits(rng, R, A, scale)
            u = pm.u01(pm.draw_block(np.arange(R), draw=A, seed=R)[:, 0])
            got, ref = pm.categorical_f32(l, u), pm.categorical_truth(l)
            rows, k = np.arange(R), got["index"]
            assert not got["bad"].any() and (k >= 0).all()
            F = ref["cdf"]
            below = np.where(k > 0, F[rows, np.maximum(k - 1, 0)], 0.0)
            assert (below - mg <= u).all() and (u <= F[rows, k] + mg).all() and (ref["p"][rows, k] > 0).all()
            lp = ref["logp"][rows, k]
            assert (np.abs(got["logp"] - lp) <= 2.0 ** -22 * (1 + np.abs(lp)) + mg).all()
            H = ref["entropy"]
            assert (np.abs(got["entropy"] - H) <= 2.0 ** -22 * (1 + H) + mg * (1 + np.log(A))).all()


def test_equal_logits_pin_the_high_bits():
    A, R = 4096, 257
    u = pm.u01(pm.draw_block(np.arange(R), draw=1, seed=2)[:, 0])
    k = pm.categorical_f32(np.zeros((R, A), F32), u)["index"]
    # (margin(4096) * 4096 is 2: "farther than that from an integer" excludes every row.  But with equal logits every e_k is 1,
    # every sum an integer <= 4096 and u * 4096 a scaling by a power of two -- all exact -- so the index is the floor on EVERY row)
    x = u.astype(np.float64) * A
    assert np.array_equal(k, np.floor(x).astype(np.int32)) and len(set(k.tolist())) > 200


@pytest.mark.parametrize("C", (2, 3))
def test_gaussian_restatement_against_truth(C):
    rng = np.random.default_rng(C)
    R = 4096
    g = np.arange(R) + 1000
    z, zt = pm.normals(g, 7, 9, C), pm.normals(g, 7, 9, C, truth=True)
    assert (np.abs(z - zt) <= 2.0 ** -18 * (1 + np.abs(zt))).all()
    out0 = pm.gaussian_f32(np.zeros((R, C), F32), np.zeros(C, F32), z)
    assert np.array_equal(out0["raw"], z + F32(0))
    for per_row in (False, True):
        mu = (rng.standard_normal((R, C)) * 3).astype(F32)
        ls = rng.uniform(-5, 1, (R, C) if per_row else (C,)).astype(F32)
        got, ref = pm.gaussian_f32(mu, ls, z), pm.gaussian_truth(mu, ls, zt)
        sigma = np.exp(np.broadcast_to(ls.astype(np.float64).reshape(-1, C), (R, C)))
        assert not got["bad"].any()
        assert (np.abs(got["raw"] - ref["raw"]) <= sigma * 2.0 ** -18 * (1 + np.abs(zt)) + 2.0 ** -22 * (1 + np.abs(mu))).all()
        bound = (np.abs(zt) * 2.0 ** -18 * (1 + np.abs(zt))).sum(axis=1) + 2.0 ** -21 * (1 + np.abs(ref["logp"]))
        assert (np.abs(got["logp"] - ref["logp"]) <= bound).all()
        assert (np.abs(got["entropy"] - ref["entropy"]) <= 2.0 ** -21 * pm.entropy_scale(ls, R, C)).all()
