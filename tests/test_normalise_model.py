"""tests/normalise_model.py (the numpy model of img_env_amd/csrc/normalise.h) against the textbook: Stable-Baselines3's
RunningMeanStd.update_from_moments and VecNormalize's return bookkeeping written out below in plain np.mean / np.var, over a few
hundred random chains with frozen rows and resets.  The two differ only by the order of the sums.

Measured on the CPU this was written on, over the 300 chains of each of the three shapes below: the largest relative difference of
any statistic or return is 1.07e-15 (1 robot x 1: 0; 15 x 5: 1.07e-15; one tile + 1 rows x 7: 7.63e-16) -- a mean is measured
against max(|textbook|, the column's |offset| + scale), since a mean near 0 is a sum of much larger terms; a variance, a count
and a return against their own magnitude.  The test asserts 8 x 1.07e-15 = 8.56e-15 on those.  The outputs, float32 or clipped
float64 of values that differ in their last float64 bits, differed by 5.94e-8; they are held to one float32 step, 2^-23."""
import numpy as np
import pytest

import normalise_model as nm

MEASURED = 1.07e-15
BOUND = 8 * MEASURED


class Textbook:
    """RunningMeanStd (count 1e-4, mean 0, var 1) for the observation and for the returns, VecNormalize's update order"""

    def __init__(self, R, D, gamma, eps, clip_obs, clip_reward):
        self.o = [1e-4, np.zeros(D), np.ones(D)]
        self.r = [1e-4, 0.0, 1.0]
        self.returns = np.zeros(R)
        self.gamma, self.eps, self.clip_obs, self.clip_reward = gamma, eps, clip_obs, clip_reward

    @staticmethod
    def update(s, batch):
        n = batch.shape[0]
        if n == 0:
            return
        bm, bv = np.mean(batch, axis=0), np.var(batch, axis=0)
        count, mean, var = s
        delta, tot = bm - mean, count + n
        s[1] = mean + delta * n / tot
        s[2] = (var * count + bv * n + np.square(delta) * count * n / tot) / tot
        s[0] = tot

    def step(self, vs, rewards, clean, dones):
        clean = clean != 0
        self.returns[clean] = self.returns[clean] * self.gamma + rewards[clean]
        self.update(self.o, vs[clean].astype(np.float64))
        self.update(self.r, self.returns[clean])
        self.returns[dones != 0] = 0.0
        return (np.clip((vs - self.o[1]) / np.sqrt(self.o[2] + self.eps), -self.clip_obs, self.clip_obs),
                np.clip(rewards / np.sqrt(self.r[2] + self.eps), -self.clip_reward, self.clip_reward))

    def reset(self, rows, vs):
        self.update(self.o, vs[rows].astype(np.float64))
        self.returns[rows] = 0.0


def rel(a, b, scale):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), scale))) if a.size else 0.0


def run_chains(R, D, seed, chains=300):
    rng = np.random.default_rng(seed)
    offs, scl = rng.uniform(-3, 3, D), rng.uniform(0.1, 4, D)
    m = nm.Normalise(R, D)
    t = Textbook(R, D, 0.99, 1e-8, 10.0, 10.0)
    worst = worst_out = 0.0
    for _ in range(chains):
        vs = (offs + scl * rng.standard_normal((R, D))).astype(np.float32)
        if rng.random() < 0.25:
            rows = np.flatnonzero(rng.random(R) < 0.3)
            m.reset(rows, vs)
            t.reset(rows, vs)
        else:
            rewards = rng.standard_normal(R) * 3.0
            clean = (rng.random(R) < 0.8).astype(np.uint8)
            dones = (rng.random(R) < 0.1).astype(np.uint8)
            m.step(vs, rewards, clean, dones)
            to, tr = t.step(vs, rewards, clean, dones)
            worst_out = max(worst_out, rel(m.norm_vector_states, to, 1.0), rel(m.norm_rewards, tr, 1.0))
        # (the column's scale under a mean near 0: a difference is measured against what the sums were made of)
        worst = max(worst, rel(m.obs_mean, t.o[1], 1e-12 + np.abs(offs) + scl), rel(m.obs_var, t.o[2], 1e-12), rel(m.obs_count, t.o[0], 1e-12),
                    rel(m.ret_mean, t.r[1], 1.0), rel(m.ret_var, t.r[2], 1e-12), rel(m.ret_count, t.r[0], 1e-12), rel(m.returns, t.returns, 1.0))
    return worst, worst_out


@pytest.mark.parametrize("R,D,seed", [(1, 1, 0), (15, 5, 1), (nm.tile_rows(8) + 1, 7, 2)])
def test_model_against_the_textbook(R, D, seed):
    worst, worst_out = run_chains(R, D, seed)
    print("largest relative difference: statistics %.3g, outputs %.3g" % (worst, worst_out))
    assert worst <= BOUND
    assert worst_out <= 2.0 ** -23  # (float32 rounding of two values that differ in their last float64 bits)


def _bits(m):
    s = m.stats()
    return b"".join(np.asarray(s[k], np.float64).tobytes() for k in sorted(s))


def test_an_empty_batch_leaves_every_bit():
    rng = np.random.default_rng(3)
    m = nm.Normalise(6, 5)
    vs = rng.standard_normal((6, 5)).astype(np.float32)
    m.step(vs, rng.standard_normal(6), np.ones(6, np.uint8), np.zeros(6, np.uint8))
    before, ret = _bits(m), m.returns.copy()
    m.step(vs * 2, rng.standard_normal(6), np.zeros(6, np.uint8), np.zeros(6, np.uint8))  # every row frozen
    m.reset([], vs)                                                                      # a listed chain of no world
    assert _bits(m) == before and np.array_equal(m.returns, ret)
    # ... and the apply still follows the raw rows
    assert np.array_equal(m.norm_vector_states, np.clip((vs.astype(np.float64) * 2 - m.obs_mean) / np.sqrt(m.obs_var + 1e-8), -10, 10).astype(np.float32))


def test_a_single_sample():
    m = nm.Normalise(1, 2)
    x = np.array([[3.0, -1.5]], np.float32)
    m.step(x, np.array([2.0]), np.ones(1, np.uint8), np.zeros(1, np.uint8))
    c0, tot = 1e-4, 1e-4 + 1.0
    assert m.obs_count == tot and m.ret_count == tot
    assert np.array_equal(m.obs_mean, x[0].astype(np.float64) * 1.0 / tot)
    assert np.array_equal(m.obs_var, (1.0 * c0 + 0.0 + x[0].astype(np.float64) ** 2 * c0 * 1.0 / tot) / tot)
    assert m.returns[0] == 2.0 and m.ret_mean == 2.0 * 1.0 / tot
    m.step(x, np.array([1.0]), np.ones(1, np.uint8), np.ones(1, np.uint8))
    assert m.returns[0] == 0.0  # (the done row restarts after its return 2 * 0.99 + 1 went into the statistics)


def test_a_constant_column_stays_finite():
    R = 40
    m = nm.Normalise(R, 3, eps=1e-8)
    vs = np.tile(np.array([[0.25, -7.0, 1e-3]], np.float32), (R, 1))
    for _ in range(200):
        m.step(vs, np.zeros(R), np.ones(R, np.uint8), np.zeros(R, np.uint8))
    assert np.all(np.isfinite(m.norm_vector_states)) and np.all(m.obs_var >= 0.0) and np.all(m.obs_var < 1e-3)
    assert np.all(np.abs(m.norm_vector_states) <= 10.0) and m.ret_var < 1e-3 and np.all(np.isfinite(m.norm_rewards))


def test_values_at_the_clips():
    m = nm.Normalise(3, 1, clip_obs=2.0, clip_reward=0.5)
    m.training = False  # mean 0, var 1: x / sqrt(1 + 1e-8)
    vs = np.array([[2.0], [2.0000002], [-50.0]], np.float32)
    m.step(vs, np.array([0.5, 0.50000001, -9.0]), np.ones(3, np.uint8), np.zeros(3, np.uint8))
    den = np.sqrt(1.0 + 1e-8)
    assert m.norm_vector_states[:, 0].tolist() == [np.float32(2.0 / den), np.float32(2.0), np.float32(-2.0)]
    assert m.norm_rewards.tolist() == [0.5 / den, 0.5, -0.5]
    assert m.obs_count == 1e-4 and np.array_equal(m.returns, np.zeros(3))  # (evaluation: nothing moved)
