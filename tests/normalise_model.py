"""numpy model of img_env_amd/csrc/normalise.h, operation for operation and in the kernels' order of every sum: the running
statistics of the observation vector and of the discounted return (Stable-Baselines3's RunningMeanStd inside VecNormalize), the
returns, and the normalised arrays.  Everything is float64 elementwise arithmetic, which numpy rounds as the C code does.

The batch of a chain is a list of covered rows in the chain's order with a flag "counts"; its columns are the state's D elements
and, on a step, the return.  A wavefront holds rpw = 64 // cols whole rows, a tile is 8 x 4 x rpw rows: position p of a tile is
sample i = p // (4 rpw) of wavefront w = (p // rpw) % 4, row r = p % rpw.  A lane adds its 8 samples in order, the rows of a
wavefront fold by halves, the wavefronts add up 0, 1, 2, 3; the tiles merge in order (Chan), then the batch into the running triple."""
import numpy as np

WAVE, NORM_BLOCK, NORM_PER_LANE = 64, 256, 8
NORM_WAVES = NORM_BLOCK // WAVE


def rows_per_wave(cols):
    return WAVE // max(cols, 1)


def tile_rows(cols):
    return NORM_WAVES * rows_per_wave(cols) * NORM_PER_LANE


def half0(rpw):
    half = 1
    while half * 2 < rpw:
        half *= 2
    return half if rpw > 1 else 0


def block_fold(a):
    """``a`` [waves, rpw, cols] lane values -> [cols]: norm_fold"""
    a = a.copy()
    rpw = a.shape[1]
    half = half0(rpw)
    while half > 0:
        k = min(half, rpw - half)
        a[:, :k] = a[:, :k] + a[:, half:half + k]
        half >>= 1
    t = a[0, 0]
    for w in range(1, NORM_WAVES):
        t = t + a[w, 0]
    return t


def tile_partial(x, have):
    """one tile: ``x`` float64 [n, cols], ``have`` bool [n] (n <= tile_rows) -> (rows, mean [cols], M2 [cols])"""
    n, cols = x.shape
    rpw = rows_per_wave(cols)
    X = np.zeros((NORM_PER_LANE, NORM_WAVES, rpw, cols))
    H = np.zeros((NORM_PER_LANE, NORM_WAVES, rpw), bool)
    X.reshape(-1, cols)[:n] = x
    H.reshape(-1)[:n] = have
    acc = np.zeros((NORM_WAVES, rpw, cols))
    for i in range(NORM_PER_LANE):
        acc = np.where(H[i][..., None], acc + X[i], acc)
    c = int(H.sum())
    if c == 0:
        return 0, np.zeros(cols), np.zeros(cols)
    mean = block_fold(acc) / np.float64(c)
    acc = np.zeros((NORM_WAVES, rpw, cols))
    for i in range(NORM_PER_LANE):
        d = X[i] - mean
        acc = np.where(H[i][..., None], acc + d * d, acc)
    return c, mean, block_fold(acc)


def batch_triple(x, have):
    """the chain's batch: ``x`` float64 [covered, cols] in the chain's row order, ``have`` bool [covered] -> (c, mean, M2)"""
    n, cols = x.shape
    T = tile_rows(cols)
    bc, bm, b2 = np.float64(0.0), np.zeros(cols), np.zeros(cols)
    for t in range((n + T - 1) // T):
        c, m, m2 = tile_partial(x[t * T:(t + 1) * T], have[t * T:(t + 1) * T])
        if c == 0:
            continue
        cb = np.float64(c)
        if bc == 0.0:
            bc, bm, b2 = cb, m, m2
            continue
        delta, tot = m - bm, bc + cb
        bm = bm + delta * cb / tot
        b2 = b2 + m2 + delta * delta * bc * cb / tot
        bc = tot
    return bc, bm, b2


def merge(count, mean, var, c, bm, m2):
    """Chan's merge of the batch (c, bm, M2) into the running (count, mean, var); an empty batch leaves every bit"""
    if c == 0.0:
        return count, mean, var
    delta, tot = bm - mean, count + c
    return tot, mean + delta * c / tot, (var * count + m2 + delta * delta * count * c / tot) / tot


class Normalise:
    def __init__(self, R, D, K=0, obs=True, reward=True, gamma=0.99, clip_obs=10.0, clip_reward=10.0, eps=1e-8):
        self.R, self.D, self.K, self.obs, self.reward = R, D, K if obs else 0, obs, reward
        self.gamma, self.clip_obs, self.clip_reward, self.eps = (np.float64(v) for v in (gamma, clip_obs, clip_reward, eps))
        self.obs_count, self.obs_mean, self.obs_var = np.float64(1e-4), np.zeros(D), np.ones(D)
        self.ret_count, self.ret_mean, self.ret_var = np.float64(1e-4), np.float64(0.0), np.float64(1.0)
        self.returns = np.zeros(R)
        self.norm_vector_states = np.zeros((R, D), np.float32)
        self.norm_state_stack = np.zeros((R, self.K, D), np.float32)
        self.norm_rewards = np.zeros(R)
        self.training = True

    def stats(self):
        return {"obs_count": self.obs_count, "obs_mean": self.obs_mean.copy(), "obs_var": self.obs_var.copy(), "ret_count": self.ret_count,
                "ret_mean": self.ret_mean, "ret_var": self.ret_var, "returns": self.returns.copy()}

    def load(self, s):
        self.obs_count, self.ret_count = np.float64(s["obs_count"]), np.float64(s["ret_count"])
        self.ret_mean, self.ret_var = np.float64(s["ret_mean"]), np.float64(s["ret_var"])
        self.obs_mean, self.obs_var = np.array(s["obs_mean"], np.float64), np.array(s["obs_var"], np.float64)
        self.returns = np.array(s["returns"], np.float64)

    def _apply_obs(self, rows, vector_states, state_stack):
        if not self.obs:
            return
        den = np.sqrt(self.obs_var + self.eps)
        x = np.asarray(vector_states, np.float32)[rows].astype(np.float64)
        self.norm_vector_states[rows] = np.clip((x - self.obs_mean) / den, -self.clip_obs, self.clip_obs).astype(np.float32)
        if self.K:
            f = np.asarray(state_stack, np.float32)[rows].astype(np.float64)
            self.norm_state_stack[rows] = np.clip((f - self.obs_mean) / den, -self.clip_obs, self.clip_obs).astype(np.float32)

    def step(self, vector_states, rewards, is_clean, dones, state_stack=None):
        """a step chain: every row is covered, the rows with ``is_clean`` are the batch"""
        R = self.R
        rows = np.arange(R)
        clean = np.asarray(is_clean) != 0
        rewards = np.asarray(rewards, np.float64)
        new_ret = self.returns * self.gamma + rewards
        if self.training:
            cols = []
            if self.obs:
                cols.append(np.asarray(vector_states, np.float32).astype(np.float64))
            if self.reward:
                cols.append(new_ret[:, None])
            c, bm, m2 = batch_triple(np.concatenate(cols, axis=1), clean)
            if self.obs:
                self.obs_count, self.obs_mean, self.obs_var = merge(self.obs_count, self.obs_mean, self.obs_var, c, bm[:self.D], m2[:self.D])
            if self.reward:
                self.ret_count, self.ret_mean, self.ret_var = merge(self.ret_count, self.ret_mean, self.ret_var, c, bm[-1], m2[-1])
        self._apply_obs(rows, vector_states, state_stack)
        if self.reward:
            self.norm_rewards = np.clip(rewards / np.sqrt(self.ret_var + self.eps), -self.clip_reward, self.clip_reward)
            if self.training:
                self.returns = np.where(np.asarray(dones) != 0, 0.0, np.where(clean, new_ret, self.returns))

    def reset(self, rows, vector_states, state_stack=None):
        """a reset chain over ``rows`` (the chain's order): all of them count; their returns restart"""
        rows = np.asarray(rows, np.int64)
        if self.training and self.obs:
            x = np.asarray(vector_states, np.float32)[rows].astype(np.float64).reshape(len(rows), self.D)
            c, bm, m2 = batch_triple(x, np.ones(len(rows), bool))
            self.obs_count, self.obs_mean, self.obs_var = merge(self.obs_count, self.obs_mean, self.obs_var, c, bm, m2)
        if len(rows):
            self._apply_obs(rows, vector_states, state_stack)
        if self.training and self.reward:
            self.returns[rows] = 0.0
