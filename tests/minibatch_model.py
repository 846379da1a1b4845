"""A numpy model of the rollout minibatches (img_env_amd/csrc/minibatch.h, include/imgenv.h): the compaction of the transitions
that count, the shuffle's permutation pi, the order list, the gather of a minibatch with its zero and weight rule, the float32
normalisation, and the statistics with the kernels' order of partial sums.  k = t * R + row numbers the stored transitions."""
import numpy as np

M32 = 0xFFFFFFFF
ROUNDS = 6
STATS_BLOCK, STATS_PER_LANE = 256, 16
STATS_TILE = STATS_BLOCK * STATS_PER_LANE


def valid_list(is_clean, n):
    """the ascending k < n * R with is_clean != 0; ``is_clean`` is [T, R]"""
    return np.flatnonzero(np.asarray(is_clean)[:n].reshape(-1) != 0).astype(np.int32)


def fmix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def keys(seed_lo, seed_hi):
    return [fmix((seed_lo & M32) ^ ((r * 0x9E3779B9) & M32)) ^ (seed_hi & M32) for r in range(ROUNDS)]


def split_seed(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & M32, seed >> 32


def perm(V, x, key, count=None):
    """pi(x) for one x < V, in Python integers.  ``count``: a one-element list that receives the number of six-round passes"""
    if V <= 1:
        return x
    b = max(2, (V - 1).bit_length())
    hb = b // 2
    ha = b - hb
    mA, mB = (1 << ha) - 1, (1 << hb) - 1
    passes = 0
    while True:
        L, R = x >> hb, x & mB
        for r in range(ROUNDS):
            if r % 2 == 0:
                L ^= fmix((R + key[r]) & M32) & mA
            else:
                R ^= fmix((L + key[r]) & M32) & mB
        x = (L << hb) | R
        passes += 1
        if x < V:
            break
    if count is not None:
        count[0] = max(count[0], passes)
    return x


def _fmix_v(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x85EBCA6B)
    x = x ^ (x >> np.uint32(13))
    x = x * np.uint32(0xC2B2AE35)
    return x ^ (x >> np.uint32(16))


def perm_all(V, key):
    """pi(0 .. V - 1) as a uint32 array, vectorised (uint32 arithmetic wraps)"""
    x = np.arange(V, dtype=np.uint32)
    if V <= 1:
        return x
    b = max(2, (V - 1).bit_length())
    hb = np.uint32(b // 2)
    ha = np.uint32(b - b // 2)
    mA, mB = np.uint32((1 << int(ha)) - 1), np.uint32((1 << int(hb)) - 1)
    k = [np.uint32(v) for v in key]
    todo = np.ones(V, bool)
    with np.errstate(over="ignore"):
        while todo.any():
            y = x[todo]
            L, R = y >> hb, y & mB
            for r in range(ROUNDS):
                if r % 2 == 0:
                    L = L ^ (_fmix_v(R + k[r]) & mA)
                else:
                    R = R ^ (_fmix_v(L + k[r]) & mB)
            x[todo] = (L << hb) | R
            todo &= x >= V
    return x


def order_list(valid, TR, seed):
    """order [TR]: valid[pi(p)] for p < V, -1 behind"""
    V = len(valid)
    order = np.full(TR, -1, np.int32)
    if V:
        order[:V] = np.asarray(valid, np.int32)[perm_all(V, keys(*split_seed(seed)))]
    return order


def normalise(x, norm):
    """(x - norm[0]) * norm[1] in float32, two roundings"""
    x, norm = np.asarray(x, np.float32), np.asarray(norm, np.float32)
    return ((x - norm[0]).astype(np.float32) * norm[1]).astype(np.float32)


def gather(order, j, B, fields, ring_scalars, scalars=(), normalise_index=None, norm=None):
    """Minibatch j.  ``fields``: name -> array [slots, R, ...] (k indexes the flattened first two axes); ``ring_scalars``: the ring's
    actions [T, R, 3], rewards, dones, dones_info [T, R]; ``scalars``: the caller's arrays [T or T + 1, R].  Returns a dict of mb_* arrays."""
    order = np.asarray(order, np.int32)
    pos = j * B + np.arange(B, dtype=np.int64)
    k = np.where(pos < len(order), order[np.minimum(pos, len(order) - 1)], -1).astype(np.int32)
    ok = k >= 0
    kk = np.where(ok, k, 0)
    out = {"mb_index": np.where(ok, k, -1).astype(np.int32), "mb_weight": ok.astype(np.float32)}
    for name, a in fields.items():
        flat = np.asarray(a).reshape((-1,) + a.shape[2:])
        rows = flat[kk].copy()
        rows[~ok] = 0
        out["mb_" + name] = rows
    for name, a in ring_scalars.items():
        a = np.asarray(a)
        flat = a.reshape((-1,) + a.shape[2:])
        rows = flat[kk].copy()
        rows[~ok] = 0
        out["mb_" + name] = rows
    sc = np.zeros((len(scalars), B), np.float32)
    for s, a in enumerate(scalars):
        v = np.asarray(a, np.float32).reshape(-1)[kk]
        if normalise_index is not None and s == normalise_index:
            v = normalise(v, norm)
        sc[s] = np.where(ok, v, np.float32(0))
    out["mb_scalars"] = sc
    return out


def fold(a):
    """the workgroup's fold of STATS_BLOCK float64 lane sums: a[l] += a[l + half], half = 128 .. 1"""
    a = np.array(a, np.float64)
    half = STATS_BLOCK // 2
    while half:
        a[:half] = a[:half] + a[half:2 * half]
        half //= 2
    return float(a[0])


def _tile_sums(v, n_tiles):
    """per tile: lane l adds v[tile + i * BLOCK + l], i ascending; then the fold"""
    V = len(v)
    pad = np.zeros(n_tiles * STATS_TILE, np.float64)
    pad[:V] = v
    pad = pad.reshape(n_tiles, STATS_PER_LANE, STATS_BLOCK)
    parts = np.zeros(n_tiles, np.float64)
    for t in range(n_tiles):
        acc = np.zeros(STATS_BLOCK, np.float64)
        for i in range(STATS_PER_LANE):  # (adding the +0.0 of a missing position changes no bit of a sum that started at +0.0)
            acc = acc + pad[t, i]
        parts[t] = fold(acc)
    return parts


def _reduce(parts):
    acc = np.zeros(STATS_BLOCK, np.float64)
    for q in range(0, len(parts), STATS_BLOCK):
        chunk = parts[q:q + STATS_BLOCK]
        acc[:len(chunk)] = acc[:len(chunk)] + chunk
    return fold(acc)


def stats(x, valid, total, eps):
    """(float32 mean, float32 1 / sqrt(var + eps)) with the kernels' order of sums; ``total`` = n * R sizes the tiles"""
    V = len(valid)
    if V == 0:
        return np.array([0.0, 1.0], np.float32)
    n_tiles = max(1, -(-total // STATS_TILE))
    v = np.asarray(x, np.float32).reshape(-1)[np.asarray(valid)].astype(np.float64)
    mean = _reduce(_tile_sums(v, n_tiles)) / V
    d = v - mean
    var = _reduce(_tile_sums(d * d, n_tiles)) / V
    s = var + float(eps)
    return np.array([np.float32(mean), np.float32(1.0) if s == 0.0 else np.float32(1.0 / np.sqrt(s))], np.float32)
