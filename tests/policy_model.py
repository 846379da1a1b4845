"""The policy head (csrc/policy.h; include/imgenv.h: imgenv_policy_enable) in numpy, without the library:

  * Philox4x32-10 in uint64 integer arithmetic, and the two exact conversions to a uniform float32;
  * the float32 restatement of the categorical row -- the lane blocks, the sums, the scan and the pick in the kernel's fixed order,
    vectorised over rows -- which gives the kernel's bits for given e[] (expf and logf are the platform's, everything else IEEE);
  * the float32 restatement of the Gaussian row;
  * float64 "truth" for probabilities, log-probabilities, entropies and z, which the GPU tests bound the kernel's error against.
"""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
POL_REG = 16
F32 = np.float32
TWO_PI = F32(6.2831855)
HALF_LN_2PI = F32(0.9189385)
ENT_CONST = F32(1.4189385)
INT_MAX = 2 ** 31 - 1


def philox(ctr, key):
    """ctr [..., 4], key [..., 2] (anything that fits uint32) -> uint32 [..., 4]; ten rounds in uint64 arithmetic"""
    c = [np.asarray(ctr, np.uint64)[..., q] & np.uint64(MASK) for q in range(4)]
    k = [np.asarray(key, np.uint64)[..., q] & np.uint64(MASK) for q in range(2)]
    c = list(np.broadcast_arrays(*c, *k))
    k, c = c[4:], c[:4]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & np.uint64(MASK), (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & np.uint64(MASK)]
        k = [(k[0] + np.uint64(W0)) & np.uint64(MASK), (k[1] + np.uint64(W1)) & np.uint64(MASK)]
    return np.stack(c, axis=-1).astype(np.uint32)


def draw_block(g, draw, seed, second=False):
    """robot g's block of draw number `draw` under `seed` (g: array of global robot numbers) -> uint32 [len(g), 4]"""
    g = np.asarray(g, np.uint64)
    draw, seed = int(draw) & (2 ** 64 - 1), int(seed) & (2 ** 64 - 1)
    hi = (draw >> 32) ^ (0x80000000 if second else 0)
    ctr = np.stack([g & np.uint64(MASK), g >> np.uint64(32), np.full_like(g, draw & MASK), np.full_like(g, hi)], axis=-1)
    return philox(ctr, np.array([seed & MASK, seed >> 32], np.uint64))


def u01(x):
    """[0, 1): float32(x >> 8) * 2^-24, exact"""
    return (np.asarray(x, np.uint32) >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)


def u01_open(x):
    """(0, 1]: float32((x >> 8) + 1) * 2^-24, exact"""
    return ((np.asarray(x, np.uint32) >> np.uint32(8)) + np.uint32(1)).astype(F32) * F32(2.0 ** -24)


def group(A):
    """lanes per robot (launch_plan.h: plan_policy_group)"""
    return 1 if A <= POL_REG else 4 if A <= 4 * POL_REG else 16 if A <= 16 * POL_REG else 64


def block(A, G, j):
    """(k0, n): lane j of G owns logits [k0, k0 + n)"""
    per = -(-A // G)
    k0 = j * per
    return k0, min(max(A - k0, 0), per)


def launch(R, A):
    """(grid, block) of the categorical launch over R local robots"""
    return -(-R * group(A) // 256), 256


def bad_rows(logits):
    logits = np.asarray(logits, F32)
    with np.errstate(invalid="ignore"):
        return np.isnan(logits).any(axis=1) | (logits == np.inf).any(axis=1) | ~np.isfinite(logits).any(axis=1)


def categorical_f32(logits, u, deterministic=False, e=None, G=None):
    """The kernel's order in float32 on rows [R, A] with uniforms u [R]: dict of index (int32, -1 bad), logp, entropy, s, target,
    part [R, G], scan [R, G] (the inclusive scan), bad.  `e`: given e[] [R, A] instead of exp(l - m) (then bit for bit the
    kernel's sums, scan and index)."""
    l = np.asarray(logits, F32)
    R, A = l.shape
    G = group(A) if G is None else G
    per = -(-A // G)
    pad = G * per - A
    bad = bad_rows(l)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.where(np.isnan(l), -np.inf, l).max(axis=1).astype(F32)
        if e is None:
            e = np.where(l == -np.inf, F32(0), np.exp(l - m[:, None]).astype(F32)).astype(F32)
        e = np.asarray(e, F32)
        lp = np.pad(l, ((0, 0), (0, pad)), constant_values=-np.inf).reshape(R, G, per)
        ep = np.pad(e, ((0, 0), (0, pad)), constant_values=0).reshape(R, G, per)
        part = np.zeros((R, G), F32)
        for i in range(per):
            part = part + ep[:, :, i]
        P = part.copy()
        d = 1
        while d < G:
            Q = P.copy()
            Q[:, d:] = P[:, d:] + P[:, :-d]
            P, d = Q, d * 2
        s = P[:, -1]
        X = np.concatenate([np.zeros((R, 1), F32), P[:, :-1]], axis=1)
        target = (np.asarray(u, F32) * s).astype(F32)
        log_s = np.log(s).astype(F32)
        c = X.copy()
        cand = np.full((R, G), INT_MAX, np.int64)
        last = np.full((R, G), -1, np.int64)
        ent = np.zeros((R, G), F32)
        k0 = (np.arange(G) * per)[None, :]
        for i in range(per):
            ei, li = ep[:, :, i], lp[:, :, i]
            pos = ei > 0
            c = np.where(pos, c + ei, c).astype(F32)
            hit = pos & ((li == m[:, None]) if deterministic else (c > target[:, None]))
            cand = np.where(hit & (cand == INT_MAX), k0 + i, cand)
            last = np.where(pos, k0 + i, last)
            t = (ei / s[:, None]).astype(F32) * ((li - m[:, None]).astype(F32) - log_s[:, None]).astype(F32)
            ent = np.where(pos, ent + t.astype(F32), ent).astype(F32)
        H, d, lanes = ent, 1, np.arange(G)
        while d < G:
            H, d = (H + H[:, lanes ^ d]).astype(F32), d * 2
        cmin, lmax = cand.min(axis=1), last.max(axis=1)
        index = np.where(cmin != INT_MAX, cmin, lmax)
        safe = np.clip(index, 0, A - 1)
        logp = ((l[np.arange(R), safe] - m).astype(F32) - log_s).astype(F32)
        entropy = (F32(0) - H[:, 0]).astype(F32)
    index = np.where(bad, -1, index).astype(np.int32)
    return dict(index=index, logp=np.where(bad, F32(0), logp).astype(F32), entropy=np.where(bad, F32(0), entropy).astype(F32),
                s=s, target=target, part=part, scan=P, bad=bad, e=e, m=m)


def categorical_truth(logits):
    """float64: dict of p [R, A], logp [R, A] (-inf where masked), entropy [R], cdf [R, A] (inclusive), bad [R]"""
    l = np.asarray(logits, F32).astype(np.float64)
    bad = bad_rows(logits)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.where(np.isnan(l), -np.inf, l).max(axis=1)
        z = l - m[:, None]
        e = np.where(l == -np.inf, 0.0, np.exp(z))
        s = e.sum(axis=1)
        logp = z - np.log(s)[:, None]
        p = e / s[:, None]
        entropy = -np.where(p > 0, p * logp, 0.0).sum(axis=1)
    return dict(p=p, logp=logp, entropy=entropy, cdf=np.cumsum(p, axis=1), bad=bad)


def box_muller_f32(x0, x1):
    u1, u2 = u01_open(x0), u01(x1)
    rho = np.sqrt(F32(-2.0) * np.log(u1).astype(F32)).astype(F32)
    ang = (TWO_PI * u2).astype(F32)
    return (rho * np.cos(ang).astype(F32)).astype(F32), (rho * np.sin(ang).astype(F32)).astype(F32)


def box_muller_truth(x0, x1):
    """float64 z0, z1 of the exact uniforms and the exact 2 pi"""
    u1, u2 = u01_open(x0).astype(np.float64), u01(x1).astype(np.float64)
    rho = np.sqrt(-2.0 * np.log(u1))
    return rho * np.cos(2.0 * np.pi * u2), rho * np.sin(2.0 * np.pi * u2)


def normals(g, draw, seed, C, truth=False):
    """z [R, C] of robots g: columns 0, 1 from the first block, column 2 the z0 of the second"""
    bm = box_muller_truth if truth else box_muller_f32
    x = draw_block(g, draw, seed)
    z0, z1 = bm(x[:, 0], x[:, 1])
    cols = [z0, z1]
    if C > 2:
        y = draw_block(g, draw, seed, second=True)
        cols.append(bm(y[:, 0], y[:, 1])[0])
    return np.stack(cols[:C], axis=1)


def _per_row(log_std, R, C, dtype):
    return np.broadcast_to(np.asarray(log_std, F32).astype(dtype).reshape(-1, C), (R, C))


def gaussian_f32(mean, log_std, z):
    """the kernel's order in float32: dict of raw [R, C], logp, entropy, bad (z: float32 [R, C]; zeros for DETERMINISTIC)"""
    mu = np.asarray(mean, F32)
    R, C = mu.shape
    ls, z = _per_row(log_std, R, C, F32), np.asarray(z, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        sigma = np.exp(ls).astype(F32)
        raw = (mu + (sigma * z).astype(F32)).astype(F32)
        bad = ~(np.isfinite(mu) & np.isfinite(ls) & np.isfinite(sigma) & np.isfinite(raw)).all(axis=1)
        logp, ent = np.zeros(R, F32), np.zeros(R, F32)
        for c in range(C):
            logp = (logp + ((((F32(-0.5) * z[:, c]).astype(F32) * z[:, c]).astype(F32) - ls[:, c]).astype(F32) - HALF_LN_2PI).astype(F32)).astype(F32)
            ent = (ent + (ENT_CONST + ls[:, c]).astype(F32)).astype(F32)
    raw = np.where(bad[:, None], F32(0), raw).astype(F32)
    return dict(raw=raw, logp=np.where(bad, F32(0), logp).astype(F32), entropy=np.where(bad, F32(0), ent).astype(F32), bad=bad)


def gaussian_truth(mean, log_std, z):
    """float64 on the float32 inputs and a float64 z"""
    mu = np.asarray(mean, F32).astype(np.float64)
    R, C = mu.shape
    ls, z = _per_row(log_std, R, C, np.float64), np.asarray(z, np.float64)
    raw = mu + np.exp(ls) * z
    logp = (-0.5 * z * z - ls - 0.5 * np.log(2.0 * np.pi)).sum(axis=1)
    ent = (0.5 + 0.5 * np.log(2.0 * np.pi) + ls).sum(axis=1)
    return dict(raw=raw, logp=logp, entropy=ent)


def entropy_scale(log_std, R, C):
    """What "2^-21 relative" of the Gaussian entropy is relative to: the sum of the magnitudes of the 2 C numbers it adds up, the
    constant and log_std of every column.  log_std from -5 to 1 gives summands of both signs, and no float32 sum -- the float32
    constant alone is off by 3e-8 -- is accurate relative to a result that cancelled."""
    return (0.5 + 0.5 * np.log(2.0 * np.pi) + np.abs(_per_row(log_std, R, C, np.float64))).sum(axis=1)


def make_logits(rng, R, A, scale, masked=0.2):
    """test rows: normal logits times `scale`, `masked` of them -inf, column 0 never masked"""
    l = (rng.standard_normal((R, A)) * scale).astype(F32)
    mask = rng.random((R, A)) < masked
    mask[:, 0] = False
    l[mask] = -np.inf
    return l


def margin(A):
    return (A + 8) * 2.0 ** -23
