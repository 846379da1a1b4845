"""A numpy model of the sequence minibatches (img_env_amd/csrc/sequences.h, include/imgenv.h): the flag of every sequence, the
compaction of those that count, the order list, and the time-major gather with all its rules -- the zero and weight rule, mb_first,
the float32 normalisation, the per-slot sequence number, length and state rows.  R rows, horizon T, cursor n, chunk length L:
sequence q = c * R + row covers row ``row``'s transitions t = c * L .. min(c * L + L, n) - 1; k = t * R + row."""
import numpy as np

import minibatch_model as mm


def chunks(steps, L):
    return -(-steps // L)


def flags(is_clean, n, L):
    """seq_flag [C * R] uint8: 1 iff any covered transition has is_clean != 0; ``is_clean`` is [T, R]"""
    is_clean = np.asarray(is_clean)
    R, C = is_clean.shape[1], chunks(n, L)
    out = np.zeros((C, R), np.uint8)
    for c in range(C):
        out[c] = (is_clean[c * L:min(c * L + L, n)] != 0).any(axis=0)
    return out.reshape(-1)


def valid_list(is_clean, n, L):
    """the ascending q < C * R with the flag set"""
    return np.flatnonzero(flags(is_clean, n, L)).astype(np.int32)


def order_list(valid, S, seed):
    """seq_order [S = C_max * R]: valid[pi(p)] for p < Vs, -1 behind (the minibatches' pi over Vs)"""
    return mm.order_list(valid, S, seed)


def gather(order, j, Bs, L, n, R, fields, ring, is_clean, final_idx, scalars=(), normalise_index=None, norm=None, states=()):
    """Sequence minibatch j, time-major.  ``fields``: name -> array [slots, R, ...]; ``ring``: the ring's actions [T, R, 3], rewards,
    dones, dones_info [T, R]; ``is_clean`` [T, R]; ``final_idx`` [T + 1, R]; ``scalars``: the caller's [T or T + 1, R]; ``states``: the
    caller's [T or T + 1, R, ...].  Returns a dict of mb_* arrays ([L, Bs, ...]; mb_seq, mb_seq_len and mb_seq_state<a> per slot)."""
    order = np.asarray(order, np.int32)
    pos = j * Bs + np.arange(Bs, dtype=np.int64)
    q = np.where(pos < len(order), order[np.minimum(pos, len(order) - 1)], -1).astype(np.int32)
    q = np.where(q >= 0, q, -1).astype(np.int32)
    c, row = np.where(q >= 0, q // R, 0), np.where(q >= 0, q % R, 0)
    t = c[None, :] * L + np.arange(L)[:, None]                       # [L, Bs]
    ok = (q[None, :] >= 0) & (t < n)
    k = np.where(ok, t * R + row[None, :], -1).astype(np.int32)
    kk = np.where(ok, k, 0)
    clean = np.asarray(is_clean).reshape(-1)
    fidx = np.asarray(final_idx).reshape(-1)
    out = {"mb_index": k, "mb_weight": (ok & (clean[kk] != 0)).astype(np.float32), "mb_first": (ok & (fidx[kk] >= 0)).astype(np.uint8),
           "mb_seq": q, "mb_seq_len": np.where(q >= 0, np.clip(n - c * L, 0, L), 0).astype(np.int32)}
    for group in (fields, ring):
        for name, a in group.items():
            a = np.asarray(a)
            rows = a.reshape((-1,) + a.shape[2:])[kk].copy()
            rows[~ok] = 0
            out["mb_" + name] = rows
    sc = np.zeros((len(scalars), L, Bs), np.float32)
    for s, a in enumerate(scalars):
        v = np.asarray(a, np.float32).reshape(-1)[kk]
        if normalise_index is not None and s == normalise_index:
            v = mm.normalise(v, norm)
        sc[s] = np.where(ok, v, np.float32(0))
    out["mb_scalars"] = sc
    k0 = np.where(ok[0], k[0], 0)
    for a, st in enumerate(states):
        st = np.ascontiguousarray(st)
        rows = st.reshape(st.shape[0] * st.shape[1], -1).view(np.uint8)[k0].copy()
        rows[~ok[0]] = 0
        out["mb_seq_state%d" % a] = rows
    return out
