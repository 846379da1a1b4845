"""The rollout storage (include/imgenv.h: imgenv_rollout_*; img_env_amd/csrc/rollout.h) in numpy: what the ring, the final list and
the advantage pass hold after a recorded list of chains.  No GPU, no library: the tests compare the library, and the header's host
functions, against this.

A chain is a dict:
  {"kind": "step", "obs": {field: [R, ...]}, "actions": [R, 3], "rewards": float64 [R], "dones": [R], "is_clean": [R], "dones_info": [R]}
  {"kind": "reset", "rows": the robot rows the chain covers, in the chain's order, "obs": {field: [R, ...]}}
``obs`` is every stored field's live array AFTER the chain.
"""
import numpy as np


def replay(horizon, final_capacity, first_obs, chains):
    """the arrays after ``imgenv_rollout_begin`` on the observation ``first_obs`` followed by ``chains``; unwritten parts are zero
    (``final_idx``: -1), as in a ring that was enabled and begun once"""
    T, F = int(horizon), int(final_capacity)
    R = len(next(iter(first_obs.values())))
    r = {"n": 0, "resets": 0}
    for name, a in first_obs.items():
        a = np.asarray(a)
        r["obs_" + name] = np.zeros((T + 1,) + a.shape, a.dtype)
        r["final_" + name] = np.zeros((F,) + a.shape[1:], a.dtype)
        r["obs_" + name][0] = a
    r["actions"] = np.zeros((T, R, 3), np.float32)
    r["rewards"] = np.zeros((T, R), np.float32)
    r["dones"] = np.zeros((T, R), np.uint8)
    r["is_clean"] = np.zeros((T, R), np.uint8)
    r["dones_info"] = np.zeros((T, R), np.int32)
    r["final_idx"] = np.full((T + 1, R), -1, np.int32)
    r["final_slot"] = np.zeros(F, np.int32)
    r["final_row"] = np.zeros(F, np.int32)
    final_n = [0, 0]  # the two words, in turns
    for c in chains:
        n = r["n"]
        if c["kind"] == "step":
            assert n < T, "rollout full: imgenv_rollout_begin"
            r["actions"][n] = np.asarray(c["actions"], np.float32).reshape(R, 3)
            r["rewards"][n] = np.asarray(c["rewards"], np.float64).astype(np.float32)  # rounded once
            r["dones"][n] = np.asarray(c["dones"]).astype(np.uint8)
            r["is_clean"][n] = np.asarray(c["is_clean"]).astype(np.uint8)
            r["dones_info"][n] = np.asarray(c["dones_info"]).astype(np.int32)
            for name in first_obs:
                r["obs_" + name][n + 1] = c["obs"][name]
            r["n"] = n + 1
        else:
            k = r["resets"]
            base = final_n[k & 1]
            rows = [int(x) for x in c["rows"]]
            for m, row in enumerate(rows):
                e = base + m
                if e < F:
                    for name in first_obs:
                        r["final_" + name][e] = r["obs_" + name][n, row]
                    r["final_slot"][e], r["final_row"][e] = n, row
                r["final_idx"][n, row] = e
                for name in first_obs:
                    r["obs_" + name][n, row] = np.asarray(c["obs"][name])[row]
            final_n[(k + 1) & 1] = base + len(rows)
            r["resets"] = k + 1
    r["final_n"] = np.array(final_n, np.int32)
    r["final_count"] = final_n[r["resets"] & 1]
    return r


def gae(r, values, final_values, gamma, lam, final_capacity, adv=None, ret=None):
    """``imgenv_rollout_gae`` over the arrays ``r`` (``replay``'s, or the library's as numpy): float32 scalars in the header's order"""
    f32 = np.float32
    n = int(r["n"])
    values = np.asarray(values, f32)
    T1, R = values.shape
    adv = np.zeros((T1 - 1, R), f32) if adv is None else np.array(adv, f32)
    ret = np.zeros((T1 - 1, R), f32) if ret is None else np.array(ret, f32)
    gamma, lam, zero = f32(gamma), f32(lam), f32(0.0)
    gl = f32(gamma * lam)
    for row in range(R):
        g = zero
        for t in range(n - 1, -1, -1):
            e = int(r["final_idx"][t + 1, row])
            done = bool(r["dones"][t, row])
            terminal = done and int(r["dones_info"][t, row]) != 10
            if terminal:
                nv = zero
            elif e >= 0:
                nv = f32(final_values[e]) if (e < final_capacity and final_values is not None) else zero
            else:
                nv = values[t + 1, row]
            cont = not (done or e >= 0)
            if not r["is_clean"][t, row]:
                adv[t, row] = ret[t, row] = g = zero
                continue
            m = f32(gamma * nv)
            s = f32(f32(r["rewards"][t, row]) + m)
            delta = f32(s - values[t, row])
            c = f32(gl * g)
            c = c if cont else zero
            g = f32(delta + c)
            adv[t, row] = g
            ret[t, row] = f32(g + values[t, row])
    return adv, ret
