"""The device-side action decoding (csrc/actions.h) and observation post-processing (csrc/obs_post.h) in numpy: the rules of
include/imgenv.h operation for operation, in the same number formats, so that the GPU tests can compare bit for bit.
tests/test_action_model.py holds this file to the reference's own recordings, to its code spelled out, and to the Python port.

Decoding, per robot row (VelActionWrapper.action, base.py:37-66; action.py:23-38):
  TABLE, integer raw   table[raw]; outside [0, n_table): (0, 0, 0), bad
  TABLE, float raw     float32(raw), beep 0 with two columns
  CLIP,  float raw     x = float32(raw); x = x >= lo ? x : lo; x = x <= hi ? x : hi  (lo, hi as float32)
  a component that is not finite, as it came or as float32: the row is (0, 0, 0), bad
  speeds = (v, w) where is_clean (MultiRobotCleanWrapper's state BEFORE the step, base.py:81-83), else (0, 0)
"""
import numpy as np

TABLE, CLIP = 0, 1
PED_NORM_AVG = np.array([0.0, 0.0, 0.0, 0.0, 0.25, 0.25, 0.0])   # base.py:20
PED_NORM_STD = np.array([6.0, 6.0, 0.6, 0.9, 0.50, 0.5, 6.0])    # base.py:21


def table_rows(discrete_actions):
    """DiscreteActions (action.py:25-32) as float32 [n, 3]: a two-column row gets beep 0"""
    return np.array([[r[0], r[1], r[2] if len(r) == 3 else 0] for r in discrete_actions], np.float32).reshape(-1, 3)


def decode(raw, mode, table=None, clip=None, n_cols=2):
    """-> (actions float32 [R, 3], bad bool [R])"""
    raw = np.asarray(raw)
    R = len(raw)
    out = np.zeros((R, 3), np.float32)
    if raw.dtype.kind in "iu":
        assert mode == TABLE and raw.ndim == 1
        k = raw.astype(np.int64)
        bad = (k < 0) | (k >= len(table))
        out[~bad] = table[k[~bad]]
        return out, bad
    assert raw.dtype in (np.float32, np.float64) and raw.shape == (R, n_cols)
    bad = ~np.isfinite(raw).all(axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        x = raw.astype(np.float32)
    if mode == CLIP:
        lo, hi = (np.asarray(clip, np.float64)[:n_cols, q].astype(np.float32) for q in (0, 1))
        x = np.where(x >= lo, x, lo)
        x = np.where(x <= hi, x, hi)
    bad |= ~np.isfinite(x).all(axis=1)
    out[:, :n_cols] = x
    out[bad] = 0
    return out, bad


class ActionModel:
    """the decode with MultiRobotCleanWrapper's state next to it: ``decode`` before a step, ``step_done`` with the step's dones
    behind it, ``reset`` for the rows of the envs that restarted"""

    def __init__(self, R, mode, table=None, clip=None, n_cols=2):
        self.R, self.mode, self.clip, self.n_cols = R, mode, clip, n_cols
        self.table = None if table is None else table_rows(table)
        self.is_clean = np.ones(R, bool)
        self.n_bad = 0
        self.masked_rows = 0  # rows whose speeds the mask zeroed so far
        self.actions = np.zeros((R, 3), np.float32)
        self.speeds = np.zeros((R, 2), np.float32)

    def decode(self, raw):
        self.actions, bad = decode(raw, self.mode, self.table, self.clip, self.n_cols)
        self.n_bad += int(bad.sum())
        self.speeds = np.where(self.is_clean[:, None], self.actions[:, :2], np.float32(0))
        self.masked_rows += int((~self.is_clean).sum())
        return self.actions

    def step_done(self, dones):
        self.is_clean = np.where(np.asarray(dones) > 0, False, self.is_clean)  # base.py:87

    def reset(self, rows):
        self.is_clean = np.where(np.asarray(rows, bool), True, self.is_clean)  # base.py:90-93, per env


def ped_norm(rows, max_ped, avg=PED_NORM_AVG, std=PED_NORM_STD):
    """StatePedVectorWrapper._normalize_ped_state (base.py:30-34) on float32 rows [R, 1 + 7 max_ped], not in place:
    n = min(int(row[0]), max_ped); element 1 + 7 j + c of pedestrian j < n becomes float32((float64(x) - avg[c]) / std[c])"""
    rows = np.asarray(rows)
    assert rows.dtype == np.float32 and rows.shape[1] == 1 + 7 * max_ped
    avg, std = np.asarray(avg, np.float64), np.asarray(std, np.float64)
    out = rows.copy()
    with np.errstate(invalid="ignore"):
        n = np.where(rows[:, 0] >= 1, np.minimum(rows[:, 0], np.float32(max_ped)), 0).astype(np.int64)
    body = rows[:, 1:].reshape(len(rows), max_ped, 7).astype(np.float64)
    normed = ((body - avg) / std).astype(np.float32)
    take = np.arange(max_ped)[None, :] < n[:, None]
    out[:, 1:] = np.where(take[:, :, None], normed, rows[:, 1:].reshape(len(rows), max_ped, 7)).reshape(len(rows), -1)
    return out


def close_to_human(ped_min_dists, close_dist=1.0):
    return (np.asarray(ped_min_dists, np.float64) < close_dist).astype(np.uint8)
