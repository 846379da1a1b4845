"""The track bank's rules in numpy (include/imgenv.h, "track bank"; img_env_amd/csrc/track_bank.h): which set a world takes at
each reset under IMGENV_TRACKS_KEEP / BY_PLACEMENT / CYCLE, and the tables the world then holds.  Used by
tests/test_tracks_model.py (without a GPU) and tests/test_gpu_track_bank.py (as the expectation of ``world_tracks()``)."""
import numpy as np

M64 = (1 << 64) - 1
SALT = 0xBB67AE8584CAA73B  # the fractional bits of sqrt(3)
KEEP, BY_PLACEMENT, CYCLE = 0, 1, 2
POLICIES = {"keep": KEEP, "placement": BY_PLACEMENT, "cycle": CYCLE}


def map_for_placement(seed, n):
    """csrc/map_bank.h: splitmix64's finaliser, the upper 32 bits scaled into [0, n) by multiply-shift"""
    if n <= 1:
        return 0
    z = (seed + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return ((z >> 32) * n) >> 32


def tracks_for_placement(seed, n_sets):
    return map_for_placement((seed + SALT) & M64, n_sets)


def tracks_for_cycle(e, repeat, n_sets):
    """PedTrajectoryDatasetWrapper: cur_world moves on after repeated_time_per_env episodes -- wrapping where the reference exits"""
    return (e // repeat) % n_sets


class TracksModel:
    """cur / next / count of every world, as k_tracks_install keeps them"""

    def __init__(self, n_worlds, n_sets, policy="keep", repeat=1):
        self.n_sets = n_sets
        self.cur = np.full(n_worlds, -1, np.int32)
        self.next = np.zeros(n_worlds, np.int32)
        self.count = np.zeros(n_worlds, np.int64)
        self.set_policy(policy, repeat)

    def set_policy(self, policy, repeat=1):
        if repeat < 1:
            raise ValueError("repeat")
        self.policy, self.repeat = POLICIES[policy], repeat
        self.count[:] = 0

    def select(self, worlds, ids):
        for k, s in zip(worlds, ids):
            self.next[k] = s

    def reset(self, world, seed=None):
        """a bank-fed reset of ``world``; ``seed``: the placement's 64-bit seed where the reset has one"""
        if self.policy == CYCLE:
            s = tracks_for_cycle(int(self.count[world]), self.repeat, self.n_sets)
        elif self.policy == BY_PLACEMENT and seed is not None:
            s = tracks_for_placement(seed & M64, self.n_sets)
        else:
            s = int(self.next[world])
        self.cur[world] = self.next[world] = s
        self.count[world] += 1
        return s

    def reset_explicit(self, world):
        """a reset whose batch brought its own tracks: no set, no count"""
        self.cur[world] = -1


def installed_tables(pose, traj, traj_v, length, stride=None):
    """what a world holds after the install of one set (``_cabi.pack_track_sets`` arrays of that set): pose3 [P, 3], traj and traj_v
    [P, stride, 3] with the yaw of the velocity as third column, records behind a pedestrian's length zero, len [P]"""
    P, cap = traj.shape[0], traj.shape[1]
    stride = max(cap, 2) if stride is None else stride
    t, v = np.zeros((P, stride, 3)), np.zeros((P, stride, 3))
    for j in range(P):
        n = int(length[j])
        t[j, :n] = traj[j, :n]
        v[j, :n, :2] = traj_v[j, :n]
        v[j, :n, 2] = np.arctan2(traj_v[j, :n, 1], traj_v[j, :n, 0])
    yaw = np.arctan2(2 * pose[:, 2] * pose[:, 3], pose[:, 3] ** 2 - pose[:, 2] ** 2)  # (of a unit quaternion; the library goes through tf's matrix)
    return np.stack([pose[:, 0], pose[:, 1], yaw], 1), t, v, np.asarray(length, np.int32).copy()


def replayed_state(pose3, traj, traj_v, length, step):
    """ped_state [P, 4] ``step`` moves after the install (img_env.cpp:361-386: record min(step - 1, len - 1)); step 0: the start
    pose, velocities unknown (they persist across resets) -> NaN"""
    P = traj.shape[0]
    out = np.full((P, 4), np.nan)
    if step == 0:
        out[:, :2] = pose3[:, :2]
        return out
    for j in range(P):
        i = min(step - 1, int(length[j]) - 1)
        out[j] = [traj[j, i, 0], traj[j, i, 1], traj_v[j, i, 0], traj_v[j, i, 1]]
    return out
