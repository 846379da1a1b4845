"""The rule of the device-side episode statistics (include/imgenv.h: imgenv_episodes_enable; csrc/episodes.h) in numpy: per robot,
float64 / int32, the operations of the kernel in the kernel's order -- elementwise IEEE arithmetic, so the GPU tests compare bit
patterns.  It is the repository's ``TestEpisodeWrapper`` / ``EpisodeStats`` (img_env_amd/envs.py) per robot with its own reset
per robot, plus the episode's return and length; tests/test_episode_model.py holds it to the reference's own recording."""
import numpy as np

ENDS = ("arrive", "timeout", "static_collision", "ped_collision", "other_collision", "aborted")
FIGURES = ("w_variance", "w_zero", "v_acc", "w_acc", "v_jerk", "w_jerk", "v_avg", "w_avg")
OPEN_F64 = ("n", "sum_v", "sum_w", "sum_ww", "sum_absw", "acc_v", "acc_w", "jerk_v", "jerk_w", "prev_v", "prev_w", "prev2_v", "prev2_w",
            "w_zero", "ep_return")
PATH_ROWS = 14  # the rows of OPEN_F64 that restart with a counted episode only
INT_TOTALS = ("episodes", "short_episodes", "speed_steps", "arrive_steps", "len_sum", "last_code", "last_steps", "last_len", "last_episode")
F64_TOTALS = ("v_sum", "w_sum", "return_sum", "last_return")


def end_bin(codes):
    """dones_info -> row of ``ends``: 5 arrive, 10 time-out, 1 / 2 / 3 the collision classes, anything else aborted"""
    codes = np.asarray(codes)
    return np.where(codes == 5, 0, np.where(codes == 10, 1, np.where((codes >= 1) & (codes <= 3), 1 + codes, 5)))


def round4(x):
    return np.rint(x * 1e4) / 1e4


class EpisodeModel:
    def __init__(self, n, dt, min_steps=3):
        self.n, self.dt, self.min_steps = int(n), np.float64(dt), int(min_steps)
        self.open = np.zeros(n, np.int32)
        self.log = []  # model only: one (rows, figures [8][n]) per fold that counted something
        self.clear()

    def clear(self):
        """imgenv_episodes_clear: everything but ``open``"""
        n = self.n
        self.open_f64 = np.zeros((len(OPEN_F64), n), np.float64)
        self.open_steps, self.open_len = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.ends = np.zeros((len(ENDS), n), np.int32)
        self.figure_sums = np.zeros((len(FIGURES), n), np.float64)
        for k in INT_TOTALS:
            setattr(self, k, np.zeros(n, np.int32))
        for k in F64_TOTALS:
            setattr(self, k, np.zeros(n, np.float64))

    def step(self, actions, is_clean, rewards):
        """a step of every robot: ``actions`` float32 [n, >= 2] (v, w, ...), the step's ``step_is_clean`` and ``step_rewards``"""
        actions = np.asarray(actions)
        assert actions.dtype == np.float32
        clean = np.asarray(is_clean).astype(bool)
        v = np.where(clean, actions[:, 0].astype(np.float64), 0.0)
        w = np.where(clean, actions[:, 1].astype(np.float64), 0.0)
        self.step_speeds(v, w, clean, rewards)

    def step_speeds(self, v, w, clean, rewards):
        v, w, rewards = np.asarray(v, np.float64), np.asarray(w, np.float64), np.asarray(rewards, np.float64)
        clean = np.asarray(clean).astype(bool)
        on = self.open != 0
        f = dict(zip(OPEN_F64, self.open_f64.copy()))
        dt, n = self.dt, f["n"]
        has1, has2 = n >= 1.0, n >= 2.0
        steps = self.open_steps + 1
        v_sum, w_sum = self.v_sum + v, self.w_sum + np.abs(w)
        for k, x in (("v", v), ("w", w)):
            acc = (x - f["prev_" + k]) / dt
            acc_prev = (f["prev_" + k] - f["prev2_" + k]) / dt
            f["acc_" + k] = f["acc_" + k] + np.where(has1, np.abs(acc), 0.0)
            f["jerk_" + k] = f["jerk_" + k] + np.where(has2, np.abs((acc - acc_prev) / dt), 0.0)
        last = f["prev_w"]
        turn = ((w == 0) & (last != 0)) | ((w > 0) & (last < 0)) | ((w < 0) & (last > 0))
        f["w_zero"] = f["w_zero"] + np.where(turn, 1.0, 0.0)
        f["prev2_v"], f["prev2_w"] = f["prev_v"], f["prev_w"]
        f["prev_v"], f["prev_w"] = v, w
        f["n"] = n + 1.0
        f["sum_v"] = f["sum_v"] + v
        f["sum_w"] = f["sum_w"] + w
        f["sum_ww"] = f["sum_ww"] + w * w
        f["sum_absw"] = f["sum_absw"] + np.abs(w)
        f["ep_return"] = f["ep_return"] + rewards
        new = np.stack([f[k] for k in OPEN_F64])
        self.open_f64 = np.where(on, new, self.open_f64)
        self.open_steps = np.where(on, steps, self.open_steps).astype(np.int32)
        self.open_len = np.where(on, self.open_len + clean.astype(np.int32), self.open_len).astype(np.int32)
        self.v_sum, self.w_sum = np.where(on, v_sum, self.v_sum), np.where(on, w_sum, self.w_sum)

    def reset(self, rows, codes):
        """a reset chain over the robots ``rows`` (bool [n]); ``codes`` = the last step's ``step_dones_info`` [n]"""
        rows, codes = np.asarray(rows).astype(bool), np.asarray(codes).astype(np.int32)
        was_open = rows & (self.open != 0)
        counted = was_open & (self.open_steps > self.min_steps)
        short = was_open & ~counted
        f = dict(zip(OPEN_F64, self.open_f64))
        n = f["n"]
        n0, n1, n2 = np.maximum(n, 1.0), np.maximum(n - 1.0, 1.0), np.maximum(n - 2.0, 1.0)
        mean_w = f["sum_w"] / n0
        fig = np.stack([round4(f["sum_ww"] / n0 - mean_w * mean_w), f["w_zero"], round4(f["acc_v"] / n1), round4(f["acc_w"] / n1),
                        round4(f["jerk_v"] / n2), round4(f["jerk_w"] / n2), round4(f["sum_v"] / n0), round4(f["sum_absw"] / n0)])
        c = counted.astype(np.int32)
        bins = end_bin(codes)
        for b in range(len(ENDS)):
            self.ends[b] += c * (bins == b)
        self.episodes = self.episodes + c
        self.short_episodes = self.short_episodes + short.astype(np.int32)
        self.speed_steps = self.speed_steps + c * self.open_steps
        self.arrive_steps = self.arrive_steps + c * (codes == 5) * self.open_steps
        self.figure_sums = np.where(counted, self.figure_sums + fig, self.figure_sums)
        self.return_sum = np.where(counted, self.return_sum + f["ep_return"], self.return_sum)
        self.len_sum = self.len_sum + c * self.open_len
        self.last_return = np.where(counted, f["ep_return"], self.last_return)
        self.last_code = np.where(counted, codes, self.last_code)
        self.last_steps = np.where(counted, self.open_steps, self.last_steps)
        self.last_len = np.where(counted, self.open_len, self.last_len)
        self.last_episode = np.where(counted, self.episodes, self.last_episode)
        if counted.any():
            self.log.append((counted.copy(), fig.copy()))
        self.open_f64[:PATH_ROWS] = np.where(counted, 0.0, self.open_f64[:PATH_ROWS])
        self.open_f64[PATH_ROWS] = np.where(rows, 0.0, self.open_f64[PATH_ROWS])
        self.open_steps = np.where(rows, 0, self.open_steps).astype(np.int32)
        self.open_len = np.where(rows, 0, self.open_len).astype(np.int32)
        self.open = np.where(rows, 1, self.open).astype(np.int32)
        for k in INT_TOTALS:
            setattr(self, k, getattr(self, k).astype(np.int32))

    def arrays(self):
        """name -> array, the names and shapes of imgenv_episodes_out"""
        out = {k: getattr(self, k) for k in INT_TOTALS + F64_TOTALS}
        out.update(ends=self.ends, figure_sums=self.figure_sums, open_f64=self.open_f64, open_steps=self.open_steps, open_len=self.open_len,
                   open=self.open)
        return out

    def per_episode(self, robot, figure):
        """the figure of each counted episode of one robot, in order (the reference's ``*_array`` lists)"""
        k = FIGURES.index(figure)
        return [float(fig[k][robot]) for rows, fig in self.log if rows[robot]]

    def statistics(self):
        """``VecImageEnv.episode_statistics()`` from the model's arrays"""
        ends = dict(zip(ENDS, (int(c) for c in self.ends.sum(axis=1))))
        fig = dict(zip(FIGURES, (float(x) for x in self.figure_sums.sum(axis=1))))
        n, steps = max(1, int(self.episodes.sum())), max(1, int(self.speed_steps.sum()))
        return dict(arrive_rate=ends["arrive"] / n, static_coll_rate=ends["static_collision"] / n, ped_coll_rate=ends["ped_collision"] / n,
                    other_coll_rate=ends["other_collision"] / n, avg_arrive_steps=int(self.arrive_steps.sum()) / max(1, ends["arrive"]),
                    stuck_rate=ends["timeout"] / n, avg_v=float(self.v_sum.sum()) / steps, avg_w=float(self.w_sum.sum()) / steps,
                    avg_w_variance=fig["w_variance"] / n, avg_v_jerk=fig["v_jerk"] / n, avg_w_jerk=fig["w_jerk"] / n,
                    avg_w_zero=fig["w_zero"] / n, aborted_rate=ends["aborted"] / n, episodes=int(self.episodes.sum()),
                    short_episodes=int(self.short_episodes.sum()), avg_return=float(self.return_sum.sum()) / n,
                    avg_len=int(self.len_sum.sum()) / n)
