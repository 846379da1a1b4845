"""The rule of the device-side episode log (include/imgenv.h: imgenv_episode_log_enable; csrc/episode_log.h) in numpy, around the
unchanged ``EpisodeModel`` of tests/episode_model.py: a reset chain covers robot rows in a given order, every covered row with an
open episode appends one record -- how the episode ended, its steps, length, return and, when it counts, the figures the fold
adds to ``figure_sums`` -- tagged with what the episode ran on, noted when it opened; every covered row then takes the tags of the
episode that starts.  ``records`` holds every record ever appended; ``ring()`` is the device's memory, ``columns()`` what
``VecImageEnv.episode_log()`` returns.  tests/test_episode_log_model.py holds it to the reference's own log file."""
import numpy as np

from episode_model import FIGURES, EpisodeModel

I32_NAMES = ("robot", "world", "code", "steps", "len", "counted", "episode", "map", "tracks", "scenario_raw")
F64_NAMES = ("ep_return",) + FIGURES
NONE64 = np.uint64(0xFFFFFFFFFFFFFFFF)
SCN_DEVICE = -2


class EpisodeLogModel:
    def __init__(self, n, dt, min_steps=3, capacity=1 << 16, robots_per_world=None):
        self.m = EpisodeModel(n, dt, min_steps)
        self.n, self.capacity = int(n), int(capacity)
        self.Rw = int(robots_per_world) if robots_per_world else self.n  # one world (or a robot shard): world 0
        self.records = []  # one dict per record, in log order: I32_NAMES + F64_NAMES + placement
        # the tags of each robot's open episode: "open before the log was"
        self.tag_map, self.tag_tracks, self.tag_scn = (np.full(self.n, -1, np.int32) for _ in range(3))
        self.tag_place = np.full(self.n, NONE64, np.uint64)
        self.i32 = np.zeros((len(I32_NAMES), self.capacity), np.int32)
        self.f64 = np.zeros((len(F64_NAMES), self.capacity), np.float64)
        self.placement = np.zeros(self.capacity, np.uint64)

    n_written = property(lambda self: len(self.records))
    oldest = property(lambda self: max(0, len(self.records) - self.capacity))

    def step(self, actions, is_clean, rewards):
        self.m.step(actions, is_clean, rewards)

    def clear(self):
        """imgenv_episodes_clear: the log is not touched"""
        self.m.clear()

    def reset(self, rows, codes, maps=0, tracks=-1, scenarios=-1, placements=NONE64):
        """a reset chain over the robot rows ``rows`` IN THAT ORDER (an index array; a bool mask means ascending); ``codes`` = the
        last step's ``step_dones_info`` [n]; the tags of the episodes that start, per robot [n] or one value for all"""
        rows = np.asarray(rows)
        order = np.flatnonzero(rows) if rows.dtype == bool else rows.astype(np.int64)
        mask = np.zeros(self.n, bool)
        mask[order] = True
        assert mask.sum() == len(order), "a row listed twice"
        m, codes = self.m, np.asarray(codes).astype(np.int32)
        was_open, steps, length, ret = m.open.copy(), m.open_steps.copy(), m.open_len.copy(), m.open_f64[-1].copy()
        n_log = len(m.log)
        m.reset(mask, codes)
        counted = was_open.astype(bool) & mask & (steps > m.min_steps)
        fig = m.log[-1][1] if len(m.log) > n_log else np.zeros((len(FIGURES), self.n))
        assert len(m.log) == n_log or np.array_equal(m.log[-1][0], counted)
        first = len(self.records)
        for r in order:
            if not was_open[r]:
                continue
            rec = dict(robot=int(r), world=int(r) // self.Rw, code=int(codes[r]), steps=int(steps[r]), len=int(length[r]),
                       counted=int(counted[r]), episode=int(m.episodes[r]) if counted[r] else 0, map=int(self.tag_map[r]),
                       tracks=int(self.tag_tracks[r]), scenario_raw=int(self.tag_scn[r]), placement=np.uint64(self.tag_place[r]),
                       ep_return=np.float64(ret[r]))
            for k, name in enumerate(FIGURES):
                rec[name] = np.float64(fig[k][r]) if counted[r] else np.float64(0.0)
            self.records.append(rec)
        # the ring: of one chain's records the last `capacity` are written
        for q in range(max(first, len(self.records) - self.capacity), len(self.records)):
            s, rec = q % self.capacity, self.records[q]
            self.i32[:, s] = [rec[k] for k in I32_NAMES]
            self.f64[:, s] = [rec[k] for k in F64_NAMES]
            self.placement[s] = rec["placement"]
        for tag, new in ((self.tag_map, maps), (self.tag_tracks, tracks), (self.tag_scn, scenarios), (self.tag_place, placements)):
            tag[order] = np.broadcast_to(np.asarray(new, tag.dtype), (self.n,))[order]

    def ring(self):
        """name -> array, the names and shapes of imgenv_episode_log_out"""
        return dict(n_written=np.array([len(self.records)], np.uint64), i32=self.i32, f64=self.f64, placement=self.placement)

    def columns(self, first=None, count=None, scenario=None):
        """the records [max(first, oldest), min(first + count, n_written)) as a dict of columns plus ``seq``, ``oldest`` and
        ``n_written`` (``imgenv_episode_log_read``); ``scenario``: a function of a record that resolves its scenario (default:
        ``scenario_raw``)"""
        lo = max(self.oldest, 0 if first is None else int(first))
        hi = len(self.records) if count is None else min(len(self.records), (0 if first is None else int(first)) + int(count))
        recs = self.records[lo:hi] if lo < hi else []
        out = {k: np.array([r[k] for r in recs], np.int32) for k in I32_NAMES if k != "scenario_raw"}
        out["scenario"] = np.array([(scenario(r) if scenario else r["scenario_raw"]) for r in recs], np.int32)
        out.update({k: np.array([r[k] for r in recs], np.float64) for k in F64_NAMES})
        out["placement"] = np.array([r["placement"] for r in recs], np.uint64)
        out["seq"] = np.arange(lo, lo + len(recs), dtype=np.uint64)
        out["oldest"], out["n_written"] = self.oldest, len(self.records)
        return out
