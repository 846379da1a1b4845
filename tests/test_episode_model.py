"""The numpy model of the device-side episode statistics (tests/episode_model.py) without a GPU: replayed over the reference's own
TestEpisodeWrapper run (tests/golden/python_stack_c.npz) and against the repository's TestEpisodeWrapper / EpisodeStats
(img_env_amd/envs.py) on random multi-robot command streams."""
import ast
import os

import numpy as np
import pytest

from episode_model import ENDS, FIGURES, EpisodeModel, end_bin

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_the_model_reproduces_the_references_test_episode_wrapper():
    """44 steps of one robot, control_hz 0.25, through the reference's unmodified wrapper stack: its counters exactly, its running
    sums within 1e-6 and its per-episode lists within 1e-4 (the reference rounds with Python's decimal ``round``) -- the bars
    tests/test_gpu_envs.py holds the Python port to"""
    z = np.load(os.path.join(GOLDEN, "python_stack_c.npz"))
    meta = ast.literal_eval(str(z["meta"]))
    assert meta["steps"] == 44 and meta["n_robots"] == 1
    m = EpisodeModel(1, 0.25)
    m.reset(np.ones(1, bool), np.zeros(1, np.int32))  # the env's first reset: opens an episode, folds nothing
    assert m.episodes.sum() == 0 and m.short_episodes.sum() == 0
    for t in range(meta["steps"]):
        sp = z["exp_speeds"][t]
        m.step_speeds(sp[:, 0], sp[:, 1], np.ones(1, bool), z["exp_rewards"][t])
        if z["exp_all_down"][t].all():  # NeverStopWrapper resets with the step's info (base.py:198-211)
            m.reset(np.ones(1, bool), z["exp_dones_info"][t])
    counts = [int(m.episodes[0]), int(m.ends[0, 0]), int(m.ends[2, 0]), int(m.ends[3, 0]), int(m.ends[4, 0]), int(m.arrive_steps[0]),
              int(m.ends[1, 0]), int(m.speed_steps[0])]
    assert counts == z["te_counts"].tolist() == [5, 0, 0, 0, 0, 0, 5, 40]
    assert int(m.ends[5, 0]) == 0
    assert np.allclose([m.v_sum[0], m.w_sum[0]], z["te_sums"], atol=1e-6)
    lists = np.array([m.per_episode(0, k) for k in ("w_variance", "v_jerk", "w_jerk", "w_zero")], np.float64)
    assert lists.shape == z["te_arrays"].shape == (4, 5)
    assert np.allclose(lists, z["te_arrays"], atol=1e-4)
    # the totals are the lists' sums, in order
    for k in ("w_variance", "v_jerk", "w_jerk", "w_zero"):
        tot = 0.0
        for x in m.per_episode(0, k):
            tot += x
        assert m.figure_sums[FIGURES.index(k), 0] == tot
    # time_max 7 with resets every 8th step: every episode is 8 steps, all of them clean
    assert m.last_steps[0] == 8 and m.last_len[0] == 8 and m.last_code[0] == 10 and m.last_episode[0] == 5
    assert m.len_sum[0] == 40


def test_end_bins():
    assert end_bin([5, 10, 1, 2, 3, 0, 4, 7, -1]).tolist() == [0, 1, 2, 3, 4, 5, 5, 5, 5]
    assert ENDS[5] == "aborted"


class _FakeEnv:
    """feeds TestEpisodeWrapper the speeds of a prepared stream"""

    def __init__(self):
        self.next_speeds = None

    def step(self, action):
        import torch
        return None, None, None, {"speeds": torch.as_tensor(self.next_speeds)}

    def reset(self, **kwargs):
        return None


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_model_is_the_repositorys_test_episode_wrapper_per_robot(seed):
    """R robots of one env (they reset together, as TestEpisodeWrapper's env does) over random commands with exact-zero w, a
    too-short episode whose commands ride into the next one, and episode lengths on both sides of ``tmp_steps > 3``: the counters,
    the running sums and every per-episode figure equal the Python wrapper's -- the same float64 operations in the same order"""
    import torch
    from img_env_amd.envs import TestEpisodeWrapper
    R, dt = 5, 0.25
    rng = np.random.default_rng(seed)
    env = _FakeEnv()
    te = TestEpisodeWrapper(env, {"init_pose_bag_episodes": 10 ** 9, "control_hz": dt})
    m = EpisodeModel(R, dt)
    te.reset()
    m.reset(np.ones(R, bool), np.zeros(R, np.int32))
    lengths = [6, 2, 5, 4, 3, 1, 9, 4]  # 2, 3 and 1 are too short; 4 is the first that counts
    shorts = 0
    for ep, length in enumerate(lengths):
        for s in range(length):
            a = np.zeros((R, 3), np.float32)
            a[:, 0] = rng.uniform(0, 0.6, R)
            a[:, 1] = rng.choice([-0.9, -0.3, 0.0, 0.0, 0.3, 0.9], R) if s % 2 else rng.uniform(-0.9, 0.9, R)
            clean = rng.uniform(size=R) > 0.2
            rewards = rng.normal(size=R)
            env.next_speeds = a[:, :2] * clean[:, None].astype(np.float32)  # MultiRobotCleanWrapper's mask (base.py:83)
            te.step(None)
            m.step(a, clean, rewards)
        codes = rng.choice([5, 10, 1, 2, 3], R)
        te.reset(dones_info=torch.as_tensor(codes))
        m.reset(np.ones(R, bool), codes)
        shorts += length <= 3
    counted = len(lengths) - shorts
    assert te.cur_episode == counted and (m.episodes == counted).all() and (m.short_episodes == shorts).all() and shorts == 3
    ends = te._ends.numpy()
    for b, code in enumerate((5, 10, 1, 2, 3)):
        assert np.array_equal(m.ends[b], ends[:, code]), code
    assert (m.ends[5] == 0).all()
    assert np.array_equal(m.speed_steps, te._speed_steps.numpy()) and np.array_equal(m.arrive_steps, te._arrive_steps.numpy())
    assert np.array_equal(m.v_sum, te._v_sum.numpy()) and np.array_equal(m.w_sum, te._w_sum.numpy())
    assert len(te._episodes) == counted
    for r in range(R):
        for k in FIGURES:
            want = [float(e[k][r]) for e in te._episodes]
            assert m.per_episode(r, k) == want, (r, k)
    # pooled: statistics() divides by max_episodes, the model by the number of counted episodes
    te.max_episodes = counted
    want, got = te.statistics(), m.statistics()
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-12, abs=1e-12), k


def test_an_aborted_end_and_robots_that_reset_on_their_own():
    """a caller's reset of an unfinished robot (dones_info 0) is counted as aborted, the Python wrapper raises there; robots of
    different worlds fold on their own; steps before the first reset after enabling are ignored; clear keeps ``open``"""
    import torch
    from img_env_amd.envs import TestEpisodeWrapper
    m = EpisodeModel(4, 0.5, min_steps=1)
    a = np.array([[0.3, 0.2, 0], [0.1, -0.2, 0], [0.2, 0.0, 0], [0.5, 0.4, 0]], np.float32)
    m.step(a, np.ones(4), np.ones(4))
    assert m.open_steps.sum() == 0 and m.v_sum.sum() == 0  # no episode open yet
    m.reset(np.array([1, 1, 0, 0], bool), np.zeros(4))
    for s in range(3):
        m.step(a, np.ones(4), np.ones(4))
    assert m.open_steps.tolist() == [3, 3, 0, 0]
    m.reset(np.array([1, 0, 1, 0], bool), np.array([0, 5, 5, 5]))
    assert m.ends[5].tolist() == [1, 0, 0, 0] and m.episodes.tolist() == [1, 0, 0, 0] and m.open.tolist() == [1, 1, 1, 0]
    assert m.open_steps.tolist() == [0, 3, 0, 0] and m.last_code.tolist() == [0, 0, 0, 0] and m.last_episode.tolist() == [1, 0, 0, 0]
    assert m.last_return[0] == 3.0 and m.return_sum[0] == 3.0 and m.open_f64[-1].tolist() == [0.0, 3.0, 0.0, 0.0]
    m.clear()
    assert m.open.tolist() == [1, 1, 1, 0] and m.episodes.sum() == 0 and m.open_f64.sum() == 0 and m.open_steps.sum() == 0
    te = TestEpisodeWrapper(_FakeEnv(), {"init_pose_bag_episodes": 9, "control_hz": 0.5})
    te.env.next_speeds = a[:, :2]
    for s in range(5):
        te.step(None)
    with pytest.raises(ValueError):
        te.reset(dones_info=torch.zeros(4, dtype=torch.int64))
