"""The episode log's rule (tests/episode_log_model.py around the unchanged EpisodeModel) against the reference's own log file:
tests/golden/ped_dataset_ref.npz holds the commands of six episodes the reference's PedTrajectoryDatasetWrapper ran, how each ended,
the world it ran on and the lines ``out2logfile`` wrote.  Fed the same commands, the model's records turned into lines by
``img_env_amd.envs.episode_log_lines`` must be that file, line for line.  Then the branches the recording does not reach: episodes
too short to count, and the ring."""
import os

import numpy as np
import pytest

from episode_log_model import F64_NAMES, I32_NAMES, NONE64, EpisodeLogModel
from episode_model import FIGURES
from img_env_amd.envs import episode_log_lines

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ped_dataset_ref.npz")


def test_the_log_lines_are_the_references_own_output_file():
    z = np.load(GOLDEN)
    n_ep = sum(1 for k in z.files if k.startswith("cmds_"))
    assert n_ep == 6
    log = EpisodeLogModel(1, 0.4, min_steps=0, capacity=16)
    one = np.ones(1, bool)
    log.reset(one, [0], tracks=int(z["world_0"]))  # the first reset opens episode 0 and logs nothing
    assert log.n_written == 0
    for e in range(n_ep):
        for v, w in z["cmds_%d" % e]:
            log.m.step_speeds([v], [w], one, [0.0])
        log.reset(one, [int(z["code_%d" % e])], tracks=int(z["world_%d" % (e + 1)]) if e + 1 < n_ep else -1)
    rec = log.columns()
    assert rec["n_written"] == n_ep and rec["oldest"] == 0 and rec["counted"].all()
    assert rec["tracks"].tolist() == [int(z["world_%d" % e]) for e in range(n_ep)]
    assert rec["episode"].tolist() == list(range(1, n_ep + 1))
    lines = episode_log_lines(rec, 0.4, "ped_dataset")
    assert "\n".join(lines) + "\n" == str(z["log"])
    # the Barn wrapper's line: the map as cur_world, the static collision in the third column
    rec["map"] = np.arange(n_ep, dtype=np.int32)
    barn = episode_log_lines(rec, 0.4, "barn")
    for e, (a, b) in enumerate(zip(lines, barn)):
        fa, fb = a.split(", "), b.split(", ")
        assert fb[0] == str(e) and fb[2] == "0" and fa[1] == fb[1] and fa[3:] == fb[3:]
    with pytest.raises(ValueError):
        episode_log_lines(rec, 0.4, "other")


def test_a_short_episode_is_logged_without_figures_and_its_commands_ride_on():
    """three robots of one chain, min_steps 3: robot 0 ends after 2 steps (short), robots 1 and 2 after 5; the short record has
    counted 0, episode 0 and zero figures but its code, steps, len and return; the next counted episode of robot 0 carries the
    short one's commands in its figures (n = 2 + 5), exactly what the fold adds to figure_sums"""
    rng = np.random.default_rng(0)
    log = EpisodeLogModel(3, 0.25, min_steps=3, capacity=8, robots_per_world=1)
    log.reset(np.ones(3, bool), np.zeros(3, np.int32), maps=[0, 1, 0], placements=np.array([7, 8, 9], np.uint64))

    def steps(k):
        for _ in range(k):
            a = rng.uniform(-1, 1, (3, 3)).astype(np.float32)
            log.step(a, np.array([1, 1, 0], np.uint8), rng.uniform(-1, 1, 3))
    steps(2)
    log.reset(np.array([0]), [2, 0, 0], maps=1)  # robot 0 alone: a short episode
    steps(3)
    before = log.m.figure_sums.copy()
    log.reset(np.array([2, 1]), [0, 5, 10], maps=[5, 6, 7])  # list order 2, 1
    steps(2)
    log.reset(np.array([0, 1, 2]), [1, 3, 3])
    rec = log.columns()
    assert rec["robot"].tolist() == [0, 2, 1, 0, 1, 2] and rec["world"].tolist() == [0, 2, 1, 0, 1, 2]
    assert rec["counted"].tolist() == [0, 1, 1, 1, 0, 0] and rec["episode"].tolist() == [0, 1, 1, 1, 0, 0]
    assert rec["steps"].tolist() == [2, 5, 5, 5, 2, 2] and rec["code"].tolist() == [2, 10, 5, 1, 3, 3]
    assert rec["len"].tolist() == [2, 0, 5, 5, 2, 0]
    assert rec["map"].tolist() == [0, 0, 1, 1, 6, 7] and rec["placement"].tolist() == [7, 9, 8, int(NONE64), int(NONE64), int(NONE64)]
    for k in FIGURES:
        assert rec[k][0] == 0.0 and rec[k][4] == 0.0 and rec[k][5] == 0.0
    assert rec["ep_return"][0] != 0.0
    # the counted records are what the fold added to the robots' figure sums
    for k, name in enumerate(FIGURES):
        assert rec[name][1] == log.m.figure_sums[k][2] - before[k][2] and rec[name][2] == log.m.figure_sums[k][1] - before[k][1]
    # robot 0's counted episode took 5 steps but its path sums cover the 2 + 5 commands: v_avg is their mean
    assert log.m.short_episodes.tolist() == [1, 1, 1] and rec["v_avg"][3] != 0.0
    # robot 2 was never clean: its commands are zeros, so are its figures, but it counts
    assert rec["v_avg"][1] == 0.0 and rec["counted"][1] == 1
    log.clear()  # imgenv_episodes_clear does not touch the log
    assert log.n_written == 6


@pytest.mark.parametrize("capacity", [1, 4, 5, 64])
def test_ring_arithmetic(capacity):
    """record q lives in slot q % capacity; a chain that closes more episodes than the ring holds leaves its last ``capacity``;
    reads clip to [oldest, n_written)"""
    n = 5
    log = EpisodeLogModel(n, 0.25, min_steps=0, capacity=capacity, robots_per_world=1)
    log.reset(np.ones(n, bool), np.zeros(n, np.int32))
    rng = np.random.default_rng(capacity)
    for chain in range(4):
        log.step(rng.uniform(-1, 1, (n, 3)).astype(np.float32), np.ones(n, np.uint8), rng.uniform(-1, 1, n))
        rows = rng.permutation(n)[:rng.integers(1, n + 1)]
        log.reset(rows, rng.integers(0, 11, n))
    N = log.n_written
    assert N == len(log.records) and log.oldest == max(0, N - capacity)
    ring = log.ring()
    assert ring["i32"].shape == (len(I32_NAMES), capacity) and ring["f64"].shape == (len(F64_NAMES), capacity)
    for q in range(log.oldest, N):
        r = log.records[q]
        assert ring["i32"][:, q % capacity].tolist() == [r[k] for k in I32_NAMES]
        assert ring["f64"][:, q % capacity].tolist() == [r[k] for k in F64_NAMES]
    allrec = log.columns()
    assert allrec["seq"].tolist() == list(range(log.oldest, N))
    part = log.columns(first=0, count=3)
    assert part["seq"].tolist() == [q for q in range(0, 3) if q >= log.oldest]
    assert log.columns(first=N)["seq"].size == 0 and log.columns(first=N + 5, count=2)["seq"].size == 0
    tail = log.columns(first=N - 1)
    assert tail["seq"].tolist() == [N - 1] and tail["robot"][0] == log.records[-1]["robot"]
