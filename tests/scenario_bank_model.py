"""Which recorded episode does placement number n replay?  The model of include/imgenv.h's scenario bank for the tests: the draw
itself in Python integers and in numpy (``scenario_for_placement``, ``scenarios_for_placements``), and ``ScenarioModel``, which
follows a handle's worlds through host resets, device resets and policy switches and answers what ``imgenv_world_scenarios``
must answer.

QUEUE is the reference's ``reset_index % len(reset_reqs)`` (envs/env/yaml_env.py:223-244) with the queue's position at placement 0
as ``first``; BY_PLACEMENT is the map bank's draw (splitmix64's finaliser, the upper 32 bits scaled by multiply-shift) over
``seed0 + n + SALT``, all sums modulo 2^64."""
import numpy as np

M64 = (1 << 64) - 1
SALT = 0x3C6EF372FE94F82B  # the fractional bits of sqrt(5)
TRACKS_SALT = 0xBB67AE8584CAA73B
POLICIES = {"off": 0, "queue": 1, "placement": 2}


def mix_draw(seed, n):
    """csrc/map_bank.h: map_for_placement"""
    if n <= 1:
        return 0
    z = (seed + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return ((z >> 32) * n) >> 32


def scenario_for_placement(policy, seed0, first, n, n_scenarios):
    policy = POLICIES.get(policy, policy)
    if n_scenarios < 1 or policy == 0:
        return -1
    if policy == 1:
        return ((first + n) & M64) % n_scenarios
    return mix_draw((seed0 + n + SALT) & M64, n_scenarios)


def scenarios_for_placements(policy, seed0, first, ns, n_scenarios):
    """the same over a numpy array of placement numbers (uint64 arithmetic wraps as the C code's does)"""
    policy = POLICIES.get(policy, policy)
    ns = np.asarray(ns, np.uint64)
    if n_scenarios < 1 or policy == 0:
        return np.full(ns.shape, -1, np.int64)
    with np.errstate(over="ignore"):
        if policy == 1:
            return ((np.uint64(first & M64) + ns) % np.uint64(n_scenarios)).astype(np.int64)
        if n_scenarios == 1:
            return np.zeros(ns.shape, np.int64)
        z = np.uint64((seed0 + SALT) & M64) + ns + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return (((z >> np.uint64(32)) * np.uint64(n_scenarios)) >> np.uint64(32)).astype(np.int64)


class ScenarioModel:
    """``cur[k]``: the scenario world k's running episode came from, -1 where its reset was not fed by the bank"""

    def __init__(self, n_worlds, n_scenarios, seed0=0):
        self.n, self.seed0 = n_scenarios, seed0
        self.cur = np.full(n_worlds, -1, np.int32)
        self.epochs = [(0, "off", 0)]  # (first placement number, policy, first)

    def set_policy(self, policy, first=0, at=0):
        """``imgenv_scenarios_policy`` queued when the device had handed out ``at`` placements"""
        if at == 0:
            self.epochs = [(0, policy, first)]
        else:
            self.epochs.append((at, policy, first))

    def policy_of(self, serial):
        return [e for e in self.epochs if e[0] <= serial][-1]

    def scenario_of(self, serial):
        _, policy, first = self.policy_of(serial)
        return scenario_for_placement(policy, self.seed0, first, serial, self.n)

    def host_reset(self, k, scenario=-1):
        self.cur[k] = scenario

    def device_reset(self, k, serial):
        self.cur[k] = self.scenario_of(serial)
        return int(self.cur[k])
