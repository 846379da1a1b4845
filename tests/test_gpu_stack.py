"""The observation stacks on the device (imgenv_stack_enable, csrc/stack.h: StateBatchWrapper per robot of a handle) against the
numpy model of tests/stack_model.py, which tests/test_stack_abi.py holds to the reference's own recordings.  Stacking only
moves bytes, so every comparison against the model is exact: bit patterns, no tolerance.  The frames fed to the model are
``world.snapshot()`` rows taken after each call."""
import ast
import copy
import json
import os

import numpy as np
import pytest

from scenarios import golden_cfg, random_actions, small_world
from stack_model import StackModel, bits, depths

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIELDS = ("sensor_maps", "vector_states", "lasers")


class Tracker:
    """the model of every stacked field of one ``World`` handle"""

    def __init__(self, world, kd):
        self.world, self.kd = world, dict(zip(FIELDS, kd))
        assert set(world.stack) == {f for f in FIELDS if self.kd[f] > 0}, (sorted(world.stack), self.kd)
        self.models = {f: StackModel(self.kd[f]) for f in world.stack}

    def reset(self, frames, rows):
        for f, m in self.models.items():
            m.reset(frames[f], rows)

    def step(self, frames, rows=None):
        for f, m in self.models.items():
            m.update(frames[f], np.zeros(len(frames[f]), bool) if rows is None else rows)

    def stacks(self):
        import torch
        torch.cuda.synchronize()
        return {f: t.cpu().numpy() for f, t in self.world.stack.items()}

    def check(self, where, got=None):
        got = self.stacks() if got is None else got
        for f, m in self.models.items():
            want = m.value
            assert got[f].dtype == want.dtype, (where, f)
            if f == "vector_states":  # [n, k * state_dim] (base.py:135-136)
                assert got[f].shape == (want.shape[0], want.shape[1] * want.shape[2]), (where, f, got[f].shape)
                want = want.reshape(got[f].shape)
            assert got[f].shape == want.shape, (where, f, got[f].shape, want.shape)
            same = bits(got[f]) == bits(want)
            assert same.all(), (where, f, "robots", np.unique(np.argwhere(~same)[:, 0])[:8].tolist())


def _env_rows(envs, E, R):
    rows = np.zeros(E * R, bool)
    for k in envs:
        rows[k * R:(k + 1) * R] = True
    return rows


# ---- 1. the reference's recordings through VecImageEnv(env_num=1, stack=True) ----
@pytest.mark.parametrize("name", ["a", "c"])
def test_vec_env_stack_matches_the_references_recordings(name):
    """depths 2 / 3 / 2 over 3 robots and 3 resets (a), 1 / 3 / 1 over 6 resets (c): the observation list equals what the
    reference's wrapper stack returned on every step (sensor maps exact, the others <= 1e-4: the simulator's difference, not
    the stack's), through its time-limit auto-resets"""
    import torch
    from img_env_amd import worldgen
    from img_env_amd.vec_env import VecImageEnv
    z = np.load(os.path.join(GOLDEN, "python_stack_%s.npz" % name))
    meta = ast.literal_eval(str(z["meta"]))
    grid = worldgen.make_grid(200, meta["seed"])
    cfg = golden_cfg(meta, grid)
    layouts = [worldgen.make_layout(grid, 0.125, meta["n_robots"], meta["n_peds"], seed=meta["seed"] + 100 + k, n_obstacles=2)
               for k in range(meta["n_layouts"])]
    table = np.array([list(a) + [0] * (3 - len(a)) for a in cfg["discrete_actions"]], np.float32)  # (v, w[, beep]): action.py:23-38
    vec = VecImageEnv(cfg, env_num=1, stack=True)

    class Seq:  # every reset takes the next fixed layout, as the generator's reset service did
        n = 0

        def reset(self, extent=None):
            lay = layouts[Seq.n % len(layouts)]
            Seq.n += 1
            return lay
    vec.env_poses[0] = Seq()

    def same_obs(obs, t):
        assert isinstance(obs, list) and len(obs) == 3
        for k, o in enumerate(obs):
            want = z["exp_obs%d" % k][t]
            got = o.cpu().numpy()
            assert got.shape == want.shape, (t, k, got.shape, want.shape)
            if meta["obs_names"][k] == "sensor_maps":
                assert np.array_equal(got, want), (t, k)
            else:
                assert np.abs(got.astype(np.float64) - want).max() <= 1e-4, (t, k)
    try:
        assert vec.world.stack_depths == depths(cfg["image_batch"], cfg["state_batch"], cfg["laser_batch"])
        same_obs(vec.reset(), 0)
        for s in range(meta["steps"]):
            act = torch.as_tensor(table[z["actions"][s]], device="cuda")
            obs, rew, done, info = vec.step(act)
            same_obs(obs, s + 1)
            assert np.array_equal(info["all_down"].cpu().numpy(), z["exp_all_down"][s]), s
        assert Seq.n == int(z["n_resets"]) >= 3
    finally:
        vec.close()


# ---- 2. / 3. / 4. auto-reset with the envs out of phase ----
def _run_out_of_phase(cfg, E, R, device_reset, steps=20, manual=(1,), min_resets=None):
    import torch
    from img_env_amd.vec_env import VecImageEnv
    kd = depths(cfg["image_batch"], cfg["state_batch"], cfg["laser_batch"])
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, native_spawn=True, device_reset=device_reset, stack=True)
    try:
        assert vec.world.stack_depths == kd
        tr = Tracker(vec.world, kd)
        vec.reset()
        tr.reset(vec.world.snapshot(), np.ones(E * R, bool))
        tr.check("reset")
        rng = np.random.default_rng(2)
        resets, mixed = 0, 0
        for s in range(steps):
            a = np.zeros((E * R, 3), np.float32)
            a[:, 0], a[:, 1] = rng.uniform(0, 0.6, E * R), rng.uniform(-0.9, 0.9, E * R)
            state, rew, done, info = vec.step(torch.as_tensor(a, device="cuda"))
            finished = vec.world.autoreset_last()[0] if device_reset else list(info["reset_envs"])
            if device_reset:
                assert info["reset_envs"] is None
            resets += len(finished)
            mixed += 0 < len(finished) < E
            tr.step(vec.world.snapshot(), _env_rows(finished, E, R))
            tr.check(s)
            if isinstance(state, list):  # ObsStateTmp / ObsLaserStateTmp: [sensor_maps | lasers, vector_states, ped_maps]
                assert len(state) == 3 and state[1].data_ptr() == vec.world.stack["vector_states"].data_ptr()
            else:  # the state handed out carries the stacks
                for f in vec.world.stack:
                    assert getattr(state, f).data_ptr() == vec.world.stack[f].data_ptr(), f
            if s == 2 and manual:  # put some envs out of phase with the others
                vec.reset_envs(list(manual))
                tr.reset(vec.world.snapshot(), _env_rows(manual, E, R))
                tr.check("manual reset")
        assert resets >= (2 * E if min_resets is None else min_resets), resets
        assert mixed >= 1  # a step on which some envs restarted and others did not
    finally:
        vec.close()


@pytest.mark.parametrize("batches", [(2, 3, 2), (4, 1, -1)])
@pytest.mark.parametrize("E,R,P", [(5, 3, 4), (70, 2, 3), (300, 4, 0)])
@pytest.mark.parametrize("device_reset", [False, True], ids=["host_reset", "device_reset"])
def test_stacks_follow_every_env_through_its_own_resets(E, R, P, batches, device_reset):
    """imgenv_step_autoreset / imgenv_step_autoreset_device: the finished envs restart their stacks, the others shift -- one env put
    out of phase by hand (imgenv_reset_worlds_spawn), so that every later step mixes both"""
    from img_env_amd import worldgen
    grid = worldgen.make_grid(200, 3)
    cfg = worldgen.make_yaml_cfg(R, P, grid, time_max=5, n_obstacles=3, seed=9, image_batch=batches[0], state_batch=batches[1],
                                 laser_batch=batches[2])
    _run_out_of_phase(cfg, E, R, device_reset)


def test_rows_that_are_no_multiple_of_16_bytes():
    """20-byte vector states and 1448-byte scans (181 beams): the narrow paths of the kernel"""
    from img_env_amd import worldgen
    grid = worldgen.make_grid(200, 3)
    cfg = worldgen.make_yaml_cfg(3, 2, grid, time_max=5, n_obstacles=3, seed=9, state_dim=5, beams=181, image_batch=2, state_batch=3,
                                 laser_batch=2)
    _run_out_of_phase(cfg, 7, 3, True)


@pytest.mark.parametrize("batches", [(1, 3, 0), (3, 3, 2)])
def test_stacks_behind_the_tiled_view_kernels_of_the_shipped_geometry(tmp_path, batches):
    """the shipped test.yaml cast and geometry (48 x 48 sensor maps from 400 x 400 views, 1000 beams, device-side reset): the launch
    sits behind both branches of launch_views; (1, 3, 0) are the shipped file's depths"""
    from PIL import Image
    from img_env_amd import worldgen
    m = np.full((110, 110), 255, np.uint8)
    m[:5] = m[-5:] = 0
    m[:, :5] = m[:, -5:] = 0
    Image.fromarray(m).save(str(tmp_path / "room.png"))
    z = np.load(os.path.join(GOLDEN, "spawn_ref.npz"))
    cfg = worldgen.shipped_test_yaml_cfg("room.png", json.loads(str(z["test@1/cfg"])))
    assert (cfg["image_batch"], cfg["state_batch"], cfg["laser_batch"]) == (1, 3, 0)
    cfg.update(map_dir=str(tmp_path), seed=3, time_max=4, image_batch=batches[0], state_batch=batches[1], laser_batch=batches[2])
    _run_out_of_phase(cfg, 24, 1, True, steps=14, manual=(1, 5))


# ---- 5. depth 1 is an alias ----
def test_depth_one_is_an_alias_and_costs_no_launch():
    from img_env_amd.world import World
    grid, params, layout = small_world(6, 3, seed=4)
    plain, one, deep = World(params, grid), World(params, grid), World(params, grid)
    try:
        assert one.enable_stack(1, 1, 0) is one.stack and one.stack_arena is None
        assert one.stack_depths == (1, 1, 1)
        for f in FIELDS:
            assert one.stack[f].data_ptr() == one.out[f].data_ptr(), f
        assert one.stack["sensor_maps"].shape == (6, 1, 48, 48) and one.stack["lasers"].shape == (6, 1, 360)
        assert one.stack["vector_states"].shape == (6, 3)
        deep.enable_stack(2, 0, -1)
        assert set(deep.stack) == {"sensor_maps"} and deep.stack["sensor_maps"].shape == (6, 2, 48, 48)
        rng = np.random.default_rng(0)
        for w in (plain, one, deep):
            w.reset(layout)
        assert plain.launches() == one.launches() == deep.launches() - 1
        for s in range(3):
            a = random_actions(rng, 6)
            for w in (plain, one, deep):
                w.step(a)
            assert plain.launches() == one.launches() == deep.launches() - 1, s
        with pytest.raises(RuntimeError, match="already"):
            one.enable_stack(2, 2, 2)
        with pytest.raises(RuntimeError, match="after the first reset"):
            plain.enable_stack(2, 2, 2)
        fresh = World(params, grid)
        try:
            with pytest.raises(ValueError, match="IMGENV_STACK_MAX_DEPTH"):
                fresh.enable_stack(17, 0, -1)
        finally:
            fresh.close()
    finally:
        for w in (plain, one, deep):
            w.close()


# ---- 6. stream order ----
def test_push_is_ordered_on_the_stream_without_any_synchronisation():
    """40 steps of a device-reset VecImageEnv queued back to back with device-resident actions, each followed on the same stream
    by clones of the stacked fields and of all_down; ONE synchronisation at the end.  The next step's early observation work runs
    on side streams: the final stacks must equal the model fed those clones."""
    import torch
    from img_env_amd import worldgen
    from img_env_amd.vec_env import VecImageEnv
    E, R, steps = 64, 2, 40
    grid = worldgen.make_grid(200, 3)
    cfg = worldgen.make_yaml_cfg(R, 3, grid, time_max=5, n_obstacles=3, seed=9, image_batch=2, state_batch=3, laser_batch=2)
    vec = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, stack=True)
    try:
        tr = Tracker(vec.world, (2, 3, 2))
        g = torch.Generator(device="cuda").manual_seed(1)
        acts = torch.zeros(steps, E * R, 3, device="cuda")
        acts[:, :, 0] = torch.rand(steps, E * R, generator=g, device="cuda") * 0.6
        acts[:, :, 1] = torch.rand(steps, E * R, generator=g, device="cuda") * 1.8 - 0.9
        vec.reset()
        first = {f: vec.world.out[f].clone() for f in FIELDS}
        frames, downs = [], []
        for s in range(steps):
            _, _, _, info = vec.step(acts[s])
            frames.append({f: vec.world.out[f].clone() for f in FIELDS})
            downs.append(info["all_down"].clone())
        torch.cuda.synchronize()
        tr.reset({f: t.cpu().numpy() for f, t in first.items()}, np.ones(E * R, bool))
        restarts = 0
        for s in range(steps):
            rows = downs[s].cpu().numpy().astype(bool)
            restarts += int(rows.sum()) // R
            tr.step({f: t.cpu().numpy() for f, t in frames[s].items()}, rows)
        tr.check("after %d unsynchronised steps" % steps)
        assert restarts >= 64
    finally:
        vec.close()


def test_push_is_ordered_in_a_plain_step_loop():
    import torch
    from img_env_amd.world import World
    n, steps = 16, 40
    grid, params, layout = small_world(n, 6, seed=3)
    w = World(params, grid)
    try:
        w.enable_stack(3, 2, 4)
        tr = Tracker(w, (3, 2, 4))
        g = torch.Generator(device="cuda").manual_seed(2)
        acts = torch.zeros(steps, n, 3, device="cuda")
        acts[:, :, 0] = torch.rand(steps, n, generator=g, device="cuda") * 0.6
        acts[:, :, 1] = torch.rand(steps, n, generator=g, device="cuda") * 1.8 - 0.9
        w.reset(layout)
        first = {f: w.out[f].clone() for f in FIELDS}
        frames = []
        for s in range(steps):
            w.step(acts[s])
            frames.append({f: w.out[f].clone() for f in FIELDS})
        torch.cuda.synchronize()
        tr.reset({f: t.cpu().numpy() for f, t in first.items()}, np.ones(n, bool))
        for s in range(steps):
            tr.step({f: t.cpu().numpy() for f, t in frames[s].items()})
        tr.check("after %d unsynchronised steps" % steps)
        moved = np.abs(frames[-1]["vector_states"].cpu().numpy() - first["vector_states"].cpu().numpy()).max()
        assert moved > 0  # (the frames differ from step to step: a stack of equal frames would prove nothing)
    finally:
        w.close()


# ---- 7. the stacks disturb nothing ----
@pytest.mark.parametrize("guard", ["first", "copy", "check"])
def test_a_handle_with_stacks_computes_what_one_without_computes(guard):
    """same parameters, layout and actions, one handle with stacks (2, 3, 2) and one without: every output is bit-identical on every
    step.  Under "copy" (IMGENV_FLAG_FULL_REWRITE) ``out`` is the public copy and the stacks are fed from the working arena: they
    must still equal the model."""
    from img_env_amd.world import World
    n = 12
    grid, params, layout = small_world(n, 5, seed=7)
    params = dict(params, output_guard=guard)
    a_, b_ = World(params, grid), World(params, grid)
    try:
        assert a_.output_guard == guard
        a_.enable_stack(2, 3, 2)
        tr = Tracker(a_, (2, 3, 2))
        a_.reset(layout)
        b_.reset(layout)
        sa, sb = a_.snapshot(), b_.snapshot()
        tr.reset(sa, np.ones(n, bool))
        tr.check("reset")
        rng = np.random.default_rng(5)
        for s in range(10):
            a = random_actions(rng, n)
            a_.step(a)
            b_.step(a)
            sa, sb = a_.snapshot(), b_.snapshot()
            assert set(sa) == set(sb)
            for f in sa:
                assert sa[f].tobytes() == sb[f].tobytes(), (s, f)
            tr.step(sa)
            tr.check(s)
    finally:
        a_.close()
        b_.close()


# ---- 8. robot shards ----
def test_shards_stack_their_local_rows():
    """two handles owning halves of one 24-robot world (step_begin, the exchange by hand, step_end), each with stacks (2, 3, 2),
    through one reset in the middle: their stacks concatenated equal the whole-world handle's on every step"""
    import torch
    from img_env_amd.world import World
    n, n_peds, steps = 24, 10, 12
    grid, params, layout = small_world(n, n_peds, seed=31, grid_size=320, clearance=0.8)
    _, _, layout2 = small_world(n, n_peds, seed=32, grid_size=320, clearance=0.8)
    bounds = [0, n // 2, n]
    full = World(params, grid)
    ranks = [World(dict(params, robot_begin=bounds[r], robot_end=bounds[r + 1]), grid) for r in range(2)]
    try:
        for w in [full] + ranks:
            w.enable_stack(2, 3, 2)
        assert ranks[0].stack["sensor_maps"].shape[0] == n // 2
        tr = Tracker(full, (2, 3, 2))

        def exchange():
            torch.cuda.synchronize()
            for r, w in enumerate(ranks):
                for q, o in enumerate(ranks):
                    if q != r:
                        w.records[bounds[q]:bounds[q + 1]].copy_(o.records[bounds[q]:bounds[q + 1]])

        def same(where):
            torch.cuda.synchronize()
            for f in FIELDS:
                whole = full.stack[f].cpu().numpy()
                parts = np.concatenate([w.stack[f].cpu().numpy() for w in ranks], axis=0)
                assert bits(whole).shape == bits(parts).shape and (bits(whole) == bits(parts)).all(), (where, f)

        def reset_all(lay):
            for w in [full] + ranks:
                w.reset(lay)
            tr.reset(full.snapshot(), np.ones(n, bool))
            tr.check("reset")
            same("reset")
        reset_all(layout)
        rng = np.random.default_rng(5)
        for s in range(steps):
            a = random_actions(rng, n)
            full.step(a)
            for r, w in enumerate(ranks):
                w.step_begin(a[bounds[r]:bounds[r + 1]])
            exchange()
            for w in ranks:
                w.step_end()
            tr.step(full.snapshot())
            tr.check(s)
            same(s)
            if s == steps // 2:
                reset_all(layout2)
    finally:
        full.close()
        for w in ranks:
            w.close()


# ---- the probe's torch variant is the same computation ----
def test_the_probes_torch_stack_keeps_the_same_stacks():
    """tools/vec_env_probe.py measures the library's stacks against the same semantics done with torch ops on an unstacked
    VecImageEnv (shift + torch.where on all_down): both must hold the same bytes, or the comparison compares nothing"""
    import sys
    import torch
    from img_env_amd import worldgen
    from img_env_amd.vec_env import VecImageEnv
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from vec_env_probe import TorchStack, stack_depths
    E, R, batches = 12, 2, (2, 3, 2)
    grid = worldgen.make_grid(200, 3)
    cfg = worldgen.make_yaml_cfg(R, 3, grid, time_max=5, n_obstacles=3, seed=9, image_batch=batches[0], state_batch=batches[1],
                                 laser_batch=batches[2])
    lib = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True, stack=True)
    ref = VecImageEnv(copy.deepcopy(cfg), env_num=E, seed=9, device_reset=True)
    try:
        ts = TorchStack(ref, stack_depths(batches))
        lib.reset()
        ref.reset()
        ts.reset()
        rng = np.random.default_rng(2)
        restarts = 0
        for s in range(16):
            a = np.zeros((E * R, 3), np.float32)
            a[:, 0], a[:, 1] = rng.uniform(0, 0.6, E * R), rng.uniform(-0.9, 0.9, E * R)
            a = torch.as_tensor(a, device="cuda")
            lib.step(a)
            _, _, _, info = ref.step(a)
            ts.push(info["all_down"])
            restarts += int(info["all_down"].sum())
            torch.cuda.synchronize()
            for f in FIELDS:
                got, want = lib.world.stack[f].cpu().numpy(), ts.stack[f].cpu().numpy().reshape(lib.world.stack[f].shape)
                assert (bits(got) == bits(want)).all(), (s, f)
        assert restarts >= 2 * E * R
    finally:
        lib.close()
        ref.close()
