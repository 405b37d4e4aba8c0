"""CPU-only: the push world's definition (include/ndp.h "push world") as tests/world_common.py restates it -- what the
render draws, what the starts promise, that the scripted expert solves the task inside the reference's 15-frame
trajectories and that chance does not --, the golden file, and every argument push_world refuses before it touches a
GPU.  The kernels against this restatement: tests/test_world_host.py (CPU) and tests/test_gpu_push_world.py."""
import os

import numpy as np
import pytest
import torch

import world_common as W
from ndivplanning_amd import push_world as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "push_world_case.npz")
FAR_GOAL = (1.15, 0.95)


def _state(g, o, t=FAR_GOAL):
    return W._state(g, o, t)


def _pixel(v, v0, size):
    return (float(np.float32(v)) - v0) / W.SIDE * size


# ------------------------------------------------------------------------------------------------------------ render
def test_constants_agree_with_the_header_and_the_package():
    text = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "ndp.h")).read()
    for name, value in (("X0", W.X0), ("Y0", W.Y0), ("SIDE", W.SIDE), ("REST_X", W.REST[0]), ("REST_Y", W.REST[1]),
                        ("Z_MIN", W.Z_MIN), ("Z_MAX", W.Z_MAX), ("Z_CONTACT", W.Z_CONTACT), ("OBJECT_Z", W.OBJECT_Z),
                        ("R_G", W.R_G), ("R_O", W.R_O), ("STEP", W.STEP), ("SUB", W.SUB), ("RING", W.RING),
                        ("SHADOW", W.SHADOW)):
        line = [ln for ln in text.splitlines() if ln.startswith("#define NDP_WORLD_%s " % name)]
        assert len(line) == 1, name
        assert float(line[0].split()[2]) == value, name
    for name in ("X0", "Y0", "SIDE", "REST", "Z_MIN", "Z_MAX", "Z_CONTACT", "OBJECT_Z", "R_G", "R_O", "R", "STEP", "SUB"):
        assert getattr(P, name) == getattr(W, name), name


@pytest.mark.parametrize("size", [32, 64, 128])
def test_the_rendered_block_lies_where_the_state_puts_it(size):
    state = _state((1.50, 0.60, 0.53), (1.2831, 0.8177))
    frame = W.render(state[None], size)[0]
    mask = (frame == np.array(W.OBJECT_RGB, np.uint8)).all(axis=2)
    assert mask.any()
    rows, cols = np.nonzero(mask)
    want_x, want_y = _pixel(1.2831, W.X0, size), _pixel(0.8177, W.Y0, size)
    assert abs(cols.mean() + 0.5 - want_x) <= 1.0 and abs(rows.mean() + 0.5 - want_y) <= 1.0
    k = W.coverage(W.scene(state, size)["object"], size).astype(np.float64)
    assert k.max() == 16
    px = np.arange(size) + 0.5
    assert abs((k.sum(axis=0) * px).sum() / k.sum() - want_x) <= 1.0
    assert abs((k.sum(axis=1) * px).sum() / k.sum() - want_y) <= 1.0
    area = np.pi * (W.R_O / W.SIDE * size) ** 2
    assert abs(k.sum() / 16.0 - area) <= 0.15 * area + 1.0


def test_the_centre_pixel_has_the_layers_colour():
    size = 64
    state = _state((1.50, 0.60, 0.42), (1.2831, 0.8177))
    frame = W.render(state[None], size)[0]
    assert tuple(frame[int(_pixel(0.8177, W.Y0, size)), int(_pixel(1.2831, W.X0, size))]) == W.OBJECT_RGB
    assert tuple(frame[int(_pixel(0.60, W.Y0, size)), int(_pixel(1.50, W.X0, size))]) == W.GRIPPER_RGB
    # the ring's centre is hollow: the table shows; a pixel on the ring's middle radius is the goal's colour
    gx, gy = _pixel(FAR_GOAL[0], W.X0, size), _pixel(FAR_GOAL[1], W.Y0, size)
    assert tuple(frame[int(gy), int(gx)]) in (W.TABLE, tuple(v - 12 for v in W.TABLE))
    on_ring = (W.R_O - W.RING / 2) / W.SIDE * size
    assert W.coverage(W.scene(state, 128)["goal"], 128).max() == 16
    assert abs(int(frame[int(gy), int(gx + on_ring)][1]) - W.GOAL_RGB[1]) < abs(int(frame[int(gy), int(gx)][1]) - W.GOAL_RGB[1])
    # the gripper is drawn over the object, the object over the shadow and the goal
    over = W.render(_state((1.30, 0.70, 0.55), (1.30, 0.70), (1.30, 0.70))[None], size)[0]
    assert tuple(over[int(_pixel(0.70, W.Y0, size)), int(_pixel(1.30, W.X0, size))]) == W.GRIPPER_RGB


def test_the_table_is_a_checkerboard_of_eight_cells():
    for size in (32, 36, 128):
        t = W.table(size)
        assert tuple(t[0, 0]) == W.TABLE and tuple(t[0, size // 8]) == tuple(v - 12 for v in W.TABLE)
        assert tuple(t[size // 8, size // 8]) == W.TABLE


@pytest.mark.parametrize("k", [1, 3, 7])
def test_moving_a_shape_by_k_pixels_moves_its_mask_by_k(k):
    size = 64
    a = _state((1.50, 0.60, 0.60), (1.30, 0.80))
    b = _state((1.50, 0.60, 0.60), (1.30 + k * W.SIDE / size, 0.80 + k * W.SIDE / size))
    ka, kb = (W.coverage(W.scene(s, size)["object"], size) for s in (a, b))
    assert W.scene(b, size)["object"][0] - W.scene(a, size)["object"][0] == 16 * k
    assert (np.roll(np.roll(ka, k, axis=0), k, axis=1) == kb).all() and ka.sum() == kb.sum()
    fa, fb = (W.render(s[None], size)[0] for s in (a, b))
    ma, mb = ((f == np.array(W.OBJECT_RGB, np.uint8)).all(axis=2) for f in (fa, fb))
    assert (np.roll(np.roll(ma, k, axis=0), k, axis=1) == mb).all()


def test_a_sixteenth_of_a_pixel_changes_the_frame_only_at_the_rim():
    states, actions = (np.stack(v) for v in zip(*[(s, a) for name, s, a in W.cases() if "sixteenth" in name]))
    after = W.step(states, actions)
    assert W.scene(after[0], 32)["gripper"][0] - W.scene(states[0], 32)["gripper"][0] == 1
    assert W.scene(after[1], 32)["gripper"][1] - W.scene(states[1], 32)["gripper"][1] == 2
    changed = (W.render(states, 32) != W.render(after, 32)).any(axis=3).sum(axis=(1, 2))
    assert (changed <= 40).all()


def test_the_height_shows_in_the_radius_and_in_the_shadow():
    low, high = (W.scene(_state((1.30, 0.70, z), (1.50, 0.90)), 128) for z in (W.Z_MIN, W.Z_MAX))
    assert high["gripper"][3] == 2 * low["gripper"][3]
    assert low["shadow"][0:2] == low["gripper"][0:2]
    assert high["shadow"][0] > high["gripper"][0] and high["shadow"][1] > high["gripper"][1]


# -------------------------------------------------------------------------------------------------------------- step
def test_the_step_does_what_the_words_say():
    by_name = {name: (s, a) for name, s, a in W.cases()}

    def after(name):
        s, a = by_name[name]
        return s, W.step(s[None], a[None])[0]

    s, n = after("r2 == 0")
    assert n[3] == np.float32(np.float64(s[0]) + W.R) and n[4] == s[4]
    s, n = after("at Z_CONTACT, the fp32 below it")
    assert (n[3:5] != s[3:5]).any()
    s, n = after("at Z_CONTACT, the fp32 above it")
    assert (n[3:5] == s[3:5]).all()
    s, n = after("a NaN action component")
    assert n[0] == s[0] and n[2] == s[2] and n[1] > s[1] and np.isfinite(n).all()
    s, n = after("actions beyond +-1")
    assert abs(n[0] - s[0] - W.STEP) < 1e-6 and abs(n[1] - s[1] + W.STEP) < 1e-6
    s, n = after("the block into the wall")
    assert n[3] == np.float32(W.X0 + W.SIDE - W.R_O) and n[3] - n[0] < W.R          # the gripper overlaps it
    s, n = after("the block into the corner")
    assert n[3] == np.float32(W.X0 + W.R_O) and n[4] == np.float32(W.Y0 + W.R_O)
    s, n = after("raised over the block")
    assert (n[3:5] == s[3:5]).all() and n[0] > s[0]
    s, n = after("descending onto the block")
    assert np.hypot(n[3] - n[0], n[4] - n[1]) >= W.R - 1e-6
    for name, s, a in W.cases():
        n = W.step(s[None], a[None])[0]
        assert (n[5:8] == s[5:8]).all(), name


# ------------------------------------------------------------------------------------------------------------ starts
@pytest.mark.parametrize("kind", P.STARTS)
def test_starts_keep_their_promises(kind):
    s = W.starts(kind, 0, np.arange(256)).astype(np.float64)
    assert s.dtype == np.float64 and s.shape == (256, 8)
    for x, y in ((0, 1), (3, 4), (6, 7)):
        assert (s[:, x] >= W.X0).all() and (s[:, x] <= W.X0 + W.SIDE).all()
        assert (s[:, y] >= W.Y0).all() and (s[:, y] <= W.Y0 + W.SIDE).all()
    assert (s[:, 3] >= W.X0 + W.R_O).all() and (s[:, 3] <= W.X0 + W.SIDE - W.R_O).all()
    assert (s[:, 6] >= W.X0 + W.R_O).all() and (s[:, 7] <= W.Y0 + W.SIDE - W.R_O).all()
    assert (s[:, 2] >= W.Z_MIN).all() and (s[:, 2] <= W.Z_MAX).all() and (s[:, 5] == np.float32(W.OBJECT_Z)).all()
    apart = np.hypot(s[:, 3] - s[:, 0], s[:, 4] - s[:, 1])
    assert ((s[:, 2] >= W.Z_CONTACT) | (apart > W.R)).all()                        # never in contact
    assert (np.hypot(s[:, 6] - s[:, 3], s[:, 7] - s[:, 4]) >= 0.06).all()
    stay = W.step(s.astype(np.float32), np.zeros((256, 4), np.float32))
    assert W.bits_equal(stay, s.astype(np.float32))                                # nothing moves by itself


@pytest.mark.parametrize("kind", P.STARTS)
def test_starts_depend_on_seed_and_index_alone(kind):
    many = W.starts(kind, 3, np.arange(40))
    assert W.bits_equal(W.starts(kind, 3, [7]), many[7:8])
    assert W.bits_equal(W.starts(kind, 3, [39, 0, 7]), many[[39, 0, 7]])
    assert not W.bits_equal(W.starts(kind, 4, np.arange(40)), many)
    assert len({row.tobytes() for row in many}) == 40


# ------------------------------------------------------------------------------------------------ expert and the floor
def _run(kind, policy, steps=14, n=256):
    s = W.starts(kind, 0, np.arange(n))
    gen = torch.Generator().manual_seed(1)
    for _ in range(steps):
        if policy == "random":
            a = (torch.rand(n, 4, generator=gen) * 2.0 - 1.0).numpy()
        else:
            a = P.expert_actions(torch.from_numpy(s)).numpy()
            assert a.dtype == np.float32 and a.shape == (n, 4) and np.abs(a).max() <= 1.0 and (a[:, 3] == 0).all()
        s = W.step(s, a)
    return np.hypot(s[:, 3] - s[:, 6], s[:, 4] - s[:, 7])


@pytest.mark.parametrize("kind", P.STARTS)
def test_the_expert_solves_the_task_and_chance_does_not(kind):
    expert, chance = _run(kind, "expert"), _run(kind, "random")
    print(kind, "expert success %.3f worst %.4f; random success %.3f" % ((expert < 0.05).mean(), expert.max(),
                                                                         (chance < 0.05).mean()))
    assert (expert < 0.05).mean() >= 0.95
    assert (chance < 0.05).mean() <= 0.10


def test_epsilon_replaces_actions_by_the_uniform_draws():
    s = torch.from_numpy(W.starts("scattered", 0, np.arange(64)))
    uni = torch.rand(64, 5, generator=torch.Generator().manual_seed(2))
    plain = P.expert_actions(s)
    mixed = P.expert_actions(s, uniform=uni, epsilon=0.5)
    swapped = uni[:, 4] < 0.5
    assert 10 < int(swapped.sum()) < 54
    assert torch.equal(mixed[swapped], (2.0 * uni[:, 0:4] - 1.0)[swapped]) and torch.equal(mixed[~swapped], plain[~swapped])
    assert torch.equal(P.expert_actions(s, uniform=uni, epsilon=0.0), plain)
    assert torch.equal(P.expert_actions(s, uniform=uni, epsilon=1.0), 2.0 * uni[:, 0:4] - 1.0)


def test_a_move_lands_exactly_on_its_target():
    delta = torch.tensor([[0.02, -0.01, 0.0], [0.12, 0.06, -0.03]], dtype=torch.float64)
    a = P._towards(delta)
    assert torch.allclose(a[0] * W.STEP, delta[0]) and float(a[1].abs().max()) == 1.0
    assert torch.allclose(a[1] / a[1, 0], delta[1] / delta[1, 0])


# ------------------------------------------------------------------------------------------------------------ golden
def test_the_golden_file_is_reproduced():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_push_world",
                                                  os.path.join(os.path.dirname(GOLDEN), "make_golden_push_world.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    want, got = np.load(GOLDEN), maker.build()
    assert sorted(want.files) == sorted(got)
    assert os.path.getsize(GOLDEN) < 400 * 1024
    for key in want.files:
        if key == "names":
            assert list(want[key]) == list(got[key])
        else:
            assert W.bits_equal(want[key], got[key]), key
    assert len(want["states"]) == 12 and want["frames32"].shape == (12, 32, 32, 3) and want["frame128"].shape == (128, 128, 3)


# ---------------------------------------------------------------------------------------------------------- refusals
def test_bad_arguments_are_refused_without_a_gpu(tmp_path, monkeypatch):
    def no_gpu(*a, **k):
        raise AssertionError("a refused argument reached the library")
    monkeypatch.setattr(P._capi, "load", no_gpu)
    for size in (0, 30, 34, 28, 1028, 2048, 127, 64.5):
        with pytest.raises(ValueError):
            P.PushWorld(2, "cuda:0", frame_size=size)
    for n in (0, -1, 65536, 1.5):
        with pytest.raises(ValueError):
            P.PushWorld(n, "cuda:0")
    with pytest.raises(ValueError):
        P.PushWorld(2, "cuda:0", start="random")
    with pytest.raises(ValueError):
        P.PushWorld(2, "cuda:0", seed=-1)
    state = torch.from_numpy(W.starts("simplified", 0, [0, 1]))
    for eps in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            P.expert_actions(state, epsilon=eps)
        with pytest.raises(ValueError):
            P.generate(4, str(tmp_path / "d"), epsilon=eps)
    with pytest.raises(ValueError):
        P.expert_actions(state[:, :7])
    with pytest.raises(ValueError):
        P.expert_actions(state, uniform=torch.zeros(2, 4), epsilon=0.5)
    with pytest.raises(ValueError):
        P.generate(0, str(tmp_path / "d"))
    with pytest.raises(ValueError):
        P.generate(4, str(tmp_path / "d"), start="nowhere")
    with pytest.raises(ValueError):
        P.generate(4, str(tmp_path / "d"), frame_size=64)
    with pytest.raises(ValueError):
        P.generate(4, str(tmp_path / "d"), steps=0)
    with pytest.raises(ValueError):
        P.starts("nowhere", 0, [0])
    assert not (tmp_path / "d").exists()
    world = P.PushWorld.__new__(P.PushWorld)                  # step checks the actions before it looks at anything else
    world.n = 3
    for bad in (np.zeros((2, 4), np.float32), np.zeros((3, 3), np.float32), np.zeros(12, np.float32)):
        with pytest.raises(ValueError):
            world.step(bad)
    with pytest.raises(ValueError):
        P.main(["generate", "4", str(tmp_path / "d"), "--epsilon", "2"])
    with pytest.raises(ValueError):
        P.main(["mpc", "--config-file", os.path.join(os.path.dirname(GOLDEN), "..", "..", "config", "evaluation.yaml"),
                "--envs", "0"])
