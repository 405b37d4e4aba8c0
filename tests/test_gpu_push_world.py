"""GPU tests of the push world (ndp_world_step_render, ndp_world_render, ndivplanning_amd/push_world.py) against the numpy
restatement of include/ndp.h's definition (tests/world_common.py): frames bit for bit, states to within 1 fp32 ulp (the
device's fp64 sqrt and divide), then everything that sits on top -- the gym view under both drop-ins, the data
generator, the batched closed loop."""
import ctypes
import types

import numpy as np
import pytest
import torch

import eval_oracle as EV
import world_common as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(32, 1), (32, 3), (32, 65), (36, 1), (36, 3), (36, 65), (128, 1), (128, 3), (128, 65), (256, 1)]


@pytest.fixture(scope="module")
def lib():
    from ndivplanning_amd import _build, _capi
    _build.build()
    return _capi.load()


@pytest.fixture(scope="module")
def P(lib):
    from ndivplanning_amd import push_world
    return push_world


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _render(lib, states, size):
    s = torch.from_numpy(np.ascontiguousarray(states)).to(DEV)
    frames = torch.full((len(states), size, size, 3), 7, dtype=torch.uint8, device=DEV)
    assert lib.ndp_world_render(_ptr(s), len(states), size, _ptr(frames), _stream()) == 0, lib.ndp_last_error()
    return frames.cpu().numpy()


def _step(lib, states, actions, size, with_frames=True):
    n = len(states)
    s = torch.from_numpy(np.ascontiguousarray(states)).to(DEV)
    a = torch.from_numpy(np.ascontiguousarray(actions)).to(DEV)
    out = torch.full((n, 8), -7.0, dtype=torch.float32, device=DEV)
    frames = torch.full((n, size, size, 3), 7, dtype=torch.uint8, device=DEV) if with_frames else None
    rc = lib.ndp_world_step_render(_ptr(s), _ptr(a), n, size, _ptr(out), _ptr(frames), _stream())
    assert rc == 0, lib.ndp_last_error()
    return out.cpu().numpy(), None if frames is None else frames.cpu().numpy()


# ------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("size,n", SHAPES)
def test_render_is_bit_equal_to_the_restatement(lib, size, n):
    states, _ = W.case_arrays(n)
    got, want = _render(lib, states, size), W.render(states, size)
    assert W.bits_equal(got, want), np.argwhere(got != want)[:6]


@pytest.mark.parametrize("size,n", SHAPES)
def test_step_render_against_the_restatement(lib, size, n):
    states, actions = W.case_arrays(n)
    got_state, got_frames = _step(lib, states, actions, size)
    want_state = W.step(states, actions)
    ulps = W.ulp_distance(got_state, want_state)
    print("size %d n %d: %d of %d state components differ from the restatement, the farthest by %d ulp"
          % (size, n, int((ulps > 0).sum()), ulps.size, int(ulps.max())))
    assert np.isfinite(got_state).all() and ulps.max() <= 1, np.argwhere(ulps > 1)[:6]
    want_frames = W.render(got_state, size)                         # of the state the device wrote
    assert W.bits_equal(got_frames, want_frames), np.argwhere(got_frames != want_frames)[:6]


def test_a_step_without_frames_writes_the_same_state(lib):
    states, actions = W.case_arrays(65)
    with_frames, _ = _step(lib, states, actions, 36)
    without, none = _step(lib, states, actions, 36, with_frames=False)
    assert none is None and W.bits_equal(with_frames, without)


def test_argument_errors_launch_nothing(lib):
    states, actions = W.case_arrays(3)
    s = torch.from_numpy(states).to(DEV)
    a = torch.from_numpy(actions).to(DEV)
    out = torch.full((3, 8), -7.0, dtype=torch.float32, device=DEV)
    frames = torch.full((3, 32, 32, 3), 7, dtype=torch.uint8, device=DEV)
    st = _stream()
    bad = [lib.ndp_world_step_render(_ptr(s), _ptr(a), 3, size, _ptr(out), _ptr(frames), st) for size in (0, 28, 30, 34, 1028)]
    bad += [lib.ndp_world_step_render(_ptr(s), _ptr(a), n, 32, _ptr(out), _ptr(frames), st) for n in (0, -1, 65536)]
    bad.append(lib.ndp_world_step_render(None, _ptr(a), 3, 32, _ptr(out), _ptr(frames), st))
    bad.append(lib.ndp_world_step_render(_ptr(s), None, 3, 32, _ptr(out), _ptr(frames), st))
    bad.append(lib.ndp_world_step_render(_ptr(s), _ptr(a), 3, 32, None, _ptr(frames), st))
    bad.append(lib.ndp_world_step_render(_ptr(s), _ptr(a), 3, 32, _ptr(s), _ptr(frames), st))
    assert b"aliases" in lib.ndp_last_error()
    bad += [lib.ndp_world_render(_ptr(s), 3, size, _ptr(frames), st) for size in (0, 30, 2048)]
    bad += [lib.ndp_world_render(_ptr(s), n, 32, _ptr(frames), st) for n in (0, 65536)]
    bad.append(lib.ndp_world_render(None, 3, 32, _ptr(frames), st))
    bad.append(lib.ndp_world_render(_ptr(s), 3, 32, None, st))
    assert bad == [1] * len(bad), bad                               # NDP_E_ARG
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((frames == 7).all()) and W.bits_equal(s.cpu().numpy(), states)


# ------------------------------------------------------------------------------------------------------ the Python surface
def _expert_run(P, world, steps):
    """[(state, frames, actions)] of `steps` expert steps from the world's current state, on the host."""
    out = []
    for _ in range(steps):
        actions = P.expert_actions(world.state)
        frames = world.step(actions)
        out.append((world.state.cpu().numpy().copy(), frames.cpu().numpy(), actions.cpu().numpy()))
    return out


def test_a_15_step_expert_trajectory_of_65_environments_twice(P):
    runs = []
    for _ in range(2):
        world = P.PushWorld(65, DEV, frame_size=36, seed=4, start="scattered")
        first = world.reset().cpu().numpy()
        runs.append((first, _expert_run(P, world, 15), world.goal_distance().cpu().numpy()))
    assert W.bits_equal(runs[0][0], runs[1][0]) and W.bits_equal(runs[0][0], W.render(W.starts("scattered", 4, np.arange(65)), 36))
    for (s0, f0, a0), (s1, f1, a1) in zip(runs[0][1], runs[1][1]):
        assert W.bits_equal(s0, s1) and W.bits_equal(f0, f1) and W.bits_equal(a0, a1)
    assert len({f.tobytes() for _, f, _ in runs[0][1]}) > 5         # it moves
    assert (runs[0][2] < 0.05).mean() >= 0.95                       # and the expert pushes the device's world home too
    # every step of the trajectory follows the restatement to within an ulp, every frame bit for bit
    state = W.starts("scattered", 4, np.arange(65))
    for t, (got, frames, actions) in enumerate(runs[0][1]):
        assert W.ulp_distance(got, W.step(state, actions)).max() <= 1
        if t in (0, 7, 14):
            assert W.bits_equal(frames, W.render(got, 36))
        state = got


def test_world_accessors_and_host_actions(P):
    world = P.PushWorld(3, DEV, frame_size=32, seed=1)
    start = W.starts("simplified", 1, np.arange(3))
    assert W.bits_equal(world.state.cpu().numpy(), start)
    assert W.bits_equal(world.observation().cpu().numpy(), W.observation(start))
    assert W.bits_equal(world.goal3().cpu().numpy()[:, :2], start[:, 6:8]) and float(world.goal3()[0, 2]) == np.float32(W.OBJECT_Z)
    want = np.hypot(start[:, 3] - start[:, 6], start[:, 4] - start[:, 7])
    assert np.allclose(world.goal_distance().cpu().numpy(), want, rtol=1e-6)
    assert world.success(1.0).all() and not world.success(0.01).any()
    act = np.array([[1, 0, 0, 0], [0, -0.5, 0.5, 0], [0.25, 0.25, 0, 1]], np.float32)
    host = world.step(act).cpu().numpy()                            # host actions
    after = world.state.cpu().numpy().copy()
    world.reset()
    dev = world.step(torch.from_numpy(act).to(DEV)).cpu().numpy()    # device actions
    assert W.bits_equal(host, dev) and W.bits_equal(after, world.state.cpu().numpy())
    assert W.bits_equal(world.render().cpu().numpy(), host)
    custom = W.case_arrays(3)[0]
    world.set_state(custom)
    assert W.bits_equal(world.render().cpu().numpy(), W.render(custom, 32))
    assert W.bits_equal(world.reset(seed=9, index=[5, 0, 2]).cpu().numpy(), W.render(W.starts("simplified", 9, [5, 0, 2]), 32))
    for bad in (np.zeros((2, 4), np.float32), np.zeros((3, 3), np.float32)):
        with pytest.raises(ValueError):
            world.step(bad)
    with pytest.raises(ValueError):
        world.set_state(np.zeros((3, 7), np.float32))


def test_a_batched_world_equals_single_worlds(P):
    singles = []
    for i in range(3):
        world = P.PushWorld(1, DEV, frame_size=32, seed=2, start="scattered")
        world.reset(index=i)
        actions = []
        trace = []
        for _ in range(6):
            actions.append(P.expert_actions(world.state).cpu())
            frames = world.step(actions[-1])
            trace.append((world.state.cpu().numpy().copy(), frames.cpu().numpy()))
        singles.append((actions, trace))
    world = P.PushWorld(3, DEV, frame_size=32, seed=2, start="scattered")
    for t in range(6):
        frames = world.step(torch.cat([singles[i][0][t] for i in range(3)])).cpu().numpy()
        state = world.state.cpu().numpy()
        for i in range(3):
            assert W.bits_equal(state[i:i + 1], singles[i][1][t][0]) and W.bits_equal(frames[i:i + 1], singles[i][1][t][1])


def test_generate_writes_bundles_the_loaders_read_back(P, tmp_path):
    from ndivplanning_amd.jpeg import JpegDecoder, pack_jpegs
    from ndivplanning_amd.utils.trajectory_loader import PushDataset
    out_dir = str(tmp_path / "push")
    written = P.generate(6, out_dir, steps=4, seed=3, epsilon=0.5, start="scattered", batch=4, per_file=5)
    assert [p.rsplit("/", 1)[1] for p in written] == ["trajectory_bundle_00001.ndpt", "trajectory_bundle_00002.ndpt"]
    data = PushDataset(out_dir, seq_length=4, raw_jpeg=True)
    assert len(data) == 6
    decoder = JpegDecoder(DEV)
    at = 0
    for lo, m in ((0, 4), (4, 2)):                                  # the generator's batches, run again
        world = P.PushWorld(m, DEV, seed=3, start="scattered")
        world.reset(index=lo, render=False)
        goal = world.goal3().cpu()
        frames = torch.empty(4, m, 128, 128, 3, dtype=torch.uint8, device=DEV)
        states, actions = P.rollout(world, 4, 0.5, torch.Generator().manual_seed(3 * 1000003 + lo), frames)
        rendered = frames.cpu().numpy()
        for i in range(m):
            streams, s, a, g = data[at]
            at += 1
            assert torch.equal(s, states[:, i].cpu()) and torch.equal(a, actions[:, i].cpu()) and torch.equal(g, goal[i])
            buffer, offsets = pack_jpegs(streams, pin=False)
            decoded = decoder.decode(buffer, offsets).cpu().numpy().reshape(4, 128, 128, 3)
            _check_jpeg_error(decoded, rendered[:, i])
    assert float(torch.stack([data[i][2] for i in range(6)]).abs().max()) <= 1.0
    # frame t shows the state of row t: the recorded object position lies under the object's colour
    streams, s, _, _ = data[0]
    world = P.PushWorld(1, DEV, seed=3, start="scattered")
    state0 = world.state.cpu().numpy()
    assert np.array_equal(s[0, 0:6].numpy(), state0[0, 0:6])


def _check_jpeg_error(decoded, rendered):
    """A 16x16 MCU whose pixels are all one colour has only DC coefficients.  At quality 95 their steps are 2 (luma: 16
    scaled by 10 %) and 2 (chroma: 17), an eighth of a level per pixel; what remains is rounding: RGB -> YCbCr (half a level
    per component), the inverse DCT and YCbCr -> RGB, whose largest gain is 1.772 (Cb into B): at most
    0.7 + 1.772 * 0.7 + 0.5 = 2.4 levels, 3 after rounding.  Fancy chroma upsampling mixes in the neighbouring MCU's sample
    only on the MCU's outermost pixels, so the bound is asserted on the 14x14 interior of such MCUs."""
    assert decoded.shape == rendered.shape and decoded.dtype == np.uint8
    t = rendered.shape[0]
    tiles = rendered.reshape(t, 8, 16, 8, 16, 3)
    flat = (tiles == tiles[:, :, :1, :, :1, :]).all(axis=(2, 4, 5))                           # [t,8,8]
    assert flat.mean() >= 0.5
    err = np.abs(decoded.astype(np.int32) - rendered.astype(np.int32)).reshape(t, 8, 16, 8, 16, 3)[:, :, 1:15, :, 1:15, :]
    worst = err.max(axis=(2, 4, 5))
    print("JPEG error: flat MCUs %.2f, worst inside them %d levels, worst anywhere %d" % (flat.mean(), worst[flat].max(),
                                                                                        worst.max()))
    assert worst[flat].max() <= 3


# ----------------------------------------------------------------------------------------------- under the two drop-ins
def test_generate_trajectory_runs_on_the_gym_view(P):
    import generate_trajectories
    world = P.PushWorld(2, DEV, seed=5)
    env = P.GymPushEnv(world, index=1)
    args = types.SimpleNamespace(simplify_task=True, goal_inline=True, trajectory_length=4, image_shape=(128, 128),
                                 clip_obs=200, clip_range=5, device=DEV,
                                 normalizer=(np.zeros(25), np.ones(25), np.zeros(3), np.ones(3)))
    other = world.state[0].cpu().numpy().copy()
    np.random.seed(3)
    frames, states, actions, goal = generate_trajectories.generate_trajectory(
        env, lambda x: torch.tensor([[0.5, 0.25, 0.0, 0.0]]), args)
    assert len(frames) == 4 and all(bytes(f[:2]) == b"\xff\xd8" for f in frames)
    assert states.shape == (4, 25) and actions.shape == (4, 4) and goal.shape == (3,)
    assert np.allclose(states[0, 0:3], [W.REST[0], W.REST[1], 0.44], atol=1e-6)
    assert np.allclose(np.hypot(*(states[0, 3:5] - states[0, 0:2])), 0.056, atol=1e-6)
    assert np.allclose(states[1:, 0] - states[:-1, 0], 0.025, atol=1e-6) and goal[2] == env.height_offset
    assert np.allclose(states[:, 6:9], states[:, 3:6] - states[:, 0:3], atol=1e-7)
    assert np.allclose(env.goal, goal) and W.bits_equal(world.state[0].cpu().numpy(), other)   # the neighbour stayed
    obs, reward, done, info = env.step(np.zeros(4))
    assert reward == 0.0 and done is False and info == {} and set(obs) == {"observation", "achieved_goal", "desired_goal"}
    frame = env.render(mode="rgb_array")
    assert isinstance(frame, np.ndarray) and frame.shape == (128, 128, 3) and frame.dtype == np.uint8
    assert W.bits_equal(frame[None], W.render(world.state[1:2].cpu().numpy(), 128))


def _modules():
    from ndivplanning_amd.models.forward_encoder import ForwardAutoencoder
    from ndivplanning_amd.models.gan import Decoder
    from ndivplanning_amd.models.image_autoencoder import Encoder
    enc_s, fm_s, g_s = EV.case_states()
    enc, fm, gen = Encoder(), ForwardAutoencoder(), Decoder(EV.NOISE_DIM)
    enc.load_state_dict(enc_s)
    fm.load_state_dict(fm_s)
    gen.load_state_dict(g_s)
    return enc.to(DEV).eval(), fm.to(DEV).eval(), gen.to(DEV).eval()


class _PushTrajectories(torch.utils.data.Dataset):
    """(images uint8 [T,128,128,3], states [T,25], actions [T,4], goal [3]) of n expert trajectories, as PushDataset
    yields them with raw_uint8."""

    def __init__(self, P, n, seq_length, seed):
        world = P.PushWorld(n, DEV, seed=seed)
        frames = torch.empty(seq_length, n, 128, 128, 3, dtype=torch.uint8, device=DEV)
        self.goal = world.goal3().cpu()
        states, actions = P.rollout(world, seq_length, frames=frames)
        self.frames, self.states, self.actions = frames.cpu(), states.cpu(), actions.cpu()
        self.seq_length = seq_length

    def __len__(self):
        return int(self.goal.shape[0])

    def __getitem__(self, i):
        return self.frames[:, i], self.states[:, i], self.actions[:, i], self.goal[i]


def test_mpc_gym_eval_runs_on_the_gym_view(P):
    import MPC_gym_eval
    from ndivplanning_amd.utils.file import DotMap
    config = DotMap({"random_seed": 5, "gpu_id": 0,
                     "evaluation": {"batch_size": 1, "num_sample": 1, "noise_dim": EV.NOISE_DIM, "threshold": 0.05},
                     "mpc": {"rollouts": 2, "time_horizon": 1}})
    data = _PushTrajectories(P, 2, 3, seed=6)
    env = P.GymPushEnv(P.PushWorld(1, DEV, seed=6))
    record = []
    four = MPC_gym_eval.fetch_push_control_evaluation(types.SimpleNamespace(image_shape=(128, 128)), *_modules(), data,
                                                      config, env, record=record)
    assert len(four) == 4 and all(np.isfinite(v) for v in four) and 0.0 <= four[3] <= 1.0
    assert len(record) == 2 * 2
    # controlled_reset put the block where the trajectory starts and made its goal the environment's
    assert np.allclose(env.goal, data.goal[1].numpy())


def test_closed_loop_mpc_twice_and_evaluate(P):
    from ndivplanning_amd import evaluation as E
    models = E.EvalModels(*_modules(), DEV)
    runs = []
    for _ in range(2):
        world = P.PushWorld(3, DEV, seed=8)
        for _ in range(3):
            world.step(P.expert_actions(world.state), render=False)
        goal_frames = world.render()
        world.reset(render=False)
        run = P.closed_loop_mpc(models, world, goal_frames, steps=3, rollouts=3, horizon=2, seed=1)
        runs.append((run, world.state.cpu().numpy().copy()))
    (a, sa), (b, sb) = runs
    assert tuple(a["actions"].shape) == (3, 3, 4) and tuple(a["distance"].shape) == (3,) and a["success"].dtype == torch.bool
    assert torch.equal(a["actions"], b["actions"]) and torch.equal(a["distance"], b["distance"]) and W.bits_equal(sa, sb)
    assert torch.isfinite(a["actions"]).all()          # a random-weight generator proposes beyond +-1: the world clamps
    # the gripper went where the chosen actions lead: an ulp per step at the most (its path has no sqrt and no divide
    # by a computed value, so nothing amplifies a rounding difference)
    state = W.starts("simplified", 8, np.arange(3))
    for t in range(3):
        state = W.step(state, a["actions"][t].numpy())
    assert W.ulp_distance(sa[:, 0:3], state[:, 0:3]).max() <= 3
    result = P.evaluate_mpc(models, 3, 3, rollouts=2, horizon=1, seed=8)
    assert set(result) == {"expert", "random", "mpc", "mpc_actions"}
    for policy in ("expert", "random", "mpc"):
        assert np.isfinite(result[policy]["distance"]) and 0.0 <= result[policy]["success"] <= 1.0
    assert result["expert"]["distance"] < result["random"]["distance"]
