"""The generate_trajectories drop-in on the MI355X against tests/golden/generate_case.npz, which
tests/golden/make_golden_generate.py records by running the REFERENCE's own generate_trajectory (PIL resize, PIL save) on
the same stand-ins: `PushEnv25`, a small subclass of tests/fake_push_env.py with a 25-value observation, and a seeded
two-layer actor.  Streams must be byte-equal; states, actions and goal equal.

So that equality does not ride on the order of a sum, the stand-ins compute exactly: observations and goals are snapped
to multiples of 1/64, the normaliser's means are such multiples and its deviations powers of two, the actor's weights are
multiples of 1/4 and its activations clamp to [-1, 1] -- every product and sum of the actor is exact in fp32 (at most 16
significant bits in the first layer, 15 in the second)."""
import hashlib
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
from fake_push_env import FakePushEnv

pytestmark = pytest.mark.gpu

T = 4
CASES = (("plain", False, False), ("simplified", True, False), ("simplified_inline", True, True))
NP_SEED = 7


def digest(a):
    return np.frombuffer(hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=16).digest(), np.uint8)


def snap(v):
    return np.round(np.asarray(v, np.float64) * 64.0) / 64.0


class PushEnv25(FakePushEnv):
    """FakePushEnv with what generate_trajectories.py touches beyond MPC_gym_eval.py: a 25-value observation,
    initial_gripper_xpos and height_offset."""
    initial_gripper_xpos = np.array([1.34375, 0.75, 0.53125])
    height_offset = 0.421875

    def reset(self):
        self.steps = 0
        return super().reset()

    def step(self, action):
        super().step(action)
        self.steps += 1
        self.gripper = snap(self.gripper)
        self.object_qpos[:3] = snap(self.object_qpos[:3])
        return self._get_obs(), 0.0, False, {}

    def _get_obs(self):
        obs = np.zeros(25)
        obs[0:3], obs[3:6] = snap(self.gripper), snap(self.object_qpos[:3])
        obs[6:9] = obs[3:6] - obs[0:3]
        obs[9] = getattr(self, "steps", 0) / 8.0
        return {"observation": obs, "achieved_goal": obs[3:6].copy(), "desired_goal": snap(self.goal)}


def make_actor(seed=3):
    gen = torch.Generator().manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(28, 16), torch.nn.Hardtanh(), torch.nn.Linear(16, 4), torch.nn.Hardtanh())
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randint(-4, 5, p.shape, generator=gen).float() / 4.0)
    return net.eval()


def normalizer():
    rng = np.random.RandomState(11)
    o_mean = snap(np.concatenate([[1.3, 0.7, 0.5, 1.3, 0.7, 0.4], rng.uniform(-0.2, 0.2, 19)]))
    o_std = 2.0 ** rng.randint(-3, 1, 25)
    g_mean = snap([1.3, 0.7, 0.4])
    g_std = np.array([0.25, 0.125, 0.5])
    return o_mean, o_std, g_mean, g_std


def make_args(simplify, inline):
    return types.SimpleNamespace(simplify_task=simplify, goal_inline=inline, trajectory_length=T, image_shape=(128, 128),
                                 clip_obs=200, clip_range=5)


def run(generate_trajectory, simplify, inline):
    """One trajectory of `generate_trajectory` (the drop-in's or the reference's) on fresh stand-ins."""
    np.random.seed(NP_SEED)
    env = PushEnv25()
    env.goal = np.array([1.5, 0.9, 0.421875])
    frames, states, actions, goal = generate_trajectory(env, make_actor(), make_args(simplify, inline))
    return env, frames, states, actions, goal


@pytest.fixture(scope="module")
def case():
    return load_golden("generate_case")


@pytest.mark.parametrize("name,simplify,inline", CASES)
def test_generate_trajectory_equals_the_reference_s(case, name, simplify, inline, monkeypatch):
    import generate_trajectories as root
    from ndivplanning_amd import generate_trajectories as G
    assert root.generate_trajectory is G.generate_trajectory
    for k, v in zip(("o_mean", "o_std", "g_mean", "g_std"), normalizer()):
        monkeypatch.setattr(G, k, v)
    env, frames, states, actions, goal = run(G.generate_trajectory, simplify, inline)
    assert isinstance(frames, list) and len(frames) == T and all(isinstance(b, bytes) for b in frames)
    assert np.array_equal(digest(np.stack(env.rendered)), case[name + ".rendered_digest"]), "the environment rendered other frames"
    off = case[name + ".offsets"]
    want = [case[name + ".streams"][off[i]:off[i + 1]].tobytes() for i in range(T)]
    assert [len(b) for b in frames] == [len(b) for b in want]
    assert frames == want
    assert states.shape == (T, 25) and actions.shape == (T, 4) and states.dtype == actions.dtype == np.float64
    assert np.array_equal(states, case[name + ".states"]) and np.array_equal(actions, case[name + ".actions"])
    assert np.array_equal(goal, case[name + ".goal"])
    assert len({case[n + ".streams"].tobytes() for n, _, _ in CASES}) == len(CASES)       # the branches differ


def test_args_normalizer_takes_precedence_and_a_missing_one_is_reported(case):
    from ndivplanning_amd import generate_trajectories as G
    args = make_args(False, False)
    np.random.seed(NP_SEED)
    env = PushEnv25()
    env.goal = np.array([1.5, 0.9, 0.421875])
    with pytest.raises(ValueError, match="normaliser"):
        G.generate_trajectory(env, make_actor(), args)
    args.normalizer = normalizer()
    frames, states, actions, goal = G.generate_trajectory(env, make_actor(), args)
    assert np.array_equal(actions, case["plain.actions"]) and np.array_equal(states, case["plain.states"])
