"""CPU-only checks of the live-environment MPC drop-in (MPC_gym_eval.py): the new noise kind, the fixture
tests/golden/mpc_gym_case.npz (from the reference's own script, tests/golden/make_golden_mpc_gym.py) against the oracle
restatement, the fake environment, and the errors the drop-in raises before it touches a GPU."""
import sys
import types

import numpy as np
import pytest
import torch

import eval_oracle as EV
import mpc_gym_oracle as MG
from conftest import load_golden
from fake_push_env import FakePushEnv


@pytest.fixture(scope="module")
def case():
    return load_golden("mpc_gym_case")


def test_noise_kind_shapes_and_order():
    from ndivplanning_amd import evaluation as E
    shapes = E.noise_piece_shapes("mpc_gym", 1, 6, 1, 2, rollouts=5, horizon=3)
    assert shapes == [(5, 1, 2)] * (5 * 3)                    # Th pieces per planning step: the horizon never shrinks
    assert len(E.noise_piece_shapes("mpc", 1, 6, 1, 2, rollouts=5, horizon=3)) == 3 + 3 + 3 + 2 + 1
    with pytest.raises(ValueError, match="num_sample"):
        E.noise_piece_shapes("mpc_gym", 1, 6, 2, 2, rollouts=5, horizon=3)
    with pytest.raises(ValueError):
        E.noise_piece_shapes("gym", 1, 6, 1, 2, rollouts=5, horizon=3)
    assert E.plan_step_noise_floats(3, 5, 4, 2) == 4 * 3 * 5 * 2


def test_noise_schedule_is_the_reference_script_s_stream(case):
    from ndivplanning_amd import evaluation as E
    n, t, r, th, seed, nz, _ = case["meta"].tolist()
    per = E.reference_noise_schedule("mpc_gym", seed, n, 1, t, 1, nz, r, th)
    assert len(per) == n and all(p.numel() == (t - 1) * th * r * nz for p in per)
    assert np.array_equal(torch.cat(per).numpy(), case["noise"])


def test_fixture_against_the_oracle_restatement(case):
    """The fp32 oracle restatement on the recorded frames makes the reference's choices by itself, and its numbers lie
    within the fixture's own fp32-to-fp64 distance (x 50, as tests/test_gpu_eval.py takes it)."""
    n, t, r, th, seed, nz, data_seed = case["meta"].tolist()
    assert (n, t, r, th, seed, nz) == (MG.N_TRAJ, MG.SEQ, MG.ROLLOUTS, MG.HORIZON, MG.RUN_SEED, EV.NOISE_DIM)
    states = EV.case_states()
    assert np.allclose(np.stack([EV.checksum(s) for s in states]), case["state_checksums"], rtol=1e-12)
    bound = np.abs(case["rollout_errors"] - case["rollout_errors_fp64"]).max(axis=1)
    assert (case["margins"] >= 100 * bound).all() and (case["margins"] > 0).all()
    env = FakePushEnv(replay=case["frames"])
    four, rec = MG.run(*EV.oracle_callables(*states), MG.GymTrajectories(data_seed), env)
    assert rec["choices"] == case["choices"].tolist()
    assert np.array_equal(torch.cat([p.reshape(-1) for p in rec["pieces"]]).numpy(), case["noise"])
    assert np.array_equal(np.stack(rec["states_u8"]), case["states_u8"])       # this machine's PIL against the recorded one

    def close(got, key, rel=1e-5):
        got = np.asarray(got, np.float64).reshape(-1)
        want, want64 = case[key].reshape(-1), case[key + "_fp64"].reshape(-1)
        tol = np.maximum(50.0 * np.abs(want - want64), rel * np.abs(want64))
        assert (np.abs(got - want64) <= tol).all(), (key, got, want64, tol)
    close(rec["rollout_errors"], "rollout_errors")
    close(rec["image_errors"], "image_errors")
    close(torch.cat(rec["actions"]).numpy(), "actions")
    close(four, "four")
    close(torch.stack(rec["gen_out"]).numpy(), "gen_out")                       # every generator output,
    close(np.array(rec["fm_out_sums"]), "fm_out_sums")                          # every forward-model output by its sums
    assert np.allclose(rec["goal_errors"], case["goal_errors"], rtol=1e-6)
    assert np.isclose(np.mean(case["goal_errors"]), case["four"][2], rtol=1e-9) and case["four"][3] in (0.0, 0.5, 1.0)


def test_fake_environment_is_deterministic_and_replays(case):
    n, t, r, th, seed, nz, data_seed = case["meta"].tolist()
    data = MG.GymTrajectories(data_seed)
    env = FakePushEnv()
    acts = case["actions"].reshape(n, t - 1, 4)
    for traj in range(n):
        _, states, _, goal = data[traj]
        MG.controlled_reset(env, states[None].numpy(), goal[None].numpy())
        assert np.allclose(env.sim.data.get_joint_qpos("object0:joint")[:2], states[0, 3:5].numpy())
        assert np.allclose(env._get_obs()["desired_goal"], goal.numpy())
        for i in range(t - 1):
            env.step(acts[traj, i])
            frame = env.render(mode="rgb_array")
            assert frame.shape == (120, 160, 3) and frame.dtype == np.uint8
    assert np.array_equal(np.stack(env.rendered), case["frames"])               # the frames the reference's run saw
    assert len({f.tobytes() for f in env.rendered}) == len(env.rendered)        # the actions move what is drawn
    replay = FakePushEnv(replay=case["frames"])
    for k in range(len(case["frames"])):
        replay.step(np.array([1.0, -1.0, 0.5, 0.0]))                            # whatever the action
        assert np.array_equal(replay.render(mode="rgb_array"), case["frames"][k])
    with pytest.raises(AssertionError):
        env.render()                                                            # only rgb_array, as the script asks


def test_main_without_gym_says_whose_the_environment_is(monkeypatch):
    import MPC_gym_eval
    monkeypatch.setitem(sys.modules, "gym", None)              # `import gym` fails here, installed or not
    with pytest.raises(ImportError, match="fetch_push_control_evaluation") as e:
        MPC_gym_eval.main(["--config-file", "config/evaluation.yaml"])
    assert "caller's to supply" in str(e.value)
    with pytest.raises(SystemExit) as e:
        MPC_gym_eval.main(["--help"])
    assert e.value.code == 0


class _Stub(torch.nn.Module):
    noise_dim = 2


def _config(bs=1, k=1, r=2):
    ns = types.SimpleNamespace
    return ns(random_seed=0, gpu_id=0, evaluation=ns(num_sample=k, noise_dim=2, batch_size=bs, threshold=0.05),
              mpc=ns(rollouts=r, time_horizon=2))


def test_dropin_refuses_what_the_reference_cannot_do():
    import MPC_gym_eval
    data = MG.GymTrajectories(41)
    m = _Stub()
    args = types.SimpleNamespace(image_shape=(128, 128))
    with pytest.raises(ValueError, match="image-shape"):
        MPC_gym_eval.fetch_push_control_evaluation(types.SimpleNamespace(image_shape=(64, 64)), m, m, m, data, _config(), None)
    with pytest.raises(ValueError, match="batch_size"):
        MPC_gym_eval.fetch_push_control_evaluation(args, m, m, m, data, _config(bs=2), None)
    with pytest.raises(ValueError, match="num_sample"):
        MPC_gym_eval.fetch_push_control_evaluation(args, m, m, m, data, _config(k=2), None)
    with pytest.raises(ValueError, match="rollouts"):
        MPC_gym_eval.fetch_push_control_evaluation(args, m, m, m, data, _config(r=1), None)
    for name in ("render", "get_state", "controlled_reset", "norm", "denorm", "fetch_push_control_evaluation", "main"):
        assert callable(getattr(MPC_gym_eval, name)), name
