"""CPU tests of the planner's call sequence (ndivplanning_amd/evaluation.py: mpc_plan, plan_step): what it asks of
EvalModels, in order, read on the recording stand-in of tests/plan_common.py.  One entry of the list is one launch (or
a few) on the device, so these lists are the planner's launch pattern."""
import pytest
import torch

import plan_common as C
from ndivplanning_amd import evaluation as E

B, T, R, TH = 2, 5, 4, 3
BR = B * R


def _inputs(t=T, seed=0):
    g = torch.Generator().manual_seed(seed)
    frames = torch.rand(B, t, 3, 128, 128, generator=g) * 2 - 1
    actions = torch.rand(B, t, 4, generator=g) * 2 - 1
    noise = torch.rand(E.mpc_noise_floats(B, t, R, TH, 2), generator=g)
    return frames, actions, noise


def _generator_rollout(s):
    """The closed-loop rollout of one planning step with s horizon steps: the state's code broadcast at ts = 0."""
    calls = [("encode", B), ("g_input", B, R, B, R, BR), ("generate", BR), ("forward", BR)]
    return calls + [("encode", BR), ("g_input", BR, 1, B, R, BR), ("generate", BR), ("forward", BR)] * (s - 1)


def _planning_step(s, iterations=0, proposal="generator", last=("score_select", B, R, True, True, False)):
    calls = _generator_rollout(s) if proposal == "generator" else [("forward", BR)] * s
    for it in range(iterations):
        calls += [("score_select", B, R, False, False, False), ("cem_update", s, B, R, it == 0)] + [("forward", BR)] * s
    return calls + [last]


def _mpc_plan_calls(t, **kw):
    calls = [("images", B * t), ("encode", B)]
    for i in range(t - 1):
        calls += _planning_step(min(TH, t - 1 - i), **kw) + [("mse", B)]
    return calls + [("mse", B)]


@pytest.fixture(scope="module")
def plain():
    models = C.RecordingModels()
    frames, actions, noise = _inputs()
    return E.mpc_plan(models, frames, actions, R, TH, noise=noise), models.calls


def test_mpc_plan_without_cem(plain):
    _, calls = plain
    assert calls == _mpc_plan_calls(T)
    assert len(calls) == 47


def test_zero_iterations_add_one_normal_draw_and_change_no_result(plain):
    res, calls = plain
    models = C.RecordingModels()
    frames, actions, noise = _inputs()
    with_cem = E.mpc_plan(models, frames, actions, R, TH, noise=noise, cem=E.CemSettings(iterations=0))
    assert [c for c in models.calls if c[0] == "normal"] == [("normal", 0)]
    assert [c for c in models.calls if c[0] != "normal"] == calls
    for key in res:
        assert torch.equal(res[key], with_cem[key]), key
    picked = res["rollout_errors"].gather(2, res["choices"].long().unsqueeze(2)).squeeze(2)
    assert torch.equal(with_cem["best_curve"][:, 0], picked) and torch.equal(with_cem["best_err"], picked)
    assert not with_cem["cem_mean"].any() and not with_cem["cem_std"].any()


def test_two_iterations_replay_the_population_open_loop():
    models = C.RecordingModels()
    frames, actions, noise = _inputs()
    normal = torch.randn(E.cem_normal_floats(B, R, TH, 2, seq_length=T), generator=torch.Generator().manual_seed(1))
    res = E.mpc_plan(models, frames, actions, R, TH, noise=noise, normal=normal, cem=E.CemSettings(iterations=2))
    assert models.calls == _mpc_plan_calls(T, iterations=2)
    assert res["best_curve"].shape == (T - 1, 3, B) and torch.isfinite(res["best_curve"]).all()
    # inside the iterations: no encode, g_input or generate
    step = _planning_step(TH, iterations=2)
    inside = step[len(_generator_rollout(TH)):]
    assert not {c[0] for c in inside} & {"encode", "g_input", "generate"}


def test_uniform_proposal_never_calls_the_generator():
    models = C.RecordingModels()
    frames, actions, noise = _inputs()
    cem = E.CemSettings(iterations=1, proposal="uniform")
    E.mpc_plan(models, frames, actions, R, TH, noise=noise, cem=cem, seed=3)
    calls = [c for c in models.calls if c[0] != "normal"]
    assert calls == _mpc_plan_calls(T, iterations=1, proposal="uniform")
    assert [c for c in models.calls if c[0] == "normal"] == [("normal", E.cem_normal_floats(B, R, TH, 1, seq_length=T))]
    assert calls.count(("encode", B)) == 1                            # the goal's; no state is encoded
    assert not {c[0] for c in calls} & {"g_input", "generate"}


def test_plan_step_without_cem():
    models = C.RecordingModels()
    frames, _, _ = _inputs(2)
    state, goal = frames[:, 0].contiguous(), frames[:, 1].contiguous()
    goal_code = models.encode(goal)
    del models.calls[:]
    noise = torch.rand(E.plan_step_noise_floats(B, R, TH, 2), generator=torch.Generator().manual_seed(2))
    out = E.plan_step(models, state, goal, goal_code, R, TH, noise=noise)
    assert models.calls == _planning_step(TH, last=("score_select", B, R, False, False, False))
    assert len(out) == 4 and out[3].shape == (B, R, 4)


def test_plan_step_is_mpc_plans_first_planning_step():
    t = TH + 1                                                        # the first planning step has the full horizon
    frames, actions, noise = _inputs(t, seed=5)
    models = C.RecordingModels()
    res = E.mpc_plan(models, frames, actions, R, TH, noise=noise)
    state, goal = frames[:, 0].contiguous(), frames[:, t - 1].contiguous()
    action, choice, errors, actions0 = E.plan_step(models, state, goal, models.encode(goal), R, TH,
                                                   noise=noise[:E.plan_step_noise_floats(B, R, TH, 2)])
    assert torch.equal(choice, res["choices"][0])
    assert torch.equal(errors, res["rollout_errors"][0])
    assert torch.equal(action, res["actions"][:, 0])
    assert torch.equal(action, actions0.gather(1, choice.long().view(B, 1, 1).expand(B, 1, 4)).view(B, 4))
