"""CPU tests of the host side of the planner's MPPI weighting and warm start (ndivplanning_amd/evaluation.py: the new
CemSettings fields and the `mpc.cem` keys, plan_normal_floats, plan_step's `prior`, mpc_plan's and MpcController's carried
fit), of the call sequence of a warm planning step read on the recording stand-in of tests/plan_warm_common.py, and of the
arguments ndp_plan_update and ndp_plan_warm refuse before they launch anything (the library loads without a GPU)."""
import pytest
import torch

import plan_common as C
import plan_warm_common as W
from ndivplanning_amd import evaluation as E
from ndivplanning_amd.utils.file import DotMap

B, T, R, TH, NZ = 2, 5, 8, 3, 2
BR = B * R


# ---------------------------------------------------------------------------------------------- the settings
def test_the_new_fields_default_to_off():
    s = E.CemSettings()
    assert (s.weighting, s.temperature, s.warm_start, s.warm_rows, s.warm_std) == ("elites", None, False, None, None)
    assert E.CemSettings.FIELDS[:7] == ("iterations", "elites", "momentum", "min_std", "proposal", "low", "high")
    assert E.CemSettings.FIELDS[7:] == ("weighting", "temperature", "warm_start", "warm_rows", "warm_std")
    for f in E.CemSettings.FIELDS:
        assert ("%s=" % f) in repr(s)


def test_accepted_settings():
    s = E.CemSettings(weighting="mppi", temperature=0.02, warm_start=True, warm_rows=3, warm_std=0.2)
    assert (s.weighting, s.temperature, s.warm_start, s.warm_rows, s.warm_std) == ("mppi", 0.02, True, 3, 0.2)
    assert s.warm_count(8) == 3 and s.carried_floor() == 0.2
    w = E.CemSettings(warm_start=True, min_std=0.125)
    assert [w.warm_count(r) for r in (2, 3, 4, 8, 32, 256)] == [1, 1, 1, 2, 8, 64]
    assert w.carried_floor() == 0.125                                 # None: min_std
    assert E.CemSettings(warm_start=True, warm_std=0).carried_floor() == 0.0
    assert E.CemSettings(warm_start=True, warm_rows=7).warm_count(8) == 7
    assert E.CemSettings(warm_start=True, iterations=1).warm_start


@pytest.mark.parametrize("kwargs", [
    {"weighting": "softmax"}, {"weighting": "mppi"}, {"weighting": "mppi", "temperature": 0.0},
    {"weighting": "mppi", "temperature": -1.0}, {"weighting": "mppi", "temperature": float("inf")},
    {"weighting": "mppi", "temperature": float("nan")}, {"weighting": "mppi", "temperature": 1e-60},
    {"weighting": "mppi", "temperature": 1e60}, {"temperature": 0.1}, {"weighting": "elites", "temperature": 0.1},
    {"warm_start": True, "iterations": 0}, {"warm_start": 1}, {"warm_rows": 2}, {"warm_std": 0.1},
    {"warm_start": True, "warm_rows": 0}, {"warm_start": True, "warm_rows": 256}, {"warm_start": True, "warm_rows": 1.5},
    {"warm_start": True, "warm_std": -0.1}, {"warm_start": True, "warm_std": float("inf")},
    {"warm_start": True, "warm_std": float("nan")}])
def test_refused_settings(kwargs):
    with pytest.raises(ValueError):
        E.CemSettings(**kwargs)


def test_warm_rows_are_checked_against_the_rollouts_where_elites_are():
    s = E.CemSettings(warm_start=True, warm_rows=8)
    with pytest.raises(ValueError):
        s.warm_count(8)                                               # W <= R - 1
    assert s.warm_count(9) == 8
    with pytest.raises(ValueError):
        E._cem_check(s, 8, 3)
    E._cem_check(s, 9, 3)
    E._cem_check(E.CemSettings(warm_rows=None), 8, 3)                 # without warm_start nothing more is checked
    with pytest.raises(ValueError):
        E.mpc_plan(W.RecordingWarmModels(), torch.zeros(1, 3, 3, 128, 128), torch.zeros(1, 3, 4), 8, 2, cem=s)
    with pytest.raises(ValueError):
        E.cem_from_config(DotMap({"mpc": {"rollouts": 4, "time_horizon": 2, "cem": {"warm_start": True, "warm_rows": 4}}}))


def test_from_config_reads_the_new_keys():
    s = E.CemSettings.from_config({"iterations": 2, "weighting": "mppi", "temperature": 0.05, "warm_start": True,
                                   "warm_rows": 2, "warm_std": 0.3})
    assert (s.iterations, s.weighting, s.temperature, s.warm_start, s.warm_rows, s.warm_std) == (2, "mppi", 0.05, True, 2, 0.3)
    with pytest.raises(ValueError, match="unknown keys"):
        E.CemSettings.from_config({"weighting": "mppi", "temperature": 0.05, "warm": True})
    with pytest.raises(ValueError):
        E.CemSettings.from_config({"weighting": "mppi"})
    cfg = DotMap({"mpc": {"rollouts": 8, "time_horizon": 3, "cem": {"weighting": "mppi", "temperature": 0.5,
                                                                  "warm_start": True}}})
    got = E.cem_from_config(cfg)
    assert got.weighting == "mppi" and got.warm_start and got.warm_count(8) == 2


# ---------------------------------------------------------------------------------------------- the normal draws
def test_plan_normal_floats_against_a_count_by_hand():
    cold = E.CemSettings(iterations=2)
    warm = E.CemSettings(iterations=2, warm_start=True, warm_rows=3)
    # one plan_step: 2 iterations of [Th,B,R,4], and with a prior [Th,B,W,4] ahead of them
    assert E.plan_normal_floats(2, 8, 3, cold) == 2 * 3 * 2 * 8 * 4 == 384
    assert E.plan_normal_floats(2, 8, 3, warm) == 384
    assert E.plan_normal_floats(2, 8, 3, warm, prior=True) == 384 + 3 * 2 * 3 * 4 == 456
    # one mpc_plan on T = 5 frames, Th = 3: horizons 3, 3, 2, 1; every step but the first has a prior
    assert E.plan_normal_floats(2, 8, 3, cold, seq_length=5) == 2 * (3 + 3 + 2 + 1) * 2 * 8 * 4 == 1152
    assert E.plan_normal_floats(2, 8, 3, warm, seq_length=5) == 1152 + (3 + 2 + 1) * 2 * 3 * 4 == 1296
    assert E.plan_normal_floats(2, 8, 3, E.CemSettings(iterations=1, warm_start=True), seq_length=2) == 3 * 0 + 1 * 2 * 8 * 4
    assert E.plan_normal_floats(1, 32, 5, E.CemSettings(iterations=3, warm_start=True), prior=True) == 3 * 5 * 32 * 4 + 5 * 8 * 4
    assert E.plan_normal_floats(1, 4, 2, E.CemSettings(iterations=0)) == 0


def test_cem_normal_floats_is_unchanged():
    assert E.cem_normal_floats(2, 8, 3, 2) == 384
    assert E.cem_normal_floats(2, 8, 3, 2, seq_length=5) == 1152
    assert E.cem_normal_floats(1, 6, 2, 2) == 96 and E.cem_normal_floats(3, 5, 4, 0, seq_length=9) == 0
    for b, r, th, i, t in ((1, 2, 1, 1, 2), (3, 5, 3, 2, 4), (2, 32, 5, 3, 7)):
        s = E.CemSettings(iterations=i)
        assert E.plan_normal_floats(b, r, th, s) == E.cem_normal_floats(b, r, th, i)
        assert E.plan_normal_floats(b, r, th, s, seq_length=t) == E.cem_normal_floats(b, r, th, i, seq_length=t)


# ---------------------------------------------------------------------------------------------- the planner's calls
def _step_inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    state = torch.rand(B, 3, 128, 128, generator=g) * 2 - 1
    goal = torch.rand(B, 3, 128, 128, generator=g) * 2 - 1
    noise = torch.rand(E.plan_step_noise_floats(B, R, TH, NZ), generator=g)
    return state, goal, noise, g


def _generator_rollout(s):
    calls = [("encode", B), ("g_input", B, R, B, R, BR), ("generate", BR), ("forward", BR)]
    return calls + [("encode", BR), ("g_input", BR, 1, B, R, BR), ("generate", BR), ("forward", BR)] * (s - 1)


def _warm_step(models, cem, prior, seed=0, **kw):
    state, goal, noise, g = _step_inputs(seed)
    normal = torch.randn(E.plan_normal_floats(B, R, TH, cem, prior=prior is not None), generator=g)
    goal_code = models.encode(goal)
    del models.calls[:]
    return E.plan_step(models, state, goal, goal_code, R, TH, noise=noise, normal=normal, cem=cem, prior=prior, **kw)


def _prior(steps_prev=TH, seed=5):
    g = torch.Generator().manual_seed(seed)
    return 0.3 * torch.randn(B, steps_prev, 4, generator=g), 0.02 + 0.2 * torch.rand(B, steps_prev, 4, generator=g)


@pytest.mark.parametrize("weighting", ["elites", "mppi"])
def test_call_order_of_a_warm_planning_step(weighting):
    """The warm launch once, ahead of the rollout; the generator's rollout as ever; every update through plan_update, the
    first with smooth = 1, first = 1, the later ones with smooth = 1, first = 0; and at every horizon step the forward
    model saw warm[ts] in rows R - W .. R - 1 and the generator's own actions below them: the injection lies after the
    generator call and before the forward call."""
    cem = E.CemSettings(iterations=2, warm_start=True, warm_rows=3, weighting=weighting,
                        temperature=0.05 if weighting == "mppi" else None)
    models = W.RecordingWarmModels()
    prior = _prior()
    res = _warm_step(models, cem, prior)
    want = [("plan_warm", TH, B, 3, TH)] + _generator_rollout(TH)
    for it in range(2):
        want += [("score_select", B, R, False, False, False), ("plan_update", TH, B, R, True, it == 0)] + [("forward", BR)] * TH
    want += [("score_select", B, R, False, False, False)]
    assert models.calls == want
    cold = W.RecordingWarmModels()
    _warm_step(cold, E.CemSettings(iterations=2, weighting=weighting, temperature=cem.temperature), None)
    assert [c[0] for c in cold.calls].count("plan_warm") == 0
    for ts in range(TH):
        seen, plain = models.forward_actions[ts].view(B, R, 4), cold.forward_actions[ts].view(B, R, 4)
        assert torch.equal(seen[:, R - 3:], models.warm[ts]), ts
        assert torch.equal(seen[:, :R - 3], plain[:, :R - 3]), ts
        assert not torch.equal(seen[:, R - 3:], plain[:, R - 3:])
    # row 0 of the injected rows is the shifted mean, clamped; the shift is by one action, the last one repeated
    src = [1, 2, 2]
    assert torch.equal(models.warm[:, :, 0], prior[0][:, src].clamp(-1, 1).transpose(0, 1))
    info = res[4]
    assert info["cem_mean"].shape == (B, TH, 4) and (info["cem_std"] >= cem.min_std).all()


def test_updates_without_a_prior():
    """Without a prior the first update starts afresh (smooth = 0, first = 1); the elites' weighting without a prior is
    the existing call, cem_update."""
    mppi = E.CemSettings(iterations=2, weighting="mppi", temperature=0.05, warm_start=True)
    models = W.RecordingWarmModels()
    _warm_step(models, mppi, None)
    assert [c for c in models.calls if c[0] in ("plan_update", "cem_update", "plan_warm")] == \
        [("plan_update", TH, B, R, False, True), ("plan_update", TH, B, R, True, False)]
    models = W.RecordingWarmModels()
    _warm_step(models, E.CemSettings(iterations=2, warm_start=True), None)
    assert [c for c in models.calls if c[0] in ("plan_update", "cem_update", "plan_warm")] == \
        [("cem_update", TH, B, R, True), ("cem_update", TH, B, R, False)]


def test_the_default_settings_make_the_calls_of_the_planner_as_it_was():
    a, b = C.RecordingModels(), C.RecordingModels()
    state, goal, noise, g = _step_inputs()
    normal = torch.randn(E.cem_normal_floats(B, R, TH, 2), generator=g)
    cem = E.CemSettings(iterations=2)
    one = E.plan_step(a, state, goal, a.encode(goal), R, TH, noise=noise, normal=normal, cem=cem)
    assert [c for c in a.calls if c[0] == "cem_update"] == [("cem_update", TH, B, R, True), ("cem_update", TH, B, R, False)]
    other = E.plan_step(b, state, goal, b.encode(goal), R, TH, noise=noise, normal=normal, cem=cem, prior=None)
    assert a.calls == b.calls
    for x, y in zip(one[:4], other[:4]):
        assert torch.equal(x, y)


def test_uniform_proposal_receives_the_injected_rows_too():
    cem = E.CemSettings(iterations=1, warm_start=True, proposal="uniform")
    models = W.RecordingWarmModels()
    _warm_step(models, cem, _prior())
    assert [c[0] for c in models.calls][:TH + 1] == ["plan_warm"] + ["forward"] * TH
    for ts in range(TH):
        assert torch.equal(models.forward_actions[ts].view(B, R, 4)[:, R - 2:], models.warm[ts])


def test_prior_is_validated():
    models = W.RecordingWarmModels()
    with pytest.raises(ValueError, match="warm_start"):
        _warm_step(models, E.CemSettings(iterations=2), _prior())
    state, goal, noise, _ = _step_inputs()
    with pytest.raises(ValueError, match="warm_start"):
        E.plan_step(models, state, goal, models.encode(goal), R, TH, noise=noise, prior=_prior())
    warm = E.CemSettings(iterations=1, warm_start=True)
    for bad in (_prior(TH - 1), (_prior()[0], _prior(TH + 1)[1]), (_prior()[0][:1], _prior()[1][:1]), _prior(33)):
        with pytest.raises(ValueError, match="prior"):
            _warm_step(models, warm, bad)
    _warm_step(models, warm, _prior(TH + 2))                          # a longer previous horizon is fine: steps <= steps_prev
    assert models.calls[0] == ("plan_warm", TH, B, 2, TH + 2)
    with pytest.raises(ValueError, match="normal"):                   # the cold count does not fit a warm step
        state, goal, noise, g = _step_inputs()
        E.plan_step(models, state, goal, models.encode(goal), R, TH, noise=noise, cem=warm, prior=_prior(),
                    normal=torch.zeros(E.plan_normal_floats(B, R, TH, warm)))


def test_mpc_plan_carries_the_fit_from_step_to_step():
    """T = 5, Th = 3: horizons 3, 3, 2, 1.  The first planning step is cold; every later one shifts the fit of the step
    before it, also onto the shorter horizon (steps = steps_prev - 1)."""
    g = torch.Generator().manual_seed(1)
    frames = torch.rand(B, T, 3, 128, 128, generator=g) * 2 - 1
    actions = torch.rand(B, T, 4, generator=g) * 2 - 1
    noise = torch.rand(E.mpc_noise_floats(B, T, R, TH, NZ), generator=g)
    cem = E.CemSettings(iterations=1, warm_start=True, weighting="mppi", temperature=0.1)
    normal = torch.randn(E.plan_normal_floats(B, R, TH, cem, seq_length=T), generator=g)
    models = W.RecordingWarmModels()
    res = E.mpc_plan(models, frames, actions, R, TH, noise=noise, normal=normal, cem=cem)
    assert [c for c in models.calls if c[0] in ("plan_warm", "plan_update")] == [
        ("plan_update", 3, B, R, False, True),
        ("plan_warm", 3, B, 2, 3), ("plan_update", 3, B, R, True, True),
        ("plan_warm", 2, B, 2, 3), ("plan_update", 2, B, R, True, True),
        ("plan_warm", 1, B, 2, 2), ("plan_update", 1, B, R, True, True)]
    assert res["cem_mean"].shape == (B, 1, 4) and res["best_curve"].shape == (T - 1, 2, B)
    for bad in (normal[:-1], torch.cat([normal, normal[:1]])):
        with pytest.raises(ValueError):
            E.mpc_plan(W.RecordingWarmModels(), frames, actions, R, TH, noise=noise, normal=bad, cem=cem)
    # the first planning step is plan_step's (T - 1 >= Th); the whole loop is replayed on the GPU (test_gpu_plan_warm.py)
    again = W.RecordingWarmModels()
    goal = frames[:, T - 1].contiguous()
    step = E.plan_step(again, frames[:, 0].contiguous(), goal, again.encode(goal), R, TH,
                       noise=noise[:E.plan_step_noise_floats(B, R, TH, NZ)], normal=normal[:E.plan_normal_floats(B, R, TH, cem)],
                       cem=cem)
    assert torch.equal(step[1], res["choices"][0]) and torch.equal(step[2], res["rollout_errors"][0])


def test_controller_reset_drops_the_prior():
    """MpcController's constructor needs a GPU (its resizer, its event); reset() and the carried state do not."""
    ctrl = E.MpcController.__new__(E.MpcController)
    ctrl.models, ctrl.frame_shape, ctrl._staging = W.RecordingWarmModels(), None, None
    ctrl._actions = torch.empty(B, 4)
    ctrl._prior, ctrl._normal_off, ctrl.steps = _prior(), 456, 3
    ctrl.reset(torch.zeros(B, 3, 128, 128))
    assert ctrl._prior is None and ctrl._normal_off == 0 and ctrl.steps == 0


# ---------------------------------------------------------------------------------------------- refused arguments
@pytest.fixture(scope="module")
def lib():
    from ndivplanning_amd import _build, _capi
    _build.build()
    return _capi.load()


@pytest.mark.parametrize("over", W.REFUSED_UPDATE, ids=lambda o: "-".join("%s=%s" % kv for kv in o.items()))
def test_plan_update_refuses(lib, over):
    assert W.refused_update(lib, **over) == 1                         # NDP_E_ARG, nothing launched
    assert b"ndp_plan_update" in lib.ndp_last_error()


@pytest.mark.parametrize("over", W.REFUSED_WARM, ids=lambda o: "-".join("%s=%s" % kv for kv in o.items()))
def test_plan_warm_refuses(lib, over):
    assert W.refused_warm(lib, **over) == 1
    assert b"ndp_plan_warm" in lib.ndp_last_error()


def test_the_old_entry_point_still_names_itself(lib):
    assert C.refused_call(lib, first=2) == 1
    assert b"ndp_plan_cem_update" in lib.ndp_last_error()
