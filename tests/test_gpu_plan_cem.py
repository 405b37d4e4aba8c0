"""GPU tests of the planner's cross-entropy refinement: ndp_plan_cem_update and ndp_normal_noise (csrc/ndp_plan.inc)
against the numpy restatements of tests/plan_common.py, and mpc_plan / plan_step / MpcController / the mpc_eval drop-in
with `cem` (ndivplanning_amd/evaluation.py).  The shapes are test_gpu_eval.py's tiny ones."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import plan_common as C
from fake_push_env import FakePushEnv
from test_gpu_eval import _modules, _mpc_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _lib():
    from ndivplanning_amd import _build, _capi
    _build.build()
    return _capi.load()


# ------------------------------------------------------------------------------- the kernel on the host driver's cases
def _run_update(lib, c):
    from ndivplanning_amd import _capi
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(DEV) for k in ("err", "seq_in", "normal", "mean", "std", "best_err")}
    th, b, r, _ = c["seq_in"].shape
    seq_out = torch.full_like(t["seq_in"], -7.0)
    idx = torch.full((b, c["elites"]), -7, dtype=torch.int32, device=DEV) if c["with_idx"] else None
    low, high = (_capi.c_float * 4)(*c["low"]), (_capi.c_float * 4)(*c["high"])
    _capi.check(lib.ndp_plan_cem_update(_capi.ptr(t["err"]), _capi.ptr(t["seq_in"]), _capi.ptr(t["normal"]), b, r, th,
                                        c["elites"], c["first"], c["momentum"], c["min_std"], low, high, _capi.ptr(t["mean"]),
                                        _capi.ptr(t["std"]), _capi.ptr(seq_out), _capi.ptr(t["best_err"]), _capi.ptr(idx),
                                        _capi.stream_ptr()), "ndp_plan_cem_update")
    got = {"mean": t["mean"], "std": t["std"], "seq_out": seq_out, "best_err": t["best_err"]}
    if idx is not None:
        got["elite_idx"] = idx
    return {k: v.cpu().numpy() for k, v in got.items()}


def _within_one_ulp(got, want):
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(invalid="ignore"):
        near = np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))
    return bool((same | near).all())


def test_update_against_the_restatement_on_the_host_drivers_cases():
    """elite_idx, mean and best_err bit-equal; std and seq_out within 1 fp32 ulp (the device's fp64 sqrt is the only
    operation that could differ), with the count of cases where they too are bit-equal printed."""
    lib = _lib()
    exact = total = 0
    for c in C.cases():
        got, want = _run_update(lib, c), C.cem_update(c)
        again = _run_update(lib, c)
        for o in got:
            assert C.bits_equal(got[o], again[o]), (c["name"], o, "two calls differ")
        for o in ("elite_idx", "mean", "best_err"):
            if o in got:
                assert C.bits_equal(got[o], want[o]), (c["name"], o)
        for o in ("std", "seq_out"):
            assert _within_one_ulp(got[o], want[o]), (c["name"], o)
            total += 1
            exact += C.bits_equal(got[o], want[o])
        if c["with_idx"]:
            C.check_special(c, got)
    print("std / seq_out bit-equal to the restatement in %d of %d comparisons" % (exact, total))


@pytest.mark.parametrize("over", C.REFUSED, ids=lambda o: "-".join("%s=%s" % kv for kv in o.items()))
def test_refused_arguments(over):
    lib = _lib()
    assert C.refused_call(lib, **over) == 1                           # NDP_E_ARG, nothing launched


# ------------------------------------------------------------------------------- the normal draws
def _draw(lib, fn, n, seed, offset=None):
    from ndivplanning_amd import _capi
    out = torch.empty(n, dtype=torch.float32, device=DEV)
    off = None if offset is None else torch.tensor([offset], dtype=torch.int32, device=DEV)
    _capi.check(getattr(lib, fn)(_capi.ptr(out), n, seed, _capi.ptr(off), _capi.stream_ptr()), fn)
    return out.cpu().numpy()


def test_normal_noise_against_box_muller_on_the_same_uniforms():
    """|device - fp64 restatement| <= 1e-5: r <= sqrt(-2 ln 2^-32) < 6.7, the angle 2 pi u2 is rounded to fp32 (<= 2^-22
    relative of 6.28) and logf, sqrtf, cosf, sinf add a few ulp: about 6.7e-6.  Measured on an MI355X: see DESIGN 5p.
    "The same uniforms" are the DEVICE's own here (ndp_uniform_noise with the same seed and offset): this test holds the
    Box-Muller arithmetic, not the stream.  tests/test_gpu_noise.py holds the stream to the host restatement and the
    normals to the Box-Muller of the restatement's uniforms."""
    lib = _lib()
    n, seed = 1 << 20, 0x5EED1234
    for offset in (None, 3):
        z = _draw(lib, "ndp_normal_noise", n, seed, offset)
        u = _draw(lib, "ndp_uniform_noise", n, seed, offset)
        want = C.box_muller(u)
        worst = np.abs(z.astype(np.float64) - want).max()
        print("offset %s: max |device - fp64| = %.3g, mean %.3g, var - 1 %.3g" % (offset, worst, z.mean(dtype=np.float64),
                                                                                z.var(dtype=np.float64) - 1))
        assert np.isfinite(z).all()
        assert worst <= 1e-5
        assert abs(z.mean(dtype=np.float64)) < 5 / 1024
        assert abs(z.var(dtype=np.float64) - 1) < 5 * np.sqrt(2 / n)
        assert C.bits_equal(z, _draw(lib, "ndp_normal_noise", n, seed, offset))          # the same seed, the same bits
    odd = _draw(lib, "ndp_normal_noise", 1001, seed, 3)               # an odd n drops the last sine
    assert C.bits_equal(odd, z[:1001])
    assert C.bits_equal(_draw(lib, "ndp_normal_noise", 3, seed, 3), z[:3])
    assert not np.array_equal(_draw(lib, "ndp_normal_noise", 1024, seed + 1, 3), z[:1024])


def test_models_normal_is_the_offset_one_stream():
    from ndivplanning_amd import evaluation as E
    models = E.EvalModels(*_modules(), DEV)
    lib = _lib()
    z = models.normal(4096, 77).cpu().numpy()
    assert C.bits_equal(z, _draw(lib, "ndp_normal_noise", 4096, 77, 1))
    assert not np.array_equal(z, _draw(lib, "ndp_normal_noise", 4096, 77, None))


# ------------------------------------------------------------------------------- the planner
@pytest.fixture(scope="module")
def models():
    from ndivplanning_amd import evaluation as E
    return E.EvalModels(*_modules(), DEV)


def _plan_step_inputs(models, b):
    frames, _ = _mpc_inputs(b, 2)
    state, goal = frames[:, 0].contiguous(), frames[:, 1].contiguous()
    return state, goal, models.encode(goal)


def test_zero_iterations_give_the_bits_of_the_planner_without_cem(models):
    """The plain planner, the planner with 0 iterations, and the restatement by hand on EvalModels' calls (_replay, which
    does not go through the planner) agree bit for bit."""
    from ndivplanning_amd import evaluation as E
    b, t, r, th, nz = 2, 5, 5, 3, 2
    frames, actions = _mpc_inputs(b, t)
    off = E.CemSettings(iterations=0)
    noise = torch.rand(E.mpc_noise_floats(b, t, r, th, nz), generator=torch.Generator().manual_seed(4)).to(DEV)
    for kw in ({"noise": noise}, {"seed": 11}):
        plain = E.mpc_plan(models, frames, actions, r, th, **kw)
        with_cem = E.mpc_plan(models, frames, actions, r, th, cem=off, **kw)
        for key in plain:
            assert torch.equal(plain[key], with_cem[key]), key
        assert with_cem["best_curve"].shape == (t - 1, 1, b)
        picked = plain["rollout_errors"].gather(2, plain["choices"].long().unsqueeze(2)).squeeze(2)
        assert torch.equal(with_cem["best_curve"][:, 0], picked) and torch.equal(with_cem["best_err"], picked)
        drawn = kw["noise"] if "noise" in kw else models.uniform(noise.numel(), kw["seed"])
        by_hand = _replay(models, off, frames, r, th, drawn, None)
        for key in ("choices", "actions", "rollout_errors"):
            assert torch.equal(plain[key], by_hand[key]), key
    state, goal, goal_code = _plan_step_inputs(models, b)
    step_noise = noise[:E.plan_step_noise_floats(b, r, th, nz)]
    for kw in ({"noise": step_noise}, {"seed": 12}):
        plain = E.plan_step(models, state, goal, goal_code, r, th, **kw)
        with_cem = E.plan_step(models, state, goal, goal_code, r, th, cem=off, **kw)
        assert len(plain) == 4 and len(with_cem) == 5
        for x, y in zip(plain, with_cem):
            assert torch.equal(x, y)


def test_plan_step_is_mpc_plans_first_planning_step(models):
    """T = Th + 1: mpc_plan's first planning step has the full horizon, and plan_step on (frame 0, last frame) with the
    same noise runs the same kernels on the same inputs."""
    from ndivplanning_amd import evaluation as E
    b, t, r, th, nz = 2, 4, 5, 3, 2
    frames, actions = _mpc_inputs(b, t)
    noise = torch.rand(E.mpc_noise_floats(b, t, r, th, nz), generator=torch.Generator().manual_seed(8)).to(DEV)
    res = E.mpc_plan(models, frames, actions, r, th, noise=noise)
    state, goal = frames[:, 0].contiguous(), frames[:, t - 1].contiguous()
    action, choice, errors, actions0 = E.plan_step(models, state, goal, models.encode(goal), r, th,
                                                   noise=noise[:E.plan_step_noise_floats(b, r, th, nz)])
    assert torch.equal(choice, res["choices"][0])
    assert torch.equal(errors, res["rollout_errors"][0])
    assert torch.equal(action, res["actions"][:, 0])
    assert actions0.shape == (b, r, 4)
    assert torch.equal(action, actions0.gather(1, choice.long().view(b, 1, 1).expand(b, 1, 4)).view(b, 4))


def _replay(models, cem, frames, r, th, noise, normal):
    """mpc_plan with `cem` restated on EvalModels' calls and ndp_plan_cem_update.  Returns what mpc_plan returns under
    the same keys (rollout_errors: the err of each planning step's last selection), plus `best_trace` [T-1][I][B]
    (best_err after every update) and `row0` [(before, after)]: the rank-0 error and the error of row 0 of the next
    population, the same sequence re-evaluated."""
    from ndivplanning_amd import evaluation as E
    b, t = int(frames.shape[0]), int(frames.shape[1])
    t1, nz, br, its = t - 1, models.noise_dim, b * r, cem.iterations
    per = frames.reshape(b, t, E.IMAGE_VALUES)
    goal = per[:, t1].contiguous().view(b, 3, 128, 128)
    goal_code = models.encode(goal)
    state = per[:, 0].contiguous().view(b, 3, 128, 128)
    choices, actions, errors, curve, trace, row0 = [], [], [], [], [], []
    off = n_off = 0
    for image_num in range(t1):
        steps = min(th, t1 - image_num)
        rep = state.view(b, 1, -1).expand(b, r, -1).reshape(br, 3, 128, 128).contiguous()
        seq = torch.empty(steps, b, r, 4, device=DEV)
        pred = rep
        for ts in range(steps):
            code_in = models.g_input(models.encode(state if ts == 0 else pred), r if ts == 0 else 1, goal_code, r, br)
            act = models.generate(code_in, noise[off:off + br * nz])
            off += br * nz
            seq[ts] = act.view(b, r, 4)
            pred = models.forward(pred, act)
            if ts == 0:
                pred0 = pred
        mean, std = torch.zeros(b, steps, 4, device=DEV), torch.zeros(b, steps, 4, device=DEV)
        best = torch.empty(b, device=DEV)
        step_curve, step_trace = [], []
        err, pick = torch.empty(b, r, device=DEV), torch.empty(b, dtype=torch.int32, device=DEV)
        act_out, nxt = torch.empty(b, 4, device=DEV), torch.empty(b, 3, 128, 128, device=DEV)
        for it in range(its):
            models.score_select(pred, b, r, goal, seq[0].contiguous(), pred0, None, err, pick, act_out, nxt)
            rank0 = err.gather(1, pick.long().view(b, 1)).view(b).clone()
            step_curve.append(rank0)
            new = torch.empty_like(seq)
            n = steps * br * 4
            models.cem_update(err, seq, normal[n_off:n_off + n], cem, it == 0, mean, std, new, best)
            n_off += n
            step_trace.append(best.clone())
            seq = new
            pred = rep
            for ts in range(steps):
                pred = models.forward(pred, seq[ts].reshape(br, 4))
                if ts == 0:
                    pred0 = pred
            models.score_select(pred, b, r, goal, seq[0].contiguous(), pred0, None, err, pick, act_out, nxt)
            row0.append((rank0, err[:, 0].clone()))
        models.score_select(pred, b, r, goal, seq[0].contiguous(), pred0, None, err, pick, act_out, nxt)
        step_curve.append(err.gather(1, pick.long().view(b, 1)).view(b).clone())
        choices.append(pick.clone())
        errors.append(err.clone())
        actions.append(act_out.clone())
        curve.append(torch.stack(step_curve))
        trace.append(step_trace)
        state = nxt
    return {"choices": torch.stack(choices), "actions": torch.stack(actions).transpose(0, 1).contiguous(),
            "rollout_errors": torch.stack(errors), "best_curve": torch.stack(curve), "cem_mean": mean, "cem_std": std,
            "best_trace": trace, "row0": row0}


@pytest.fixture(scope="module")
def driven(models):
    """mpc_plan with two iterations on given noise and normals, and the same planner driven by hand."""
    from ndivplanning_amd import evaluation as E
    b, t, r, th, nz = 2, 5, 8, 3, 2
    cem = E.CemSettings(iterations=2)
    frames, actions = _mpc_inputs(b, t)
    g = torch.Generator().manual_seed(21)
    noise = torch.rand(E.mpc_noise_floats(b, t, r, th, nz), generator=g).to(DEV)
    normal = torch.randn(E.cem_normal_floats(b, r, th, cem.iterations, seq_length=t), generator=g).to(DEV)
    res = E.mpc_plan(models, frames, actions, r, th, noise=noise, normal=normal, cem=cem)
    return res, _replay(models, cem, frames, r, th, noise, normal), (b, t, r, th, cem)


def test_mpc_plan_equals_the_planner_driven_by_hand(driven):
    res, want, (b, t, r, th, cem) = driven
    assert res["best_curve"].shape == (t - 1, cem.iterations + 1, b)
    for key in ("choices", "actions", "best_curve", "cem_mean", "cem_std"):
        assert torch.equal(res[key], want[key]), key
    assert want["cem_mean"].shape == (b, 1, 4)                        # the last planning step's horizon is 1
    assert (res["cem_std"] >= cem.min_std).all()


def test_the_refinement_never_loses_its_best_sequence(driven):
    """best_err is non-increasing, exactly; the chosen row's error may rise by the 1e-4 relative allowance
    test_gpu_eval.py gives a row evaluated at a different position in the batch (row 0 is the previous winner)."""
    res, want, (b, t, r, th, cem) = driven
    for step in want["best_trace"]:
        for before, after in zip(step, step[1:]):
            assert (after <= before).all()
    curve = res["best_curve"]
    assert (curve[:, 1:] <= curve[:, :-1] * (1 + 1e-4)).all(), curve
    assert torch.equal(res["best_err"], curve.min(dim=1).values)
    same = sum(int(torch.equal(before, after)) for before, after in want["row0"])
    print("row 0 re-evaluated: bit-equal to the previous winner's error in %d of %d populations" % (same, len(want["row0"])))
    for before, after in want["row0"]:
        assert torch.allclose(after, before, rtol=1e-4, atol=0)


def test_uniform_proposal_lies_in_the_bounds_and_reads_the_same_noise(models):
    from ndivplanning_amd import evaluation as E
    b, t, r, th, nz = 2, 4, 6, 3, 2
    cem = E.CemSettings(iterations=0, proposal="uniform", low=[-0.5, -1.0, 0.25, -0.125], high=[0.5, -0.75, 0.25, 0.875])
    state, goal, goal_code = _plan_step_inputs(models, b)
    noise = torch.rand(E.plan_step_noise_floats(b, r, th, nz), generator=torch.Generator().manual_seed(6)).to(DEV)
    action, pick, err, actions0, info = E.plan_step(models, state, goal, goal_code, r, th, noise=noise, cem=cem)
    low, high = torch.tensor(cem.low, device=DEV), torch.tensor(cem.high, device=DEV)
    assert (actions0 >= low).all() and (actions0 <= high).all()
    u = noise[:b * r * nz].view(b, r, nz)                             # component c reads float c % nz of its row
    want = low + (high - low) * torch.cat([u, u], dim=2)
    assert torch.allclose(actions0, want, rtol=0, atol=1e-6)
    assert len(torch.unique(actions0[..., 0])) == b * r               # R different proposals per trajectory
    assert torch.equal(action, actions0.gather(1, pick.long().view(b, 1, 1).expand(b, 1, 4)).view(b, 4))
    frames, actions = _mpc_inputs(b, t)
    need = E.mpc_noise_floats(b, t, r, th, nz)
    stream = torch.rand(need + 1, generator=torch.Generator().manual_seed(7)).to(DEV)
    refine = E.CemSettings(iterations=1, proposal="uniform")
    res = E.mpc_plan(models, frames, actions, r, th, noise=stream[:need], cem=refine, seed=2)
    assert torch.isfinite(res["actions"]).all() and (res["actions"].abs() <= 1).all()
    for bad in (stream, stream[:need - 1]):
        with pytest.raises(ValueError):
            E.mpc_plan(models, frames, actions, r, th, noise=bad, cem=refine, seed=2)
    # the stream's last float is the last row's draw at the last planning step: all of it is read
    flat = E.CemSettings(iterations=0, proposal="uniform")
    changed = stream[:need].clone()
    changed[-1] = 1 - changed[-1]
    one, other = (E.mpc_plan(models, frames, actions, r, th, noise=n, cem=flat) for n in (stream[:need], changed))
    assert torch.equal(one["rollout_errors"][:-1], other["rollout_errors"][:-1])
    assert torch.equal(one["rollout_errors"][-1].view(-1)[:-1], other["rollout_errors"][-1].view(-1)[:-1])
    assert one["rollout_errors"][-1, -1, -1] != other["rollout_errors"][-1, -1, -1]
    with pytest.raises(ValueError):
        E.mpc_plan(models, frames, actions, r, th, noise=stream[:need], cem=refine, normal=torch.zeros(5))


def test_batched_plan_equals_single_trajectories(models):
    from ndivplanning_amd import evaluation as E
    b, t, r, th, nz = 3, 5, 6, 3, 2
    cem = E.CemSettings(iterations=2)
    frames, actions = _mpc_inputs(b, t)
    horizon = [min(th, t - 1 - i) for i in range(t - 1)]
    per_noise = [torch.rand(E.mpc_noise_floats(1, t, r, th, nz), generator=torch.Generator().manual_seed(50 + i))
                 for i in range(b)]
    per_normal = [torch.randn(E.cem_normal_floats(1, r, th, 2, seq_length=t), generator=torch.Generator().manual_seed(70 + i))
                  for i in range(b)]
    batched = torch.stack([p.view(sum(horizon), r * nz) for p in per_noise], dim=1).reshape(-1).to(DEV)
    pieces, off = [], 0
    for steps in horizon:                                             # [planning step][iteration][steps, B, R, 4]
        for _ in range(cem.iterations):
            n = steps * r * 4
            pieces.append(torch.stack([p[off:off + n].view(steps, r, 4) for p in per_normal], dim=1).reshape(-1))
            off += n
    normal = torch.cat(pieces).to(DEV)
    res = E.mpc_plan(models, frames, actions, r, th, noise=batched, normal=normal, cem=cem)
    again = E.mpc_plan(models, frames, actions, r, th, noise=batched, normal=normal, cem=cem)
    for key in res:
        assert torch.equal(res[key], again[key]), key                 # bit-reproducible
    for i in range(b):
        one = E.mpc_plan(models, frames[i:i + 1], actions[i:i + 1], r, th, noise=per_noise[i].to(DEV),
                         normal=per_normal[i].to(DEV), cem=cem)
        assert torch.equal(one["choices"][:, 0], res["choices"][:, i])
        assert torch.allclose(one["actions"][0], res["actions"][i], rtol=1e-5, atol=1e-6)
        assert torch.allclose(one["image_errors"][:, 0], res["image_errors"][:, i], rtol=1e-4, atol=1e-7)
        assert torch.allclose(one["rollout_errors"][:, 0], res["rollout_errors"][:, i], rtol=1e-4, atol=1e-7)
        assert torch.allclose(one["best_curve"][:, :, 0], res["best_curve"][:, :, i], rtol=1e-4, atol=1e-7)


def test_no_host_synchronisation_with_cem(models):
    from ndivplanning_amd import evaluation as E
    frames, actions = _mpc_inputs(2, 4)
    state, goal, goal_code = _plan_step_inputs(models, 2)
    for cem in (E.CemSettings(iterations=2), E.CemSettings(iterations=1, proposal="uniform")):
        E.mpc_plan(models, frames, actions, 4, 2, cem=cem)            # workspaces allocated outside the checked calls
        E.plan_step(models, state, goal, goal_code, 4, 2, cem=cem)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            res = E.mpc_plan(models, frames, actions, 4, 2, cem=cem, seed=3)
            step = E.plan_step(models, state, goal, goal_code, 4, 2, cem=cem, seed=3)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        assert res["best_curve"].shape == (3, cem.iterations + 1, 2) and step[4]["best_curve"].shape == (cem.iterations + 1, 2)
        assert torch.isfinite(res["best_curve"]).all() and torch.isfinite(step[0]).all()


def test_controller_with_cem_on_the_fake_environment(models):
    from ndivplanning_amd import evaluation as E
    env = FakePushEnv()
    goal = torch.from_numpy(np.pad(env.draw()[:, 16:144], ((4, 4), (0, 0), (0, 0))))[None]   # 128 x 128 of the scene
    cem = E.CemSettings(iterations=2, low=-0.5, high=[0.5, 0.5, 0.25, 0.5])
    ctrl = E.MpcController(models, 6, 2, seed=5, cem=cem)
    ctrl.reset(goal)
    low, high = np.float32(cem.low), np.float32(cem.high)
    for _ in range(2):
        actions, info = ctrl.act(env.render(mode="rgb_array")[None])
        assert actions.shape == (1, 4) and torch.isfinite(actions).all()
        assert (actions.numpy() >= low).all() and (actions.numpy() <= high).all()
        assert info["best_curve"].shape == (3, 1) and info["cem_mean"].shape == (1, 2, 4)
        assert torch.equal(info["action"].cpu(), actions)
        env.step(actions.numpy().ravel())
    given = E.MpcController(models, 6, 2, cem=cem, normal=torch.zeros(2 * E.cem_normal_floats(1, 6, 2, 2)))
    given.reset(goal)
    _, info = given.act(env.render(mode="rgb_array")[None])
    # normal draws of 0: every resampled row is the clamped mean, row 0 the previous winner
    rows = info["actions0"][0, 1:]
    assert torch.equal(rows, rows[0:1].expand_as(rows))


def test_gym_dropin_reads_the_cem_mapping():
    """MPC_gym_eval on the fake environment with `mpc.cem`: the four results are finite, the actions the environment
    received lie inside the mapping's bounds, and they are not those of the planner without the mapping."""
    import MPC_gym_eval
    import mpc_gym_oracle as MG
    import test_gpu_mpc_gym as T
    taken = {}
    for name in ("plain", "cem"):
        config = T._config(5)
        if name == "cem":
            config.mpc.cem = {"iterations": 1, "low": -0.5, "high": 0.5}
        env = FakePushEnv()
        four = MPC_gym_eval.fetch_push_control_evaluation(T.ARGS, *T._fixture_modules(), MG.GymTrajectories(43), config, env)
        assert len(four) == 4 and all(np.isfinite(v) for v in four) and 0.0 <= four[3] <= 1.0
        taken[name] = np.stack(env.actions)
    assert taken["cem"].shape == taken["plain"].shape and (np.abs(taken["cem"]) <= 0.5).all()
    assert not np.array_equal(taken["cem"], taken["plain"])


def test_the_planner_kernels_are_timed(models):
    from ndivplanning_amd import _capi
    from ndivplanning_amd import evaluation as E
    frames, actions = _mpc_inputs(1, 3)
    _capi.timing_enable(True)
    try:
        E.mpc_plan(models, frames, actions, 4, 2, cem=E.CemSettings(iterations=2))
        torch.cuda.synchronize()
        seen = _capi.timing_collect()
    finally:
        _capi.timing_enable(False)
    assert seen["k_plan_cem_update"][1] == 2 * 2 and seen["k_normal_noise"][1] == 1, sorted(seen)


def test_launch_counts_of_the_planner_without_cem(models):
    """mpc_plan without `cem` at T = 4, Th = 2: S = 2 + 2 + 1 horizon steps in T - 1 planning steps.  One generator,
    one code-input and one forward-model launch per horizon step, one encoder pass per horizon step and one for the goal,
    one selection per planning step, and nothing of the refinement."""
    from ndivplanning_amd import _capi
    from ndivplanning_amd import evaluation as E
    b, t, r, th = 2, 4, 4, 2
    frames, actions = _mpc_inputs(b, t)
    s = sum(min(th, t - 1 - i) for i in range(t - 1))
    assert s == 5
    _capi.timing_enable(True)
    try:
        E.mpc_plan(models, frames, actions, r, th, seed=1)
        torch.cuda.synchronize()
        seen = _capi.timing_collect()
    finally:
        _capi.timing_enable(False)
    counts = {k: v[1] for k, v in seen.items()}
    print(sorted(counts.items()))
    assert counts["k_g_fwd"] == s and counts["k_eval_g_input"] == s and counts["k_fm_image_cols"] == s, counts
    assert counts["k_enc_conv1"] == s + 1 and counts["k_eval_select"] == t - 1, counts
    assert "k_plan_cem_update" not in counts and "k_normal_noise" not in counts, counts


def test_mpc_eval_cli_with_and_without_the_cem_mapping(tmp_path):
    import yaml
    sys.path.insert(0, ROOT)
    import models.forward_encoder  # noqa: F401  (the class paths the training scripts record)
    import models.gan  # noqa: F401
    import models.image_autoencoder  # noqa: F401
    from ndivplanning_amd import evaluation as E
    from ndivplanning_amd.utils.file import DotMap
    enc, fm, gen = _modules()
    paths = {}
    for key, m in (("image_encoder_model_path", enc), ("forward_model_autoencoder_path", fm), ("gan_decoder_model_path", gen)):
        paths[key] = str(tmp_path / (key + ".pt"))
        torch.save(m, paths[key])
    cfg = dict(paths, random_seed=3, gpu_id=0, evaluation_data_path="synthetic:2:frames_u8", trajectory_length=3,
               evaluation={"batch_size": 1, "num_sample": 1, "noise_dim": 2, "threshold": 0.05},
               mpc={"rollouts": 4, "time_horizon": 2})
    printed = {}
    for name in ("plain", "cem"):
        if name == "cem":
            cfg["mpc"]["cem"] = {"iterations": 1, "elites": 2}
        yml = tmp_path / (name + ".yaml")
        yml.write_text(yaml.safe_dump(cfg))
        p = subprocess.run([sys.executable, os.path.join(ROOT, "mpc_eval.py"), "--config-file", str(yml)], cwd=str(tmp_path),
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        last = [ln for ln in p.stdout.splitlines() if ln.startswith("avg_action_error, avg_image_loss:")][-1]
        printed[name] = [float(v) for v in last.split(":")[1].split()]
        assert len(printed[name]) == 2 and all(np.isfinite(printed[name]))
    # without the key: the numbers of the planner as it was, mpc_plan without `cem` on the reference's noise stream
    config = DotMap({k: v for k, v in cfg.items() if k != "mpc"})
    config.mpc = DotMap({"rollouts": 4, "time_horizon": 2})
    data = E.make_eval_dataset(config)
    ev = E.EvalModels(enc, fm, gen, DEV)
    noise = E.reference_noise_schedule("mpc", 3, len(data), 1, 3, 1, 2, 4, 2)
    acc = torch.zeros(1, device=DEV)
    for i in range(len(data)):
        images, _, actions, _ = data[i]
        acts = torch.as_tensor(actions)[None].to(DEV).float()
        res = E.mpc_plan(ev, torch.as_tensor(images)[None], acts, 4, 2, noise=noise[i])
        ev.mse(acts[:, :2].contiguous(), res["actions"], 1, 8, acc=acc)
    want = [(acc[0] / (2 * len(data))).item(), (res["image_error_sum"][0] / (2 * len(data))).item()]
    assert printed["plain"] == [float(repr(v)) for v in want], (printed, want)
    assert printed["cem"] != printed["plain"]
