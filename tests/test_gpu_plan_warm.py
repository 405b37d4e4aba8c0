"""GPU tests of the planner's MPPI weighting and warm start: ndp_plan_update and ndp_plan_warm (csrc/ndp_plan.inc) against
the numpy restatements of tests/plan_warm_common.py on the host driver's cases, and mpc_plan / plan_step / MpcController /
the mpc_eval drop-in with the new `cem` settings (ndivplanning_amd/evaluation.py).  Random-weight models as in
test_gpu_plan_cem.py; B = 2, R = 8, W = 2, Th <= 3, T = 4."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import plan_common as C
import plan_warm_common as W
from fake_push_env import FakePushEnv
from test_gpu_eval import _modules, _mpc_inputs
from test_gpu_plan_cem import _replay

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
B, T, R, TH, NZ, WR = 2, 4, 8, 3, 2, 2


def _lib():
    from ndivplanning_amd import _build, _capi
    _build.build()
    return _capi.load()


# ------------------------------------------------------------------------------- the kernels on the host driver's cases
def _run_update(lib, c):
    from ndivplanning_amd import _capi
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(DEV) for k in ("err", "seq_in", "normal", "mean", "std", "best_err")}
    th, b, r, _ = c["seq_in"].shape
    seq_out = torch.full_like(t["seq_in"], -7.0)
    idx = torch.full((b, c["elites"]), -7, dtype=torch.int32, device=DEV)
    low, high = (_capi.c_float * 4)(*c["low"]), (_capi.c_float * 4)(*c["high"])
    _capi.check(lib.ndp_plan_update(_capi.ptr(t["err"]), _capi.ptr(t["seq_in"]), _capi.ptr(t["normal"]), b, r, th, c["elites"],
                                    c["weighting"], c["temperature"], c["smooth"], c["first"], c["momentum"], c["min_std"],
                                    low, high, _capi.ptr(t["mean"]), _capi.ptr(t["std"]), _capi.ptr(seq_out),
                                    _capi.ptr(t["best_err"]), _capi.ptr(idx), _capi.stream_ptr()), "ndp_plan_update")
    got = {"mean": t["mean"], "std": t["std"], "seq_out": seq_out, "best_err": t["best_err"], "elite_idx": idx}
    return {k: v.cpu().numpy() for k, v in got.items()}


def _run_warm(lib, c):
    from ndivplanning_amd import _capi
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(DEV) for k in ("mean_prev", "std_prev", "normal")}
    steps, b, w, _ = c["normal"].shape
    sp = c["mean_prev"].shape[1]
    mean, std = (torch.full((b, steps, 4), -7.0, device=DEV) for _ in range(2))
    warm = torch.full_like(t["normal"], -7.0)
    low, high = (_capi.c_float * 4)(*c["low"]), (_capi.c_float * 4)(*c["high"])
    _capi.check(lib.ndp_plan_warm(_capi.ptr(t["mean_prev"]), _capi.ptr(t["std_prev"]), _capi.ptr(t["normal"]), b, w, sp, steps,
                                  c["warm_std"], low, high, _capi.ptr(mean), _capi.ptr(std), _capi.ptr(warm),
                                  _capi.stream_ptr()), "ndp_plan_warm")
    return {"mean": mean.cpu().numpy(), "std": std.cpu().numpy(), "warm": warm.cpu().numpy()}


def test_update_against_the_restatement_on_the_host_drivers_cases():
    """Exact: elite_idx, best_err, row 0 of seq_out, and every output with weighting = elites (those with smooth = !first
    also against plan_common's restatement of ndp_plan_cem_update).  MPPI mean and std within 1 fp32 ulp, seq_out within
    ulp(mean) + |n| ulp(std) + ulp(result); the count of elements that differ at all is printed."""
    lib = _lib()
    differ = total = 0
    for c in W.update_cases():
        got = _run_update(lib, c)
        d, n = W.compare_update(c, got, W.plan_update(c))
        if c["weighting"] == W.MPPI:
            differ, total = differ + d, total + n
        elif c["smooth"] == 1 - c["first"]:
            want = C.cem_update(c)
            for o in C.OUTPUTS:
                assert C.bits_equal(got[o], want[o]), (c["name"], o)
    print("MPPI mean / std / seq_out: %d of %d elements differ from the restatement" % (differ, total))
    c = W.update_cases()[0]
    one, two = _run_update(lib, c), _run_update(lib, c)
    for o in one:
        assert C.bits_equal(one[o], two[o]), (o, "two calls differ")


def test_the_two_exact_limits_of_the_temperature():
    lib = _lib()
    for pair in W.limit_cases():
        W.check_limits(pair, _run_update(lib, pair[0]), None if pair[1] is None else _run_update(lib, pair[1]))


def test_warm_against_the_restatement_on_the_host_drivers_cases():
    lib = _lib()
    for c in W.warm_cases():
        got = _run_warm(lib, c)
        W.compare_warm(c, got, W.plan_warm(c))
        W.check_warm_special(c, got)
        again = _run_warm(lib, c)
        for o in got:
            assert C.bits_equal(got[o], again[o]), (c["name"], o, "two calls differ")


def test_refused_arguments_launch_nothing():
    lib = _lib()
    for over in W.REFUSED_UPDATE:
        assert W.refused_update(lib, **over) == 1, over               # NDP_E_ARG
    for over in W.REFUSED_WARM:
        assert W.refused_warm(lib, **over) == 1, over
    torch.cuda.synchronize()                                          # a launch on the made-up addresses would fault here


# ------------------------------------------------------------------------------- the planner
@pytest.fixture(scope="module")
def models():
    from ndivplanning_amd import evaluation as E
    return E.EvalModels(*_modules(), DEV)


def _streams(cem, b=B, t=T, seed=21):
    from ndivplanning_amd import evaluation as E
    g = torch.Generator().manual_seed(seed)
    noise = torch.rand(E.mpc_noise_floats(b, t, R, TH, NZ), generator=g).to(DEV)
    normal = torch.randn(E.plan_normal_floats(b, R, TH, cem, seq_length=t), generator=g).to(DEV)
    return noise, normal


def _step_inputs(models, b=B):
    frames, _ = _mpc_inputs(b, 2)
    state, goal = frames[:, 0].contiguous(), frames[:, 1].contiguous()
    return state, goal, models.encode(goal)


def test_the_default_settings_keep_the_bits_of_the_planner_as_it_was(models):
    """CemSettings with the new fields at their defaults: mpc_plan equals the restatement by hand on ndp_plan_cem_update
    (test_gpu_plan_cem._replay), which does not go through the planner; so does plan_step, against the first planning
    step of that restatement (T - 1 = Th: it has the full horizon and scores against the last frame); and spelling the
    defaults out changes nothing."""
    from ndivplanning_amd import evaluation as E
    cem = E.CemSettings(iterations=2)
    spelt = E.CemSettings(iterations=2, weighting="elites", temperature=None, warm_start=False, warm_rows=None, warm_std=None)
    frames, actions = _mpc_inputs(B, T)
    noise, normal = _streams(cem)
    assert normal.numel() == E.cem_normal_floats(B, R, TH, 2, seq_length=T)
    res = E.mpc_plan(models, frames, actions, R, TH, noise=noise, normal=normal, cem=cem)
    want = _replay(models, cem, frames, R, TH, noise, normal)
    for key in ("choices", "actions", "rollout_errors", "best_curve", "cem_mean", "cem_std"):
        assert torch.equal(res[key], want[key]), key
    again = E.mpc_plan(models, frames, actions, R, TH, noise=noise, normal=normal, cem=spelt)
    for key in res:
        assert torch.equal(res[key], again[key]), key
    assert T - 1 == TH
    state, goal = frames[:, 0].contiguous(), frames[:, T - 1].contiguous()
    goal_code = models.encode(goal)
    n1, n2 = noise[:E.plan_step_noise_floats(B, R, TH, NZ)], normal[:E.cem_normal_floats(B, R, TH, 2)]
    one = E.plan_step(models, state, goal, goal_code, R, TH, noise=n1, normal=n2, cem=cem)
    assert torch.equal(one[1], want["choices"][0]) and torch.equal(one[2], want["rollout_errors"][0])
    assert torch.equal(one[0], want["actions"][:, 0]) and torch.equal(one[4]["best_curve"], want["best_curve"][0])
    assert torch.equal(one[4]["best_err"], torch.fmin(want["best_trace"][0][-1], want["best_curve"][0][-1]))
    two = E.plan_step(models, state, goal, goal_code, R, TH, noise=n1, normal=n2, cem=spelt, prior=None)
    for x, y in zip(one[:4], two[:4]):
        assert torch.equal(x, y)
    for key in one[4]:
        assert torch.equal(one[4][key], two[4][key]), key


@pytest.mark.parametrize("weighting", ["elites", "mppi"])
def test_mpc_plan_with_warm_start_equals_a_loop_of_plan_step(models, weighting):
    """The replay by hand: plan_step(prior=...) per planning step on the same noise and normal slices, with the horizon
    mpc_plan gives the step; the next state is the chosen row of the forward model's pass on the last population's first
    actions from the broadcast state, the launch _plan_once took it from."""
    from ndivplanning_amd import evaluation as E
    cem = E.CemSettings(iterations=2, warm_start=True, warm_rows=WR, weighting=weighting,
                        temperature=0.01 if weighting == "mppi" else None, warm_std=0.1)
    frames, actions = _mpc_inputs(B, T)
    noise, normal = _streams(cem)
    res = E.mpc_plan(models, frames, actions, R, TH, noise=noise, normal=normal, cem=cem)
    per = frames.reshape(B, T, E.IMAGE_VALUES)
    goal = per[:, T - 1].contiguous().view(B, 3, 128, 128)
    goal_code = models.encode(goal)
    state = per[:, 0].contiguous().view(B, 3, 128, 128)
    off = n_off = 0
    prior = None
    for i in range(T - 1):
        steps = min(TH, T - 1 - i)
        n_noise = E.plan_step_noise_floats(B, R, steps, NZ)
        n_normal = E.plan_normal_floats(B, R, steps, cem, prior=prior is not None)
        action, pick, err, act0, info = E.plan_step(models, state, goal, goal_code, R, steps, noise=noise[off:off + n_noise],
                                                    normal=normal[n_off:n_off + n_normal], cem=cem, prior=prior)
        off, n_off = off + n_noise, n_off + n_normal
        assert torch.equal(pick, res["choices"][i]), i
        assert torch.equal(err, res["rollout_errors"][i]), i
        assert torch.equal(action, res["actions"][:, i]), i
        assert torch.equal(info["best_curve"], res["best_curve"][i]) and torch.equal(info["best_err"], res["best_err"][i]), i
        prior = info["cem_mean"], info["cem_std"]
        rep = state.view(B, 1, -1).expand(B, R, -1).reshape(B * R, 3, 128, 128).contiguous()
        pred0 = models.forward(rep, act0.reshape(B * R, 4)).view(B, R, -1)
        state = pred0.gather(1, pick.long().view(B, 1, 1).expand(B, 1, pred0.shape[2])).view(B, 3, 128, 128).contiguous()
    assert off == noise.numel() and n_off == normal.numel()
    assert torch.equal(prior[0], res["cem_mean"]) and torch.equal(prior[1], res["cem_std"])
    cold = E.mpc_plan(models, frames, actions, R, TH, noise=noise, cem=E.CemSettings(iterations=2), seed=1)
    assert torch.equal(res["best_curve"][0, 0], cold["best_curve"][0, 0])          # population 0 of the first step is cold


class _Watch:
    """Records the action operand of every forward-model call and the rows of the warm launch on an EvalModels."""

    def __init__(self, models):
        self.models, self.actions, self.warm, self.mean = models, [], None, None
        self._forward, self._plan_warm = models.forward, models.plan_warm
        models.forward, models.plan_warm = self.forward, self.plan_warm

    def forward(self, state, actions):
        self.actions.append(actions.clone())
        return self._forward(state, actions)

    def plan_warm(self, mean_prev, std_prev, normal, settings, mean, std, warm):
        self._plan_warm(mean_prev, std_prev, normal, settings, mean, std, warm)
        self.warm, self.mean = warm.clone(), mean.clone()

    def close(self):
        del self.models.forward, self.models.plan_warm                # the class's methods again


def test_population_0_of_a_warm_step(models):
    """Row R - W of seq is the clamped shifted mean at every horizon step, rows R - W + 1 .. R - 1 the launch's draws, and
    the rows below R - W are the generator's of the same call without injection."""
    from ndivplanning_amd import evaluation as E
    cem = E.CemSettings(iterations=1, warm_start=True, warm_rows=WR, low=-0.5, high=[0.5, 0.5, 0.25, 0.5])
    state, goal, goal_code = _step_inputs(models)
    g = torch.Generator().manual_seed(31)
    noise = torch.rand(E.plan_step_noise_floats(B, R, TH, NZ), generator=g).to(DEV)
    normal = torch.randn(E.plan_normal_floats(B, R, TH, cem, prior=True), generator=g).to(DEV)
    prior = (torch.randn(B, TH, 4, generator=g).to(DEV), (0.02 + 0.2 * torch.rand(B, TH, 4, generator=g)).to(DEV))
    seen = {}
    for name, kw in (("warm", {"prior": prior, "normal": normal}), ("cold", {"normal": normal[TH * B * WR * 4:]})):
        watch = _Watch(models)
        try:
            E.plan_step(models, state, goal, goal_code, R, TH, noise=noise, cem=cem, **kw)
        finally:
            watch.close()
        seen[name] = watch
    assert seen["cold"].warm is None and len(seen["warm"].actions) == len(seen["cold"].actions) == 2 * TH
    low, high = torch.tensor(cem.low, device=DEV), torch.tensor(cem.high, device=DEV)
    shifted = prior[0][:, [1, 2, 2]]
    assert torch.equal(seen["warm"].mean, shifted)
    for ts in range(TH):
        got, plain = seen["warm"].actions[ts].view(B, R, 4), seen["cold"].actions[ts].view(B, R, 4)
        assert torch.equal(got[:, R - WR], torch.minimum(torch.maximum(shifted[:, ts], low), high)), ts
        assert torch.equal(got[:, R - WR:], seen["warm"].warm[ts]), ts
        assert torch.equal(got[:, :R - WR], plain[:, :R - WR]), ts
    assert (seen["warm"].warm >= low).all() and (seen["warm"].warm <= high).all()


def test_batched_warm_plan_equals_single_trajectories(models):
    from ndivplanning_amd import evaluation as E
    b = 2
    cem = E.CemSettings(iterations=1, warm_start=True, warm_rows=WR, weighting="mppi", temperature=0.01)
    frames, actions = _mpc_inputs(b, T)
    horizon = [min(TH, T - 1 - i) for i in range(T - 1)]
    per_noise = [torch.rand(E.mpc_noise_floats(1, T, R, TH, NZ), generator=torch.Generator().manual_seed(50 + i))
                 for i in range(b)]
    per_normal = [torch.randn(E.plan_normal_floats(1, R, TH, cem, seq_length=T), generator=torch.Generator().manual_seed(70 + i))
                  for i in range(b)]
    batched = torch.stack([p.view(sum(horizon), R * NZ) for p in per_noise], dim=1).reshape(-1).to(DEV)
    pieces, off = [], 0
    for i, steps in enumerate(horizon):                               # [planning step]([steps,B,W,4])[iteration][steps,B,R,4]
        for rows in ([WR] if i else []) + [R] * cem.iterations:
            n = steps * rows * 4
            pieces.append(torch.stack([p[off:off + n].view(steps, rows, 4) for p in per_normal], dim=1).reshape(-1))
            off += n
    normal = torch.cat(pieces).to(DEV)
    res = E.mpc_plan(models, frames, actions, R, TH, noise=batched, normal=normal, cem=cem)
    again = E.mpc_plan(models, frames, actions, R, TH, noise=batched, normal=normal, cem=cem)
    for key in res:
        assert torch.equal(res[key], again[key]), key                 # bit-reproducible
    for i in range(b):
        one = E.mpc_plan(models, frames[i:i + 1], actions[i:i + 1], R, TH, noise=per_noise[i].to(DEV),
                         normal=per_normal[i].to(DEV), cem=cem)
        assert torch.equal(one["choices"][:, 0], res["choices"][:, i])
        assert torch.allclose(one["actions"][0], res["actions"][i], rtol=1e-5, atol=1e-6)
        assert torch.allclose(one["image_errors"][:, 0], res["image_errors"][:, i], rtol=1e-4, atol=1e-7)
        assert torch.allclose(one["rollout_errors"][:, 0], res["rollout_errors"][:, i], rtol=1e-4, atol=1e-7)
        assert torch.allclose(one["best_curve"][:, :, 0], res["best_curve"][:, :, i], rtol=1e-4, atol=1e-7)


def test_no_host_synchronisation_with_warm_start(models):
    from ndivplanning_amd import evaluation as E
    frames, actions = _mpc_inputs(2, 4)
    state, goal, goal_code = _step_inputs(models)
    for cem in (E.CemSettings(iterations=2, warm_start=True), E.CemSettings(iterations=1, warm_start=True, proposal="uniform",
                                                                           weighting="mppi", temperature=0.01)):
        first = E.plan_step(models, state, goal, goal_code, 4, 2, cem=cem)       # workspaces allocated outside the checked calls
        prior = first[4]["cem_mean"], first[4]["cem_std"]
        E.mpc_plan(models, frames, actions, 4, 2, cem=cem)
        E.plan_step(models, state, goal, goal_code, 4, 2, cem=cem, prior=prior)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            res = E.mpc_plan(models, frames, actions, 4, 2, cem=cem, seed=3)
            step = E.plan_step(models, state, goal, goal_code, 4, 2, cem=cem, seed=3, prior=prior)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        assert res["best_curve"].shape == (3, cem.iterations + 1, 2) and step[4]["best_curve"].shape == (cem.iterations + 1, 2)
        assert torch.isfinite(res["best_curve"]).all() and torch.isfinite(step[0]).all()


def test_controller_carries_the_fit_and_reset_drops_it(models):
    from ndivplanning_amd import evaluation as E
    env = FakePushEnv()
    goal = torch.from_numpy(np.pad(env.draw()[:, 16:144], ((4, 4), (0, 0), (0, 0))))[None]   # 128 x 128 of the scene
    frames = [env.render(mode="rgb_array")[None]]
    env.step(np.float32([0.3, -0.2, 0.0, 0.1]))
    frames.append(env.render(mode="rgb_array")[None])
    keys = ("rollout_errors", "choice", "actions0", "action", "best_curve", "best_err", "cem_mean", "cem_std")

    def run(cem, ctrl=None):
        ctrl = ctrl or E.MpcController(models, 6, 2, seed=5, cem=cem)
        ctrl.reset(goal)
        out = []
        for f in frames:
            actions, info = ctrl.act(f)
            assert sorted(info) == sorted(keys + ("state", "state_u8"))            # `info` is unchanged in its keys
            out.append((actions.clone(), {k: info[k].clone() for k in keys}))
        return out, ctrl
    cold, _ = run(E.CemSettings(iterations=2))
    warm, ctrl = run(E.CemSettings(iterations=2, warm_start=True))
    assert torch.equal(cold[0][0], warm[0][0])
    for k in keys:
        assert torch.equal(cold[0][1][k], warm[0][1][k]), k           # the first call has no fit to carry
    assert not torch.equal(cold[1][1]["rollout_errors"], warm[1][1]["rollout_errors"])
    assert not torch.equal(cold[1][1]["cem_mean"], warm[1][1]["cem_mean"])
    assert ctrl._prior is not None
    after, _ = run(None, ctrl)                                        # reset(): the first call is the cold one again
    assert torch.equal(after[0][0], cold[0][0])
    for k in keys:
        assert torch.equal(after[0][1][k], cold[0][1][k]), k
        assert torch.equal(after[1][1][k], warm[1][1][k]), k


def test_the_new_launches_are_timed_under_their_names(models):
    from ndivplanning_amd import _capi
    from ndivplanning_amd import evaluation as E
    frames, actions = _mpc_inputs(1, 3)
    cem = E.CemSettings(iterations=2, warm_start=True, weighting="mppi", temperature=0.01)
    _capi.timing_enable(True)
    try:
        E.mpc_plan(models, frames, actions, 4, 2, cem=cem)
        torch.cuda.synchronize()
        seen = _capi.timing_collect()
    finally:
        _capi.timing_enable(False)
    assert seen["k_plan_update"][1] == 2 * 2 and seen["k_plan_warm"][1] == 1 and seen["k_normal_noise"][1] == 1, sorted(seen)
    assert "k_plan_cem_update" not in seen


def test_mpc_eval_cli_with_mppi_and_warm_start(tmp_path):
    """The drop-in reads the new keys from `mpc.cem` and prints the figures of mpc_plan called directly with the same
    settings, the reference's noise stream and the drop-in's seeds."""
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
    mapping = {"iterations": 1, "elites": 2, "weighting": "mppi", "temperature": 0.01, "warm_start": True, "warm_rows": 1}
    cfg = dict(paths, random_seed=3, gpu_id=0, evaluation_data_path="synthetic:2:frames_u8", trajectory_length=3,
               evaluation={"batch_size": 1, "num_sample": 1, "noise_dim": 2, "threshold": 0.05},
               mpc={"rollouts": 4, "time_horizon": 2, "cem": mapping})
    yml = tmp_path / "warm.yaml"
    yml.write_text(yaml.safe_dump(cfg))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "mpc_eval.py"), "--config-file", str(yml)], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    last = [ln for ln in p.stdout.splitlines() if ln.startswith("avg_action_error, avg_image_loss:")][-1]
    printed = [float(v) for v in last.split(":")[1].split()]
    config = DotMap({k: v for k, v in cfg.items() if k != "mpc"})
    config.mpc = DotMap({"rollouts": 4, "time_horizon": 2})
    data = E.make_eval_dataset(config)
    ev = E.EvalModels(enc, fm, gen, DEV)
    cem = E.CemSettings(**mapping)
    noise = E.reference_noise_schedule("mpc", 3, len(data), 1, 3, 1, 2, 4, 2)
    acc = torch.zeros(1, device=DEV)
    for i in range(len(data)):
        images, _, actions, _ = data[i]
        acts = torch.as_tensor(actions)[None].to(DEV).float()
        res = E.mpc_plan(ev, torch.as_tensor(images)[None], acts, 4, 2, noise=noise[i], cem=cem, seed=3 + i)
        ev.mse(acts[:, :2].contiguous(), res["actions"], 1, 8, acc=acc)
    want = [(acc[0] / (2 * len(data))).item(), (res["image_error_sum"][0] / (2 * len(data))).item()]
    assert printed == [float(repr(v)) for v in want], (printed, want)
