"""GPU tests of the planner's gradient stage: ndp_plan_goal_grad, ndp_plan_grad_gather and ndp_plan_grad_step
(csrc/ndp_plan.inc) against the numpy restatements of tests/plan_grad_common.py on the host driver's cases, bit for bit;
the gradient the stage descends along against the fp64 and fp32 oracles; and mpc_plan / plan_step / MpcController / the
mpc_eval drop-in / push_world.closed_loop_mpc with `grad` (ndivplanning_amd/evaluation.py).

Comparison rule of the gradient (tests/test_gpu_input_grad.py, restated): with _rel(a, b) = |a - b| / |b| in fp64, the
kernels' error against the fp64 oracle may be at most max(2e-5, 2 x the fp32 CPU oracle's error against the same fp64
result).  That the error falls along grad_curve is not asserted: with random weights and ReLUs it is not a property of a
correct implementation; a sign error is caught by the gradient test."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import plan_common as C
import plan_grad_common as G
from fake_push_env import FakePushEnv
from oracle import forward_model_oracle as FO
from test_gpu_eval import _modules, _mpc_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
B, R, TH, T, NZ = 2, 5, 3, 3, 2


def _lib():
    from ndivplanning_amd import _build, _capi
    _build.build()
    return _capi.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------- the kernels on the host driver's cases
def _run_goal(lib, c, inplace=None):
    from ndivplanning_amd import _capi
    inplace = c["inplace"] if inplace is None else inplace
    pred, goal = _dev(c["pred"]), _dev(c["goal"])
    n = int(pred.shape[0])
    err = torch.full((n,), -7.0, device=DEV)
    d_pred = pred if inplace else torch.full_like(pred, -7.0)
    _capi.check(lib.ndp_plan_goal_grad(_capi.ptr(pred), n, _capi.ptr(goal), int(goal.shape[0]), c["rows_per_goal"],
                                       _capi.ptr(err), _capi.ptr(d_pred), _capi.stream_ptr()), "ndp_plan_goal_grad")
    return {"err": err.cpu().numpy(), "d_pred": d_pred.cpu().numpy()}


def _run_gather(lib, c):
    from ndivplanning_amd import _capi
    err, seq = _dev(c["err"]), _dev(c["seq"])
    th, b, r, _ = c["seq"].shape
    g = c["rows"]
    src, dst = (torch.full((b, g), -7, dtype=torch.int32, device=DEV) for _ in range(2))
    seq_g, m, v = (torch.full((th, b, g, 4), -7.0, device=DEV) for _ in range(3))
    _capi.check(lib.ndp_plan_grad_gather(_capi.ptr(err), _capi.ptr(seq), b, r, th, g, _capi.ptr(src), _capi.ptr(dst),
                                         _capi.ptr(seq_g), _capi.ptr(m), _capi.ptr(v), _capi.stream_ptr()), "ndp_plan_grad_gather")
    return {k: x.cpu().numpy() for k, x in (("src", src), ("dst", dst), ("seq_g", seq_g), ("m", m), ("v", v))}


def _run_step(lib, c):
    from ndivplanning_amd import _capi
    t = {k: _dev(c[k]) for k in ("grad", "seq_g", "m", "v", "err_g")}
    th, b, g, _ = c["seq_g"].shape
    curve = torch.full((b, g), -7.0, device=DEV)
    dst = None if c["dst"] is None else _dev(c["dst"])
    full = None if c["dst"] is None else _dev(c["seq_full"])
    low, high = (_capi.c_float * 4)(*c["low"]), (_capi.c_float * 4)(*c["high"])
    _capi.check(lib.ndp_plan_grad_step(_capi.ptr(t["grad"]), _capi.ptr(t["seq_g"]), _capi.ptr(t["m"]), _capi.ptr(t["v"]),
                                       _capi.ptr(t["err_g"]), b, g, th, c["t"], c["optimizer"], c["lr"], c["beta1"], c["beta2"],
                                       c["eps"], low, high, _capi.ptr(curve), _capi.ptr(dst), _capi.ptr(full), c["rollouts"],
                                       _capi.stream_ptr()), "ndp_plan_grad_step")
    got = {"seq_g": t["seq_g"], "m": t["m"], "v": t["v"], "curve": curve}
    if full is not None:
        got["seq_full"] = full
    return {k: x.cpu().numpy() for k, x in got.items()}


@pytest.fixture(scope="module")
def goal_wants():
    """The restatement of every goal case, computed once."""
    return [(c, G.goal_grad(c)) for c in G.goal_cases()]


def test_goal_grad_against_the_restatement(goal_wants):
    lib = _lib()
    for c, want in goal_wants:
        got = _run_goal(lib, c)
        G.compare(c, got, want, G.GOAL_OUTPUTS)
        again = _run_goal(lib, c)                                     # two calls give the same bits
        other = _run_goal(lib, c, inplace=1 - c["inplace"])           # in place equals out of place
        for o in G.GOAL_OUTPUTS:
            assert got[o].tobytes() == again[o].tobytes() == other[o].tobytes(), (c["name"], o)


def test_goal_grad_err_has_the_bits_of_score_select(goal_wants):
    from ndivplanning_amd import _capi
    lib = _lib()
    for c, _ in goal_wants:
        n, rpg = c["pred"].shape[0], c["rows_per_goal"]
        if n % rpg:
            continue                                                  # score_select scores whole trajectories
        pred, goal = _dev(c["pred"]), _dev(c["goal"])
        b = n // rpg
        err = torch.full((n,), -7.0, device=DEV)
        choice = torch.empty(b, dtype=torch.int32, device=DEV)
        act0, act = torch.zeros(n, 4, device=DEV), torch.empty(b, 4, device=DEV)
        _capi.check(lib.ndp_eval_score_select(_capi.ptr(pred), b, rpg, _capi.ptr(goal), int(goal.shape[0]), None, G.VALUES,
                                              _capi.ptr(act0), None, None, _capi.ptr(err), _capi.ptr(choice), _capi.ptr(act),
                                              None, _capi.stream_ptr()), "ndp_eval_score_select")
        got = _run_goal(lib, c, inplace=0)
        assert got["err"].tobytes() == err.cpu().numpy().tobytes(), c["name"]


def test_gather_against_the_restatement():
    lib = _lib()
    for c in G.gather_cases():
        got = _run_gather(lib, c)
        G.compare(c, got, G.grad_gather(c), G.GATHER_OUTPUTS)
        again = _run_gather(lib, c)
        for o in G.GATHER_OUTPUTS:
            assert got[o].tobytes() == again[o].tobytes(), (c["name"], o)


def test_step_against_the_restatement():
    lib = _lib()
    for c in G.step_cases():
        got = _run_step(lib, c)
        G.compare(c, got, G.grad_step(c), G.step_outputs(c))
        G.check_step_special(c, got)
        again = _run_step(lib, c)
        for o in G.step_outputs(c):
            assert got[o].tobytes() == again[o].tobytes(), (c["name"], o)


def test_refused_arguments_launch_nothing():
    lib = _lib()
    for fn, table in ((G.refused_goal, G.REFUSED_GOAL), (G.refused_gather, G.REFUSED_GATHER), (G.refused_step, G.REFUSED_STEP)):
        for over in table:
            assert fn(lib, **over) == 1, over                         # NDP_E_ARG
            assert lib.ndp_last_error()
    torch.cuda.synchronize()                                          # nothing was launched on the made-up addresses


# ------------------------------------------------------------------------------- the gradient
def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _check(mine, ref32, ref64, what):
    mine = mine.detach().cpu()
    assert torch.isfinite(mine).all(), what
    err_mine, err_ref = _rel(mine, ref64), _rel(ref32.detach(), ref64)
    print("%s: kernels %.3e, fp32 oracle %.3e" % (what, err_mine, err_ref))
    assert err_mine <= max(2e-5, 2.0 * err_ref), (what, err_mine, err_ref)


def _fm_state(seed):
    """init_forward_model_state with every BatchNorm overwritten (tests/test_gpu_input_grad.py: _fm_state): a gradient that
    ignored the running statistics or the weights would be wrong by tens of per cent."""
    state = FO.init_forward_model_state(seed)
    gen = torch.Generator().manual_seed(1000 + seed)
    for k in list(state):
        if k.endswith(".running_mean"):
            c = state[k].numel()
            base = k[:-len(".running_mean")]
            state[k] = torch.randn(c, generator=gen) * 0.05
            state[base + ".running_var"] = torch.rand(c, generator=gen) * 1.5 + 0.5
            state[base + ".weight"] = torch.rand(c, generator=gen) + 0.5
            state[base + ".bias"] = torch.randn(c, generator=gen) * 0.1
    return state


class _Spy:
    """An EvalModels whose gather and step calls are recorded: the gathered rows, and the population after the write-back."""

    def __init__(self, models):
        self._models = models
        self.gathered = self.population = None

    def __getattr__(self, name):
        return getattr(self._models, name)

    def grad_gather(self, err, seq, src, dst, seq_g, m, v):
        self._models.grad_gather(err, seq, src, dst, seq_g, m, v)
        self.gathered = seq_g.clone()

    def grad_step(self, grad, seq_g, m, v, err_g, t, settings, curve_out=None, dst=None, seq_full=None):
        self._models.grad_step(grad, seq_g, m, v, err_g, t, settings, curve_out, dst, seq_full)
        if seq_full is not None:
            self.population = seq_full.clone()


def _masks(models, slot, n):
    """The ReLU decisions of the pass kept in `slot` (forward_encoder.saved_relu_masks, on EvalModels' workspace)."""
    from ndivplanning_amd.forward_trainer import ForwardModelTrainer
    ws = models._fm_keep[slot]["ws"]
    masks = {}
    for name, (idx, side, ld, c0, c1) in ForwardModelTrainer._MAPS.items():
        off = models.lib.ndp_fm_workspace_offset(n, idx)
        view = ws[off:off + n * side * side * ld].view(n, side, side, ld)
        masks[name] = (view[..., c0:c1] > 0).permute(0, 3, 1, 2).contiguous().cpu()
    return masks


def test_the_gradient_against_the_oracles_and_the_written_rows():
    from ndivplanning_amd import evaluation as E
    from ndivplanning_amd.models import forward_encoder as FE
    torch.set_num_threads(8)
    b, r, th, g = 2, 4, 2, 2
    state_dict = _fm_state(8)
    fm = FE.ForwardAutoencoder()
    fm.load_state_dict(state_dict)
    enc, _, gen = _modules()
    models = _Spy(E.EvalModels(enc, fm.to(DEV).eval(), gen, DEV))
    rng = torch.Generator().manual_seed(9)
    state = torch.rand(b, 3, 128, 128, generator=rng) * 2.0 - 1.0
    goal = torch.rand(b, 3, 128, 128, generator=rng) * 2.0 - 1.0
    noise = torch.rand(E.plan_step_noise_floats(b, r, th, NZ), generator=rng).to(DEV)
    lr = 0.5
    grad = E.GradSettings(iterations=1, rows=g, optimizer="sgd", lr=lr, low=-0.75, high=0.75)
    goal_code = models.encode(goal.to(DEV))
    plain = E.plan_step(models, state.to(DEV), goal.to(DEV), goal_code, r, th, noise=noise)
    action, pick, err, act0, info = E.plan_step(models, state.to(DEV), goal.to(DEV), goal_code, r, th, noise=noise, grad=grad)
    rows, curve = info["grad_rows"].cpu(), info["grad_curve"].cpu()
    src, dst = info["grad_src"].cpu().long(), info["grad_dst"].cpu().long()
    assert rows.shape == (th, b, g, 4) and curve.shape == (1, b, g)
    n = b * g
    masks = [_masks(models, ts, n) for ts in range(th)]
    assert all(sorted(m) == sorted(FO.RELU_SITES) for m in masks)
    seq_g = models.gathered.cpu()                                      # [Th,B,G,4]: the rows the gradient was taken at
    acts = seq_g.reshape(th, n, 4).transpose(0, 1).contiguous()        # [n,Th,4], rows (b, g)
    cur = state.repeat_interleave(g, dim=0)
    tgt = goal.repeat_interleave(g, dim=0)

    def oracle(dtype):
        s = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in state_dict.items()}
        a = acts.to(dtype).clone().requires_grad_(True)
        y = cur.to(dtype)
        for t in range(th):
            y = FO.forward(s, y, a[:, t], training=False, relu_masks=masks[t])
        ls = ((y - tgt.to(dtype)) ** 2).flatten(1).mean(dim=1)
        ls.sum().backward()
        return ls.detach(), a.grad
    loss64, grad64 = oracle(torch.float64)
    loss32, grad32 = oracle(torch.float32)
    mine = rows.reshape(th, n, 4).transpose(0, 1).contiguous()
    _check(curve[0].reshape(n), loss32, loss64, "grad_curve[0]")
    _check(mine, grad32, grad64, "grad_rows")
    assert float(grad64.abs().max()) > 0
    # the gathered rows are the best rows of the population that was scored, and grad_curve[0] their errors
    pop_plain = plain[3].cpu()                                          # [B,R,4], ts = 0
    assert torch.equal(seq_g[0], pop_plain.gather(1, src.view(b, g, 1).expand(b, g, 4)))
    assert torch.equal(src, torch.from_numpy(np.stack([C.rank_order(e)[:g] for e in plain[2].cpu().numpy()])))
    assert torch.equal(dst, torch.from_numpy(np.stack([C.rank_order(e)[r - g:] for e in plain[2].cpu().numpy()])))
    # the dst rows of the population are clamp(src rows - lr * grad_rows) from the restatement, bit for bit
    want = G.grad_step({"grad": rows.numpy(), "seq_g": seq_g.numpy(), "m": np.zeros_like(rows.numpy()),
                        "v": np.zeros_like(rows.numpy()), "err_g": curve[0].numpy(), "t": 1, "optimizer": G.SGD, "lr": lr,
                        "beta1": grad.beta1, "beta2": grad.beta2, "eps": grad.eps, "low": np.float32(grad.low),
                        "high": np.float32(grad.high), "dst": None, "seq_full": None})["seq_g"]
    population = models.population.cpu()                               # [Th,B,R,4]
    written = population.gather(2, dst.view(1, b, g, 1).expand(th, b, g, 4))
    assert C.bits_equal(written.numpy(), want)
    assert torch.equal(population[0], act0.cpu())
    assert (written.abs() <= 0.75).all()
    # every other row equals the call without `grad`: its first action and its error
    keep = torch.ones(b, r, dtype=torch.bool)
    keep.scatter_(1, dst, False)
    assert torch.equal(act0.cpu()[keep], pop_plain[keep]) and torch.equal(err.cpu()[keep], plain[2].cpu()[keep])
    assert not torch.equal(act0.cpu()[~keep], pop_plain[~keep])


# ------------------------------------------------------------------------------- the planner
@pytest.fixture(scope="module")
def models():
    from ndivplanning_amd import evaluation as E
    return E.EvalModels(*_modules(), DEV)


def _settings(with_cem):
    from ndivplanning_amd import evaluation as E
    cem = E.CemSettings(iterations=1, elites=2) if with_cem else None
    return cem, E.GradSettings(iterations=2, rows=2, lr=0.05)


def _streams(cem, seed=31):
    from ndivplanning_amd import evaluation as E
    g = torch.Generator().manual_seed(seed)
    noise = torch.rand(E.mpc_noise_floats(B, T, R, TH, NZ), generator=g).to(DEV)
    normal = None if cem is None else torch.randn(E.plan_normal_floats(B, R, TH, cem, seq_length=T), generator=g).to(DEV)
    return noise, normal


def _step_inputs(models):
    frames, _ = _mpc_inputs(B, 2)
    state, goal = frames[:, 0].contiguous(), frames[:, 1].contiguous()
    return state, goal, models.encode(goal)


@pytest.mark.parametrize("with_cem", [False, True], ids=["plain", "cem"])
def test_zero_iterations_give_the_bits_of_the_planner_without_grad(models, with_cem):
    from ndivplanning_amd import evaluation as E
    cem, _ = _settings(with_cem)
    off = E.GradSettings(iterations=0, rows=2)
    frames, actions = _mpc_inputs(B, T)
    noise, normal = _streams(cem)
    plain = E.mpc_plan(models, frames, actions, R, TH, noise=noise, normal=normal, cem=cem)
    zero = E.mpc_plan(models, frames, actions, R, TH, noise=noise, normal=normal, cem=cem, grad=off)
    for key in plain:
        assert torch.equal(plain[key], zero[key]), key
    assert zero["grad_curve"].shape == (T - 1, 0, B, 2) and (zero["grad_src"] == -1).all() and (zero["grad_dst"] == -1).all()
    state, goal, goal_code = _step_inputs(models)
    n1 = noise[:E.plan_step_noise_floats(B, R, TH, NZ)]
    n2 = None if cem is None else normal[:E.plan_normal_floats(B, R, TH, cem)]
    one = E.plan_step(models, state, goal, goal_code, R, TH, noise=n1, normal=n2, cem=cem)
    two = E.plan_step(models, state, goal, goal_code, R, TH, noise=n1, normal=n2, cem=cem, grad=off)
    assert len(one) == (5 if with_cem else 4) and len(two) == 5 and "grad_rows" not in two[4]
    for x, y in zip(one[:4], two[:4]):
        assert torch.equal(x, y)
    if with_cem:
        for key in one[4]:
            assert torch.equal(one[4][key], two[4][key]), key


@pytest.mark.parametrize("with_cem", [False, True], ids=["plain", "cem"])
def test_the_chosen_error_never_rises_and_the_other_rows_keep_their_bits(models, with_cem):
    from ndivplanning_amd import evaluation as E
    cem, grad = _settings(with_cem)
    state, goal, goal_code = _step_inputs(models)
    noise, normal = _streams(cem)
    n1 = noise[:E.plan_step_noise_floats(B, R, TH, NZ)]
    n2 = None if cem is None else normal[:E.plan_normal_floats(B, R, TH, cem)]
    off = E.plan_step(models, state, goal, goal_code, R, TH, noise=n1, normal=n2, cem=cem)
    on = E.plan_step(models, state, goal, goal_code, R, TH, noise=n1, normal=n2, cem=cem, grad=grad)
    again = E.plan_step(models, state, goal, goal_code, R, TH, noise=n1, normal=n2, cem=cem, grad=grad)
    info = on[4]
    assert info["grad_curve"].shape == (2, B, 2) and info["grad_rows"].shape == (TH, B, 2, 4)
    assert torch.isfinite(info["grad_curve"]).all() and torch.isfinite(info["grad_rows"]).all()
    picked_off = off[2].gather(1, off[1].long().view(B, 1))
    picked_on = on[2].gather(1, on[1].long().view(B, 1))
    print("chosen error without / with grad:", picked_off.view(-1).tolist(), picked_on.view(-1).tolist())
    assert (picked_on <= picked_off).all()
    src, dst = info["grad_src"].long(), info["grad_dst"].long()
    for i in range(B):
        assert not set(src[i].tolist()) & set(dst[i].tolist())
    keep = torch.ones(B, R, dtype=torch.bool, device=DEV)
    keep.scatter_(1, dst, False)
    assert torch.equal(on[2][keep], off[2][keep]) and torch.equal(on[3][keep], off[3][keep])
    # the refined rows start as the best rows.  Their errors come from passes on B * G rows, the population's from B * R
    # rows -- other launch variants of the same fp32 arithmetic --, so they agree as tests/test_gpu_plan_cem.py holds a
    # batched plan to single trajectories: rtol 1e-4
    assert torch.allclose(info["grad_curve"][0], off[2].gather(1, src), rtol=1e-4, atol=1e-7)
    for x, y in zip(on[:4], again[:4]):                                # two calls give the same bits
        assert torch.equal(x, y)
    for key in info:
        assert torch.equal(info[key], again[4][key]), key
    if with_cem:
        assert info["best_curve"].shape == (cem.iterations + 1, B)    # best_curve keeps its I + 1 entries
        assert torch.equal(info["best_curve"][:cem.iterations], off[4]["best_curve"][:cem.iterations])
        for key in ("cem_mean", "cem_std"):                           # the fit is untouched by the stage
            assert torch.equal(info[key], off[4][key]), key


@pytest.mark.parametrize("with_cem", [False, True], ids=["plain", "cem"])
def test_mpc_plan_equals_a_loop_of_plan_step(models, with_cem):
    from ndivplanning_amd import evaluation as E
    cem, grad = _settings(with_cem)
    frames, actions = _mpc_inputs(B, T)
    noise, normal = _streams(cem)
    res = E.mpc_plan(models, frames, actions, R, TH, noise=noise, normal=normal, cem=cem, grad=grad)
    assert res["grad_curve"].shape == (T - 1, 2, B, 2) and res["grad_src"].shape == (T - 1, B, 2)
    if with_cem:
        assert res["best_curve"].shape == (T - 1, cem.iterations + 1, B)
    per = frames.reshape(B, T, E.IMAGE_VALUES)
    goal = per[:, T - 1].contiguous().view(B, 3, 128, 128)
    goal_code = models.encode(goal)
    state = per[:, 0].contiguous().view(B, 3, 128, 128)
    off = n_off = 0
    for i in range(T - 1):
        steps = min(TH, T - 1 - i)
        n_noise = E.plan_step_noise_floats(B, R, steps, NZ)
        n_normal = 0 if cem is None else E.plan_normal_floats(B, R, steps, cem)
        action, pick, err, act0, info = E.plan_step(models, state, goal, goal_code, R, steps, noise=noise[off:off + n_noise],
                                                    normal=None if cem is None else normal[n_off:n_off + n_normal],
                                                    cem=cem, grad=grad)
        off, n_off = off + n_noise, n_off + n_normal
        assert torch.equal(pick, res["choices"][i]) and torch.equal(err, res["rollout_errors"][i]), i
        assert torch.equal(action, res["actions"][:, i]), i
        for key in ("grad_curve", "grad_src", "grad_dst"):
            assert torch.equal(info[key], res[key][i]), (i, key)
        if with_cem:
            assert torch.equal(info["best_curve"], res["best_curve"][i]), i
        rep = state.view(B, 1, -1).expand(B, R, -1).reshape(B * R, 3, 128, 128).contiguous()
        pred0 = models.forward(rep, act0.reshape(B * R, 4)).view(B, R, -1)
        state = pred0.gather(1, pick.long().view(B, 1, 1).expand(B, 1, pred0.shape[2])).view(B, 3, 128, 128).contiguous()
    assert off == noise.numel() and (cem is None or n_off == normal.numel())


def test_no_host_synchronisation_with_grad(models):
    from ndivplanning_amd import evaluation as E
    frames, actions = _mpc_inputs(B, T)
    state, goal, goal_code = _step_inputs(models)
    for with_cem in (False, True):
        cem, grad = _settings(with_cem)
        E.mpc_plan(models, frames, actions, R, TH, cem=cem, grad=grad)     # workspaces allocated outside the checked calls
        E.plan_step(models, state, goal, goal_code, R, TH, cem=cem, grad=grad)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            res = E.mpc_plan(models, frames, actions, R, TH, cem=cem, grad=grad, seed=3)
            step = E.plan_step(models, state, goal, goal_code, R, TH, cem=cem, grad=grad, seed=3)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        assert res["grad_curve"].shape == (T - 1, 2, B, 2) and step[4]["grad_curve"].shape == (2, B, 2)
        assert torch.isfinite(res["grad_curve"]).all() and torch.isfinite(step[0]).all()


def test_the_new_launches_are_timed_under_their_names(models):
    from ndivplanning_amd import _capi
    from ndivplanning_amd import evaluation as E
    state, goal, goal_code = _step_inputs(models)
    _, grad = _settings(False)
    _capi.timing_enable(True)
    try:
        E.plan_step(models, state, goal, goal_code, R, TH, grad=grad, seed=2)
        torch.cuda.synchronize()
        seen = _capi.timing_collect()
    finally:
        _capi.timing_enable(False)
    assert seen["k_plan_grad_gather"][1] == 1 and seen["k_plan_goal_grad"][1] == 2 and seen["k_plan_grad_step"][1] == 2, seen
    assert seen["k_eval_select"][1] == 2                              # the stage's selection and the last one


def test_controller_returns_the_added_keys(models):
    from ndivplanning_amd import evaluation as E
    env = FakePushEnv()
    goal = torch.from_numpy(np.pad(env.draw()[:, 16:144], ((4, 4), (0, 0), (0, 0))))[None]   # 128 x 128 of the scene
    grad = E.GradSettings(iterations=1, rows=2, low=-0.5, high=[0.5, 0.5, 0.25, 0.5])
    for cem in (None, E.CemSettings(iterations=1)):
        ctrl = E.MpcController(models, 4, 2, seed=5, cem=cem, grad=grad)
        ctrl.reset(goal)
        for _ in range(2):
            actions, info = ctrl.act(env.render(mode="rgb_array")[None])
            assert actions.shape == (1, 4) and torch.isfinite(actions).all()
            assert info["grad_curve"].shape == (1, 1, 2) and info["grad_rows"].shape == (2, 1, 2, 4)
            assert info["grad_src"].shape == (1, 2) and info["grad_dst"].shape == (1, 2)
            assert ("best_curve" in info) == (cem is not None)
            assert torch.equal(info["action"].cpu(), actions)
            env.step(actions.numpy().ravel())


def test_closed_loop_mpc_in_the_push_world_with_grad(models):
    from ndivplanning_amd import evaluation as E
    from ndivplanning_amd import push_world as P
    runs = []
    for grad in (None, E.GradSettings(iterations=1, rows=1), E.GradSettings(iterations=1, rows=1)):
        world = P.PushWorld(2, DEV, seed=8)
        for _ in range(2):
            world.step(P.expert_actions(world.state), render=False)
        goal_frames = world.render()
        world.reset(render=False)
        runs.append(P.closed_loop_mpc(models, world, goal_frames, steps=2, rollouts=3, horizon=2, seed=1, grad=grad))
    assert tuple(runs[1]["actions"].shape) == (2, 2, 4) and torch.isfinite(runs[1]["actions"]).all()
    assert torch.equal(runs[1]["actions"], runs[2]["actions"]) and torch.equal(runs[1]["distance"], runs[2]["distance"])


def test_mpc_eval_cli_with_the_grad_mapping(tmp_path):
    """The drop-in reads `mpc.grad` and prints the figures of mpc_plan called directly with the same settings, the
    reference's noise stream and the drop-in's seeds."""
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
    mapping = {"iterations": 2, "rows": 2, "lr": 0.1, "optimizer": "adam"}
    cfg = dict(paths, random_seed=3, gpu_id=0, evaluation_data_path="synthetic:2:frames_u8", trajectory_length=3,
               evaluation={"batch_size": 1, "num_sample": 1, "noise_dim": 2, "threshold": 0.05},
               mpc={"rollouts": 4, "time_horizon": 2, "grad": mapping})
    yml = tmp_path / "grad.yaml"
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
    grad = E.GradSettings(**mapping)
    noise = E.reference_noise_schedule("mpc", 3, len(data), 1, 3, 1, 2, 4, 2)
    acc = torch.zeros(1, device=DEV)
    for i in range(len(data)):
        images, _, actions, _ = data[i]
        acts = torch.as_tensor(actions)[None].to(DEV).float()
        res = E.mpc_plan(ev, torch.as_tensor(images)[None], acts, 4, 2, noise=noise[i], grad=grad, seed=3 + i)
        ev.mse(acts[:, :2].contiguous(), res["actions"], 1, 8, acc=acc)
    want = [(acc[0] / (2 * len(data))).item(), (res["image_error_sum"][0] / (2 * len(data))).item()]
    assert printed == [float(repr(v)) for v in want], (printed, want)
    assert (res["grad_dst"] >= 0).all()
