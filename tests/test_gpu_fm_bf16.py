"""GPU: the eval-mode forward model with bf16 MFMA operands (ndp_fm_forward_lp with NDP_FM_BF16, ndp_fm_pack_params_lp;
k_fm_gemm's bf16 path in csrc/ndp_forward_model.inc) held to its definition in include/ndp.h, on the golden model of
tests/golden/fm_eval_case.npz at n = 1, 3 and 9 images (the K-split path with a partial 128-row tile; odd row counts; conv5
crossing a tile boundary with 144 rows; conv2 with 8 and more row tiles, the XCD order, at every n) and at n = 16, where
deconv5 changes from mode 1 of k_fm_gemm to k_fm_deconv32, both on the bf16 path (deconv6 takes it at every n), float and byte frames.

Bounds.  Layer by layer, so that nothing compounds: each of the nine layers' stored output against the fp64 convolution of
the ROUNDED device input and the rounded weights -- bf16 products are exact in fp32, only the order of the fp32 sum can
differ from torch's, so the bound is the project's adjudication rule for fp32 (tests/test_gpu_forward_model.py): the
relative-norm error against fp64 at most max(2e-5, 2 x that of torch's fp32 convolution of the same rounded operands).
End to end: the distance of the device's prediction from the UNROUNDED fp64 oracle at most twice the distance of the fp64
restatement of the definition (tests/fm_bf16_common.py: the oracle with the nine layers' operands rounded) from it."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fm_bf16_common as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SIZES = (1, 3, 9, 16)
FP32, BF16 = 0, 1
# FmTensor (csrc/ndp_forward_model.inc): the workspace maps, NHWC
T_CAT6, T_CAT5, T_CAT4, T_CAT3, T_CAT2 = 1, 2, 3, 4, 5
T_RAW2, T_RAW3, T_RAWU2, T_RAWU3, T_RAWU4, T_RAWU5, T_RAWU6 = 8, 9, 11, 12, 13, 14, 15
# layer: (oracle weight name, transposed, input map (tensor, side, stride, first channel, channels),
#         output map (tensor, side, stride, first channel, channels), ReLU in the launch)
LAYERS = {
    "conv2": ("encoder.conv2", False, (T_CAT6, 64, 128, 64, 64), (T_RAW2, 32, 128, 0, 128), False),
    "conv3": ("encoder.conv3", False, (T_CAT5, 32, 256, 128, 128), (T_RAW3, 16, 256, 0, 256), False),
    "conv4": ("encoder.conv4", False, (T_CAT4, 16, 512, 256, 256), (T_CAT3, 8, 1024, 512, 512), True),
    "conv5": ("encoder.conv5", False, (T_CAT3, 8, 1024, 512, 512), (T_CAT2, 4, 2048, 1024, 1024), True),
    "deconv2": ("decoder.deconv2", True, (T_CAT2, 4, 2048, 0, 2048), (T_RAWU2, 8, 512, 0, 512), False),
    "deconv3": ("decoder.deconv3", True, (T_CAT3, 8, 1024, 0, 1024), (T_RAWU3, 16, 256, 0, 256), False),
    "deconv4": ("decoder.deconv4", True, (T_CAT4, 16, 512, 0, 512), (T_RAWU4, 32, 128, 0, 128), False),
    "deconv5": ("decoder.deconv5", True, (T_CAT5, 32, 256, 0, 256), (T_RAWU5, 64, 64, 0, 64), False),
    "deconv6": ("decoder.deconv6", True, (T_CAT6, 64, 128, 0, 128), (T_RAWU6, 128, 32, 0, 32), False),
}
assert tuple(LAYERS) == L.NINE


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


class _Device:
    """The packed golden model on the device and the raw entry points."""

    def __init__(self, model):
        from ndivplanning_amd import _build, _capi
        from ndivplanning_amd.models.forward_encoder import pack_module
        _build.build()
        self.capi, self.lib = _capi, _capi.load()
        self.params, self.stats = pack_module(model, torch.device(DEV))
        self.lp = torch.empty(self.lib.ndp_fm_lp_weight_bytes(), dtype=torch.uint8, device=DEV)
        self.ws = {}

    def workspace(self, n):
        if n not in self.ws:
            ws = torch.empty(self.lib.ndp_fm_workspace_floats(n), dtype=torch.float32, device=DEV)
            p, st = self.capi.ptr, self.capi.stream_ptr()
            self.capi.check(self.lib.ndp_fm_pack_params(p(self.params), p(ws), st), "ndp_fm_pack_params")
            self.capi.check(self.lib.ndp_fm_pack_params_lp(p(self.params), p(ws), p(self.lp), st), "ndp_fm_pack_params_lp")
            self.ws[n] = ws
        return self.ws[n]

    def forward_lp(self, x, actions, precision, lp="own", out=None, check=True):
        """x: float [n,3,128,128] or bytes [n,128,128,3] on the device.  Returns (rc, out)."""
        n, p = int(x.shape[0]), self.capi.ptr
        u8 = x.dtype == torch.uint8
        out = torch.empty(n, 3, 128, 128, dtype=torch.float32, device=DEV) if out is None else out
        rc = self.lib.ndp_fm_forward_lp(p(self.params), p(self.stats), None if u8 else p(x), p(x) if u8 else None, p(actions), n,
                                        precision, p(self.lp if lp == "own" else lp), p(out), p(self.workspace(n)),
                                        self.capi.stream_ptr())
        if check:
            self.capi.check(rc, "ndp_fm_forward_lp")
        return rc, out

    def map(self, n, spec):
        tensor, side, ld, first, channels = spec
        off = self.lib.ndp_fm_workspace_offset(n, tensor)
        m = self.workspace(n)[off:off + n * side * side * ld].view(n, side, side, ld)[..., first:first + channels]
        return m.permute(0, 3, 1, 2).contiguous().cpu()              # NCHW on the host


@pytest.fixture(scope="module")
def case():
    torch.set_num_threads(8)
    model, frames_u8, images, actions = L.golden_case(max(SIZES))
    # the references, computed once and left alone: the unrounded fp64 oracle and the fp64 restatement of the definition
    exact = L.oracle_forward(model, images, actions, torch.float64)
    restated = L.oracle_forward(model, images, actions, torch.float64, rounded=True)
    return {"model": model, "dev": _Device(model), "frames_u8": frames_u8, "images": images, "actions": actions,
            "exact": exact, "restated": restated, "state": model.state_dict(), "runs": {}, "layer_refs": {}}


def _run(case, n, kind):
    """One bf16 pass at n images (float or byte frames): the prediction and the eighteen maps, on the host."""
    key = (n, kind)
    if key not in case["runs"]:
        dev = case["dev"]
        x = (case["frames_u8"][:n] if kind == "bytes" else case["images"][:n]).contiguous().to(DEV)
        _, out = dev.forward_lp(x, case["actions"][:n].contiguous().to(DEV), BF16)
        torch.cuda.synchronize()
        maps = {name: (dev.map(n, spec[2]), dev.map(n, spec[3])) for name, spec in LAYERS.items()}
        case["runs"][key] = {"out": out.cpu(), "maps": maps}
    return case["runs"][key]


def _layer_refs(case, n, name, x):
    """(fp64, torch fp32) outputs of layer `name` on the rounded device input x and the rounded weights, once per (n, layer)."""
    key = (n, name)
    if key not in case["layer_refs"]:
        wname, transposed, _, _, relu = LAYERS[name]
        w, b = case["state"][wname + ".weight"], case["state"][wname + ".bias"]
        xr, wr = L.round_tensor(x), L.round_tensor(w)
        assert np.array_equal(xr.numpy().view(np.uint32), L.to_bf16(x.numpy()).view(np.uint32))     # the stated rounding
        fn = F.conv_transpose2d if transposed else F.conv2d
        with torch.no_grad():
            r64 = fn(xr.double(), wr.double(), b.double(), stride=2, padding=1)
            r32 = fn(xr, wr, b, stride=2, padding=1)
            if relu:
                r64, r32 = F.relu(r64), F.relu(r32)
        case["layer_refs"][key] = (x, r64, r32)
    return case["layer_refs"][key]


def test_fp32_precision_gives_the_bits_of_ndp_fm_forward(case):
    dev = case["dev"]
    p = dev.capi.ptr
    for n in SIZES:
        a = case["actions"][:n].contiguous().to(DEV)
        for kind, fn in (("float", dev.lib.ndp_fm_forward), ("bytes", dev.lib.ndp_fm_forward_u8)):
            x = (case["frames_u8"][:n] if kind == "bytes" else case["images"][:n]).contiguous().to(DEV)
            want = torch.empty(n, 3, 128, 128, dtype=torch.float32, device=DEV)
            dev.capi.check(fn(p(dev.params), p(dev.stats), p(x), p(a), n, 0, p(want), p(dev.workspace(n)), dev.capi.stream_ptr()),
                           "ndp_fm_forward")
            _, got = dev.forward_lp(x, a, FP32, lp=None)              # lp_weights may be NULL
            _, got2 = dev.forward_lp(x, a, FP32)
            assert _bits(got) == _bits(want) == _bits(got2), (n, kind)
            assert _bits(got) != _bits(_run(case, n, kind)["out"])    # and bf16 is another computation


@pytest.mark.parametrize("kind", ["float", "bytes"])
@pytest.mark.parametrize("n", SIZES)
def test_every_bf16_layer_against_fp64_on_its_own_rounded_input(case, n, kind):
    run = _run(case, n, kind)
    report = []
    for name in L.NINE:
        x, got = run["maps"][name]
        x0, r64, r32 = _layer_refs(case, n, name, _run(case, n, "float")["maps"][name][0])
        assert _bits(x) == _bits(x0), (name, "byte and float frames feed this layer different bits")
        assert torch.isfinite(got).all() and got.shape == r64.shape, name
        err_mine, err_ref = L.rel_norm(got, r64), L.rel_norm(r32, r64)
        report.append("%s %.3g (torch fp32 %.3g)" % (name, err_mine, err_ref))
        assert err_mine <= max(2e-5, 2.0 * err_ref), (name, n, kind, err_mine, err_ref)
    print("n %d %s: relative-norm error against fp64: %s" % (n, kind, ", ".join(report)))


@pytest.mark.parametrize("kind", ["float", "bytes"])
@pytest.mark.parametrize("n", SIZES)
def test_end_to_end_within_twice_the_restatements_distance_from_the_unrounded_oracle(case, n, kind):
    got = _run(case, n, kind)["out"].double()
    assert torch.isfinite(got).all()
    for i in range(n):
        mine = float((got[i] - case["exact"][i]).norm())
        ref = float((case["restated"][i] - case["exact"][i]).norm())
        print("n %d %s image %d: |device - fp64 oracle| %.5g, |fp64 restatement - fp64 oracle| %.5g, |device - restatement| %.3g"
              % (n, kind, i, mine, ref, float((got[i] - case["restated"][i]).norm())))
        assert ref > 0 and mine <= 2.0 * ref, (n, kind, i, mine, ref)


def test_two_runs_and_byte_and_float_frames_give_identical_bits(case):
    dev = case["dev"]
    for n in SIZES:
        first = _run(case, n, "float")["out"]
        assert _bits(first) == _bits(_run(case, n, "bytes")["out"]), n
        a = case["actions"][:n].contiguous().to(DEV)
        for x in (case["images"][:n], case["frames_u8"][:n]):
            _, again = dev.forward_lp(x.contiguous().to(DEV), a, BF16)
            assert _bits(again) == _bits(first), n


def test_a_nan_pixel_gives_a_nan_prediction_for_that_image_only(case):
    dev, n = case["dev"], 3
    x = case["images"][:n].clone()
    x[1, 2, 77, 5] = float("nan")
    _, got = dev.forward_lp(x.to(DEV), case["actions"][:n].contiguous().to(DEV), BF16)
    got, clean = got.cpu(), _run(case, n, "float")["out"]
    assert torch.isnan(got[1]).any() and not torch.isnan(got[0]).any() and not torch.isnan(got[2]).any()
    assert _bits(got[0]) == _bits(clean[0]) and _bits(got[2]) == _bits(clean[2])


def _timed(dev, fn):
    dev.capi.timing_enable(True)
    try:
        result = fn()
        torch.cuda.synchronize()
        seen = dev.capi.timing_collect()
    finally:
        dev.capi.timing_enable(False)
    return result, {k: v[1] for k, v in seen.items()}


def test_input_grads_after_a_bf16_pass_are_unsupported_and_bad_arguments_launch_nothing(case):
    dev, n = case["dev"], 3
    p = dev.capi.ptr
    x, a = case["images"][:n].contiguous().to(DEV), case["actions"][:n].contiguous().to(DEV)
    xb = case["frames_u8"][:n].contiguous().to(DEV)
    ws = dev.workspace(n)
    d_out, d_act = torch.ones(n, 3, 128, 128, device=DEV), torch.full((n, 4), -7.0, device=DEV)
    grads = lambda: dev.lib.ndp_fm_input_grads(p(dev.params), p(d_out), n, None, p(d_act), p(ws), dev.capi.stream_ptr())  # noqa: E731
    dev.forward_lp(x, a, BF16)
    rc, counts = _timed(dev, grads)
    assert rc == 3 and counts == {} and b"ndp_fm_input_grads" in dev.lib.ndp_last_error()        # NDP_E_UNSUPPORTED
    assert bool((d_act == -7.0).all())
    # ... while after an fp32 pass through the same entry point they are there, once
    dev.forward_lp(x, a, FP32)
    assert grads() == 0 and bool((d_act != -7.0).any()) and grads() == 3
    # refused arguments: NDP_E_ARG, no launch, the output untouched
    out = torch.full((n, 3, 128, 128), -7.0, device=DEV)

    def refused():
        lib, st = dev.lib, dev.capi.stream_ptr()
        full = dict(params=p(dev.params), stats=p(dev.stats), x=p(x), xb=None, a=p(a), n=n, prec=BF16, lp=p(dev.lp), out=p(out),
                    ws=p(ws))
        rcs = []
        for over in ({"prec": 2}, {"prec": -1}, {"prec": 7, "lp": None}, {"lp": None}, {"xb": p(xb)}, {"x": None}, {"stats": None},
                     {"n": 0}, {"lp": dev.capi.c_void_p(dev.lp.data_ptr() + 2)}, {"params": None}, {"out": None}):
            k = dict(full, **over)
            rcs.append(lib.ndp_fm_forward_lp(k["params"], k["stats"], k["x"], k["xb"], k["a"], k["n"], k["prec"], k["lp"], k["out"],
                                             k["ws"], st))
        rcs.append(lib.ndp_fm_pack_params_lp(p(dev.params), p(ws), None, st))
        rcs.append(lib.ndp_fm_pack_params_lp(None, p(ws), p(dev.lp), st))
        return rcs

    rcs, counts = _timed(dev, refused)
    assert rcs == [1] * len(rcs) and counts == {}, (rcs, counts)
    assert bool((out == -7.0).all())
    assert dev.lib.ndp_fm_lp_weight_bytes() == 2 * sum(case["state"][LAYERS[k][0] + ".weight"].numel() for k in L.NINE)


def test_a_bf16_pass_shows_the_nine_bf16_launches_and_no_fp32_one_for_those_layers(case):
    dev = case["dev"]
    for n in (1, 9):
        x, a = case["images"][:n].contiguous().to(DEV), case["actions"][:n].contiguous().to(DEV)
        dev.workspace(n)
        _, counts = _timed(dev, lambda: dev.forward_lp(x, a, BF16))
        print(n, sorted(counts.items()))
        for name in L.NINE:
            assert counts.get("k_fm_gemm_bf16[%s]" % name) == 1, (name, counts)
            assert "k_fm_gemm[%s]" % name not in counts, (name, counts)
        assert not [k for k in counts if "deconv32" in k or "bf16" in k and not k.startswith("k_fm_gemm_bf16[")] and len([k for k in counts if k.startswith("k_fm_gemm_bf16[")]) == 9
        assert counts["k_fm_gemm[conv1]"] == 1 and counts["k_fm_gemm[conv6]"] == 1 and counts["k_fm_gemm[deconv1]"] == 1
        assert counts["k_fm_gemm[refine1]"] == 1 and counts["k_fm_r2_fwd"] == 1
        _, fp32 = _timed(dev, lambda: dev.forward_lp(x, a, FP32))
        assert not [k for k in fp32 if "bf16" in k] and all("k_fm_gemm[%s]" % name in fp32 for name in L.NINE)
    _, pack = _timed(dev, lambda: dev.capi.check(dev.lib.ndp_fm_pack_params_lp(
        dev.capi.ptr(dev.params), dev.capi.ptr(dev.workspace(1)), dev.capi.ptr(dev.lp), dev.capi.stream_ptr()), "pack"))
    assert pack == {"k_fm_pack_lp": 1}                                 # one launch


# ------------------------------------------------------------------------------------------------ the Python surface
@pytest.fixture(scope="module")
def planner():
    from test_gpu_eval import _modules
    from ndivplanning_amd import evaluation as E
    enc, fm, gen = _modules()
    return E, (enc, fm, gen), E.EvalModels(enc, fm, gen, DEV, fm_precision="bf16"), E.EvalModels(enc, fm, gen, DEV)


def test_plan_step_returns_the_errors_of_chaining_models_forward_by_hand(planner):
    E, _, models, models32 = planner
    from test_gpu_eval import _mpc_inputs
    b, r, th = 1, 3, 2
    frames, _ = _mpc_inputs(b, 3)
    imgs = models.images(frames.view(-1, *frames.shape[2:])).view(b, 3, 3, 128, 128)
    state, goal = imgs[:, 0].contiguous(), imgs[:, 2].contiguous()
    # the planner's rollout by hand: per horizon step the generator's actions for every row (from the step's piece of the
    # noise and the codes of the rows' own predictions), then models.forward on the rows
    nz = models.noise_dim
    noise = torch.rand(E.plan_step_noise_floats(b, r, th, nz), generator=torch.Generator().manual_seed(6)).to(DEV)
    goal_code = models.encode(goal)
    action, choice, err, actions0 = E.plan_step(models, state, goal, goal_code, r, th, noise=noise)
    cur = first = None
    for ts in range(th):
        piece = noise[ts * b * r * nz:(ts + 1) * b * r * nz]
        if ts == 0:
            first = models.generate(models.g_input(models.encode(state), r, goal_code, r, b * r), piece)
            cur = models.forward(state.repeat_interleave(r, 0).contiguous(), first)
        else:
            cur = models.forward(cur, models.generate(models.g_input(models.encode(cur), 1, goal_code, r, b * r), piece))
    by_hand = torch.empty(b, r, dtype=torch.float32, device=DEV)
    pick, act = torch.empty(b, dtype=torch.int32, device=DEV), torch.empty(b, 4, dtype=torch.float32, device=DEV)
    models.score_select(cur, b, r, goal, first, None, None, by_hand, pick, act, None)
    assert _bits(err) == _bits(by_hand)                                # bit for bit the errors of the hand-made chain
    want = ((cur - goal.repeat_interleave(r, 0)).double() ** 2).mean(dim=(1, 2, 3)).cpu()
    assert torch.allclose(err.view(-1).double().cpu(), want, rtol=1e-5)                          # ... which are the rows' MSEs
    assert _bits(actions0) == _bits(first)
    e = err.cpu().numpy().reshape(b, r)
    assert int(choice.cpu()[0]) == int(np.flatnonzero(e[0] == e[0].min())[0])                    # the first minimum
    assert _bits(action) == _bits(actions0.view(b, r, 4)[0, int(choice.cpu()[0])])
    # the same planning step in fp32 is another computation
    _, _, err32, _ = E.plan_step(models32, state, goal, models32.encode(goal), r, th, noise=noise)
    assert _bits(err32) != _bits(err) and torch.allclose(err32, err, rtol=0.05)
    with pytest.raises(ValueError, match=r"(?s)GradSettings\(.*bf16"):
        E.plan_step(models, state, goal, goal_code, 4, th, noise=noise, grad=E.GradSettings(iterations=1, rows=2))


def test_evaluate_and_the_mpc_eval_command_line_take_the_precision(planner, tmp_path, capsys, monkeypatch):
    import yaml
    E, (enc, fm, gen), _, _ = planner
    from ndivplanning_amd import forward_model_eval as FME
    from ndivplanning_amd import mpc_eval
    fm_dev = fm.to(DEV).eval()
    ds = FME.make_dataset("synthetic:2:frames_u8", seq_length=3)
    res = {p: FME.evaluate(fm_dev, ds, batch_size=2, precision=p) for p in ("fp32", "bf16")}
    plain = FME.evaluate(fm_dev, ds, batch_size=2)
    assert _bits(plain["errors"]) == _bits(res["fp32"]["errors"]) != _bits(res["bf16"]["errors"])
    assert torch.allclose(res["bf16"]["horizon_mse"], res["fp32"]["horizon_mse"], rtol=0.05)
    assert _bits(FME.evaluate(fm_dev, ds, batch_size=2, precision="bf16")["errors"]) == _bits(res["bf16"]["errors"])
    ckpt = str(tmp_path / "fm.pt")
    torch.save(fm.cpu(), ckpt)
    lines = []
    FME.main(["--model", ckpt, "--data", "synthetic:2:frames_u8", "--seq-length", "3", "--batch-size", "2", "--device", DEV,
              "--fm-precision", "bf16"], log=lambda *a: lines.append(" ".join(str(v) for v in a)))
    assert lines[0].startswith("val_pred_loss:") and lines[1].startswith("horizon 1: model_mse") and len(lines) == 3
    assert float(lines[0].split()[1]) == float(res["bf16"]["one_step_mse"].item())
    # mpc_eval --fm-precision bf16 on synthetic data: its usual lines
    sys.path.insert(0, ROOT)
    import models.forward_encoder  # noqa: F401  (the class paths the training scripts record)
    import models.gan  # noqa: F401
    import models.image_autoencoder  # noqa: F401
    paths = {}
    for key, m in (("image_encoder_model_path", enc), ("forward_model_autoencoder_path", fm), ("gan_decoder_model_path", gen)):
        paths[key] = str(tmp_path / (key + ".pt"))
        torch.save(m.cpu(), paths[key])
    cfg = dict(paths, random_seed=3, gpu_id=0, evaluation_data_path="synthetic:1:frames_u8", trajectory_length=3,
               evaluation={"batch_size": 1, "num_sample": 1, "noise_dim": 2, "threshold": 0.05},
               mpc={"rollouts": 3, "time_horizon": 2})
    yml = tmp_path / "eval.yaml"
    yml.write_text(yaml.safe_dump(cfg))
    monkeypatch.chdir(tmp_path)
    outs = {}
    for flag in ((), ("--fm-precision", "bf16"), ("--fm-precision", "fp32")):
        capsys.readouterr()
        result = mpc_eval.main(["--config-file", str(yml)] + list(flag))
        text = capsys.readouterr().out
        last = [ln for ln in text.splitlines() if ln.startswith("avg_action_error, avg_image_loss:")]
        assert len(last) == 1 and "tensor(" in text and all(np.isfinite(result)), text
        outs[flag] = result
    assert outs[()] == outs[("--fm-precision", "fp32")] and outs[()][1] != outs[("--fm-precision", "bf16")][1]
    cfg["evaluation"]["fm_precision"] = "bf16"                          # the config key, without the flag
    yml.write_text(yaml.safe_dump(cfg))
    assert mpc_eval.main(["--config-file", str(yml)]) == outs[("--fm-precision", "bf16")]
    cfg["evaluation"]["fm_precision"] = "fp16"
    yml.write_text(yaml.safe_dump(cfg))
    with pytest.raises(ValueError, match="'fp32' or 'bf16'"):
        mpc_eval.main(["--config-file", str(yml)])
