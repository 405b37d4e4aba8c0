"""CPU: precision NDP_FM_BF16 of the eval-mode forward model apart from its kernels -- the rounding (tests/fm_bf16_common.py
to_bf16 against torch's conversion, bit for bit except for which NaN a NaN becomes), the restatement (the wrapped oracle rounds the nine stride-2 layers and
no other), the arguments the Python surface refuses, the planner's call sequence (the same with both precisions), and the
size of the thing: how far the bf16 restatement lies from the unrounded fp64 oracle on the golden model.  The GPU tests
(tests/test_gpu_fm_bf16.py) hold the kernels to twice that distance."""
import types

import numpy as np
import pytest
import torch

import fm_bf16_common as L
import plan_common as C
from ndivplanning_amd import _eval_io
from ndivplanning_amd import evaluation as E
from ndivplanning_amd import forward_model_eval as FME


def _corpus():
    f = np.float32
    bits = np.array([
        0x00000000, 0x80000000,                          # +-0
        0x7F800000, 0xFF800000,                          # +-Inf
        0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FFF8000, 0x7F808000,     # NaNs, quiet and signalling, payloads
        0x7F7FFFFF, 0xFF7FFFFF,                          # the largest finite fp32 -> +-Inf
        0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000,              # the largest bf16, just below its tie to Inf, the tie (-> Inf)
        0x3F808000, 0x3F818000,                          # exact ties: down to the even 0x3F80, up to the even 0x3F82
        0xBF808000, 0xBF818000,                          # the same, negative
        0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,  # one fp32 ulp either side of the ties
        0x00008000, 0x00018000, 0x00000001, 0x007FFFFF, 0x00800000,                # denormals and the smallest normal
        0x3F800000, 0x3F7FFFFF, 0x40490FDB], np.uint32).view(f)
    rng = np.random.RandomState(0)
    rand = rng.randint(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32).view(f)
    ties = ((rng.randint(0, 1 << 16, 4096, dtype=np.uint32) << np.uint32(16)) | np.uint32(0x8000)).view(f)   # every one a tie
    return np.concatenate([bits, rand, ties, (rng.randn(4096) * 0.03).astype(f)])


def test_to_bf16_is_torchs_conversion_bit_for_bit():
    x = _corpus()
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = L.to_bf16_bits(x)
    nan = np.isnan(x)
    assert nan.sum() >= 6 and got.dtype == np.uint16
    assert np.array_equal(got[~nan], want[~nan]), np.flatnonzero((got != want) & ~nan)[:8]
    # NaN stays NaN in both (exponent all ones, a non-zero mantissa); which NaN is not part of the definition
    is_nan16 = lambda b: ((b & 0x7F80) == 0x7F80) & ((b & 0x007F) != 0)                     # noqa: E731
    assert is_nan16(got[nan]).all() and is_nan16(want[nan]).all() and not is_nan16(got[~nan]).any()
    # the named cases, by hand
    one = lambda b: int(L.to_bf16_bits(np.array([b], np.uint32).view(np.float32))[0])      # noqa: E731
    assert one(0x3F808000) == 0x3F80 and one(0x3F818000) == 0x3F82                           # ties go to even, both ways
    assert one(0x7F7FFFFF) == 0x7F80 and one(0xFF7FFFFF) == 0xFF80 and one(0x7F7F7FFF) == 0x7F7F
    assert one(0x80000000) == 0x8000 and one(0xFF800000) == 0xFF80 and one(0x7F800001) == 0x7FC0 and one(0xFFFFFFFF) == 0xFFFF
    # the float view of it, and the tensor helper the restatement uses
    v = L.to_bf16(x)
    assert v.dtype == np.float32 and np.array_equal(v.view(np.uint32)[~nan] >> 16, want[~nan].astype(np.uint32))
    assert np.isnan(v[nan]).all() and not (v.view(np.uint32) & 0xFFFF).any()
    t = L.round_tensor(torch.from_numpy(x)).numpy()
    assert np.array_equal(t.view(np.uint32)[~nan], v.view(np.uint32)[~nan]) and np.isnan(t[nan]).all()
    fin = np.isfinite(x)
    t64 = L.round_tensor(torch.from_numpy(x[fin]).double())
    assert t64.dtype == torch.float64 and np.array_equal(t64.numpy(), v[fin].astype(np.float64))


@pytest.fixture(scope="module")
def golden3():
    torch.set_num_threads(8)
    return L.golden_case(3)


def test_the_wrapped_oracle_rounds_the_nine_layers_and_no_other(golden3):
    model, _, images, actions = golden3
    log = []
    seen = {}
    import torch.nn.functional as F
    real = (F.conv2d, F.conv_transpose2d)
    plain = L.oracle_forward(model, images[:1], actions[:1], torch.float32)
    # what reaches torch's own functions under the wrapper: spy beneath it
    def spy(fn, name):
        def call(x, w, *a, **k):
            seen.setdefault(name, []).append((bool(torch.equal(L.round_tensor(x), x)), bool(torch.equal(L.round_tensor(w), w))))
            return fn(x, w, *a, **k)
        return call
    F.conv2d, F.conv_transpose2d = spy(real[0], "conv2d"), spy(real[1], "conv_transpose2d")
    try:
        got = L.oracle_forward(model, images[:1], actions[:1], torch.float32, rounded=True, log=log)
    finally:
        F.conv2d, F.conv_transpose2d = real
    assert (F.conv2d, F.conv_transpose2d) == real                      # the wrapper took itself off again
    assert len(log) == 14 and [c[0] for c in log].count("conv2d") == 8 and [c[0] for c in log].count("conv_transpose2d") == 6
    assert tuple(sorted(c[2] for c in log if c[3])) == tuple(sorted(L.NINE)) and sum(c[3] for c in log) == 9
    assert sorted(c[2] for c in log if not c[3]) == ["conv1", "conv6", "deconv1", "refine1", "refine2"]
    # beneath the wrapper: both operands of the nine are bf16 values, and of the other five neither is
    assert seen["conv2d"] == [(False, False)] + [(True, True)] * 4 + [(False, False)] * 3
    assert seen["conv_transpose2d"] == [(False, False)] + [(True, True)] * 5
    assert not torch.equal(got, plain) and L.rel_norm(got - images[:1], plain - images[:1]) < 0.1
    # a second forward inside one context counts from the start again
    log2 = []
    with L.rounded_layers(log2):
        from oracle import forward_model_oracle as FO
        s = L.oracle_state(model, torch.float32)
        with torch.no_grad():
            a = FO.forward(s, images[:1], actions[:1], training=False)
            b = FO.forward(s, images[:1], actions[:1], training=False)
    assert torch.equal(a, b) and torch.equal(a, got) and log2[:14] == log2[14:] == log


def test_unknown_precisions_are_refused_with_both_names():
    for bad in ("fp16", "BF16", "", None, 1):
        with pytest.raises(ValueError, match="'fp32' or 'bf16'"):
            _eval_io.fm_precision_code(bad)
        with pytest.raises(ValueError, match="'fp32' or 'bf16'"):
            E.EvalModels(None, None, None, fm_precision=bad)           # before any module or device is touched
    assert _eval_io.fm_precision_code("fp32") == 0 and _eval_io.fm_precision_code("bf16") == 1
    assert E.FM_PRECISIONS == ("fp32", "bf16")
    x = torch.zeros(1, 3, 128, 128)
    with pytest.raises(ValueError, match="'fp32' or 'bf16'"):
        FME.predict(None, x, torch.zeros(1, 4), precision="half")
    with pytest.raises(ValueError, match="'fp32' or 'bf16'"):
        FME.rollout(None, x, torch.zeros(1, 1, 4), precision="half")
    with pytest.raises(ValueError, match="'fp32' or 'bf16'"):
        FME.evaluate(None, [], precision="half")
    with pytest.raises(SystemExit):
        FME.make_parser().parse_args(["--model", "m", "--data", "d", "--fm-precision", "half"])
    assert FME.make_parser().parse_args(["--model", "m", "--data", "d"]).fm_precision == "fp32"
    assert FME.make_parser().parse_args(["--model", "m", "--data", "d", "--fm-precision", "bf16"]).fm_precision == "bf16"


def test_the_config_key_and_the_command_line():
    from ndivplanning_amd.utils.file import DotMap
    of = _eval_io.fm_precision_of
    assert of(DotMap({"evaluation": DotMap({"batch_size": 1})})) == "fp32"          # absent: fp32
    assert of(DotMap({"other": 1})) == "fp32"
    assert of(DotMap({"evaluation": DotMap({"fm_precision": "bf16"})})) == "bf16"
    # --fm-precision becomes a top-level key (argparse_util.override_dotmap) and wins
    assert of(DotMap({"fm_precision": "fp32", "evaluation": DotMap({"fm_precision": "bf16"})})) == "fp32"
    assert of(DotMap({"fm_precision": "bf16", "evaluation": DotMap({})})) == "bf16"
    for cfg in (DotMap({"evaluation": DotMap({"fm_precision": "fp8"})}), DotMap({"fm_precision": "tf32"})):
        with pytest.raises(ValueError, match="'fp32' or 'bf16'"):
            of(cfg)


class _Bf16Recording(C.RecordingModels):
    fm_precision = "bf16"


class _Fp32Recording(C.RecordingModels):
    fm_precision = "fp32"


def test_grad_with_a_bf16_models_object_is_refused_by_every_planner_entry_point():
    from ndivplanning_amd import push_world
    grad = E.GradSettings(iterations=1, rows=2)
    frames, actions = torch.zeros(1, 3, 3, 128, 128), torch.zeros(1, 3, 4)
    state = torch.zeros(1, 3, 128, 128)
    words = r"(?s)GradSettings\(.*bf16"
    for make in (_Bf16Recording,):
        models = make()
        with pytest.raises(ValueError, match=words):
            E.mpc_plan(models, frames, actions, 4, 2, grad=grad)
        with pytest.raises(ValueError, match=words):
            E.plan_step(models, state, state, torch.zeros(1, 128), 4, 2, grad=grad)
        with pytest.raises(ValueError, match=words):
            E.MpcController(models, 4, 2, grad=grad)
        world = types.SimpleNamespace(size=128, n=1)
        with pytest.raises(ValueError, match=words):
            push_world.closed_loop_mpc(models, world, torch.zeros(1, 128, 128, 3, dtype=torch.uint8), 1, 4, 2, grad=grad)
        assert models.calls == []                                      # refused before anything was asked of the models
    # the limits of `grad` itself come first, as before, and fp32 models (or ones without the attribute) plan with grad
    with pytest.raises(ValueError, match="exceeds half the 5 rollouts"):
        E.plan_step(_Bf16Recording(), state, state, torch.zeros(1, 128), 5, 2, grad=E.GradSettings(rows=3))
    for models in (_Fp32Recording(), C.RecordingModels()):
        E.mpc_plan(models, frames, actions, 4, 2, grad=E.GradSettings(iterations=0, rows=2), seed=1)
        assert models.calls


def test_the_planners_call_sequence_is_the_same_with_both_precisions():
    b, t, r, th = 2, 4, 4, 2
    g = torch.Generator().manual_seed(0)
    frames = torch.rand(b, t, 3, 128, 128, generator=g) * 2 - 1
    actions = torch.rand(b, t, 4, generator=g) * 2 - 1
    noise = torch.rand(E.mpc_noise_floats(b, t, r, th, 2), generator=g)
    for cem in (None, E.CemSettings(iterations=1)):
        runs = []
        for make in (_Fp32Recording, _Bf16Recording, C.RecordingModels):
            models = make()
            res = E.mpc_plan(models, frames, actions, r, th, noise=noise, cem=cem, seed=3)
            runs.append((models.calls, res))
        assert runs[0][0] == runs[1][0] == runs[2][0] and ("forward", b * r) in runs[0][0]
        for key in runs[0][1]:
            assert torch.equal(runs[0][1][key], runs[1][1][key]), key
    state, goal = frames[:, 0].contiguous(), frames[:, 1].contiguous()
    calls = []
    for make in (_Fp32Recording, _Bf16Recording):
        models = make()
        goal_code = models.encode(goal)
        del models.calls[:]
        E.plan_step(models, state, goal, goal_code, r, th, noise=noise[:E.plan_step_noise_floats(b, r, th, 2)])
        calls.append(models.calls)
    assert calls[0] == calls[1] and calls[0]


def test_the_restatements_distance_from_the_unrounded_oracle_on_the_golden_model(golden3):
    """What operand rounding costs, measured (printed): the distance of the fp64 bf16-restatement from the unrounded fp64
    oracle on the golden model -- the value the GPU test's end-to-end bound is relative to.  The band asserted here is only
    a check of the restatement itself: one rounding is a relative error of at most 2^-9 (rms 2^-9 / sqrt(3) for each of the
    two operands of a product), a sum of products with independent errors keeps that relative size, and nine such layers
    lie on the way -- so the residual's relative deviation is expected between a tenth of one layer's 2^-9 sqrt(2 / 3)
    = 1.6e-3 and ten times nine layers' worth: 1.6e-4 .. 0.15.  Measured: see the printed line (3 images: 1.66e-3)."""
    model, _, images, actions = golden3
    exact = L.oracle_forward(model, images, actions, torch.float64)
    restated = L.oracle_forward(model, images, actions, torch.float64, rounded=True)
    restated32 = L.oracle_forward(model, images, actions, torch.float32, rounded=True)
    x = images.double()
    rel = L.rel_norm(restated - x, exact - x)
    per_image = [float((restated[i] - exact[i]).norm()) for i in range(len(images))]
    print("bf16 restatement (fp64) against the unrounded fp64 oracle: residual relative deviation %.4g, max |d| %.4g, "
          "per-image L2 %s; fp32 restatement against the fp64 one: max |d| %.3g"
          % (rel, float((restated - exact).abs().max()), ["%.4g" % v for v in per_image],
             float((restated32.double() - restated).abs().max())))
    assert 1.6e-4 <= rel <= 0.15
    assert all(v > 0 for v in per_image)
