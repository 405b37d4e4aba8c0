"""CPU: precision NDP_ENC_BF16 of the image encoder's pass apart from its kernels -- the names and the config key of the
Python surface, the sizes and the workspace layout the host-only entry points state, the arguments the C entry points
refuse, the restatement (tests/enc_bf16_common.py: with the rounding switched off it is the oracle's network), the size of
the thing (how far the bf16 restatement lies from the unrounded fp64 oracle: the GPU tests hold the kernels to twice that),
and the planner's call sequence, which is the same with both precisions."""
import ctypes

import pytest
import torch

import enc_bf16_common as L
import plan_common as C
from ndivplanning_amd import _eval_io
from ndivplanning_amd import evaluation as E
from oracle import encoder_oracle as EO


@pytest.fixture(scope="module")
def lib():
    from ndivplanning_amd import _build, _capi
    _build.build()
    return _capi.load()


def test_unknown_precisions_are_refused_with_both_names():
    for bad in ("fp16", "BF16", "", None, 1):
        with pytest.raises(ValueError, match="enc_precision must be 'fp32' or 'bf16'"):
            _eval_io.enc_precision_code(bad)
        with pytest.raises(ValueError, match="enc_precision must be 'fp32' or 'bf16'"):
            E.EvalModels(None, None, None, enc_precision=bad)         # before any module or device is touched
    with pytest.raises(ValueError, match="enc_precision"):
        E.EvalModels(None, None, None, fm_precision="bf16", enc_precision="fp16")
    assert _eval_io.enc_precision_code("fp32") == 0 and _eval_io.enc_precision_code("bf16") == 1
    assert E.ENC_PRECISIONS == _eval_io.ENC_PRECISIONS == ("fp32", "bf16")


def test_the_config_key_and_the_command_line():
    from ndivplanning_amd.utils.file import DotMap
    of = _eval_io.enc_precision_of
    assert E.enc_precision_of is of
    assert of(DotMap({"evaluation": DotMap({"batch_size": 1})})) == "fp32"          # absent: fp32
    assert of(DotMap({"other": 1})) == "fp32"
    assert of(DotMap({"evaluation": DotMap({"enc_precision": "bf16"})})) == "bf16"
    # --enc-precision becomes a top-level key (argparse_util.override_dotmap) and wins
    assert of(DotMap({"enc_precision": "fp32", "evaluation": DotMap({"enc_precision": "bf16"})})) == "fp32"
    assert of(DotMap({"enc_precision": "bf16", "evaluation": DotMap({})})) == "bf16"
    # the forward model's key is another one
    assert of(DotMap({"fm_precision": "bf16", "evaluation": DotMap({"fm_precision": "bf16"})})) == "fp32"
    for cfg in (DotMap({"evaluation": DotMap({"enc_precision": "fp8"})}), DotMap({"enc_precision": "tf32"})):
        with pytest.raises(ValueError, match="'fp32' or 'bf16'"):
            of(cfg)


def test_the_shipped_configs_carry_the_key_as_fp32():
    import os
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in ("default.yaml", "evaluation.yaml"):
        cfg = yaml.safe_load(open(os.path.join(root, "config", name)))
        assert cfg["evaluation"]["enc_precision"] == "fp32" and cfg["evaluation"]["fm_precision"] == "fp32", name


def test_the_bf16_weight_buffer_and_the_workspace_layout(lib):
    assert lib.ndp_encoder_lp_weight_bytes() == 16728064 == 2 * L.LP_WEIGHT_VALUES
    per_image = [s * s * L.LAYERS[l][1] for l, s in enumerate(L.SIDES)]
    for n in (1, 17, 512, 513):
        c = min(n, 512)
        offs = [lib.ndp_encoder_lp_act_offset(l, n) for l in range(5)]
        assert offs[0] == 0 and all(o % 8 == 0 for o in offs), (n, offs)
        assert all(b > a for a, b in zip(offs, offs[1:])), (n, offs)              # monotone
        assert offs == [c * sum(per_image[:l]) for l in range(5)], (n, offs)       # consecutive, nothing between
        end = offs[4] + c * per_image[4]                                           # bf16 elements
        # behind the maps: the fp32 partial sums of a split layer, at most 1,024 tiles of 128 x 128 -- they start 16-byte
        # aligned and everything fits into the workspace both precisions share
        assert (2 * end) % 16 == 0
        assert 2 * end + 4 * 1024 * 128 * 128 <= 4 * lib.ndp_encoder_workspace_floats(n), n
        # the fp32 pass's own layout (the same maps as floats) is what sizes the workspace
        assert lib.ndp_encoder_workspace_floats(n) == c * sum(per_image) + 1024 * 128 * 128
    assert [lib.ndp_encoder_lp_act_offset(l, 3) for l in (-1, 5)] == [-1, -1] and lib.ndp_encoder_lp_act_offset(0, 0) == -1


def test_argument_errors_are_reported_without_launching(lib):
    """Every refused call returns NDP_E_ARG with a message that names the entry point, and touches no device: the
    pointers are never dereferenced (a refused call on a machine without a GPU returns the same)."""
    good = ctypes.c_void_p(0x10000)                                    # aligned, never read
    odd = ctypes.c_void_p(0x10004)
    full = dict(params=good, x=good, xb=None, n=3, prec=1, lp=good, codes=good, ws=good)
    cases = ({"prec": 2}, {"prec": -1}, {"prec": 7, "lp": None}, {"lp": None}, {"xb": good}, {"x": None}, {"n": 0}, {"n": -4},
             {"params": None}, {"codes": None}, {"ws": None}, {"lp": odd}, {"ws": odd}, {"codes": odd}, {"params": odd}, {"x": odd},
             {"prec": 0, "x": None}, {"prec": 0, "xb": good}, {"prec": 0, "ws": odd})
    for over in cases:
        k = dict(full, **over)
        rc = lib.ndp_encoder_forward_lp(k["params"], k["x"], k["xb"], k["n"], k["prec"], k["lp"], k["codes"], k["ws"], None)
        assert rc == 1 and b"ndp_encoder_forward_lp" in lib.ndp_last_error(), (over, rc, lib.ndp_last_error())
    for params, lp in ((None, good), (good, None), (None, None), (odd, good), (good, odd)):
        rc = lib.ndp_encoder_pack_params_lp(params, lp, None)
        assert rc == 1 and b"ndp_encoder_pack_params_lp" in lib.ndp_last_error(), (params, lp, rc)


@pytest.fixture(scope="module")
def case():
    torch.set_num_threads(8)
    state, packed, images = L.model_case(2)
    return state, packed, images


def test_the_restatement_without_rounding_is_the_oracles_network(case):
    state, packed, images = case
    want = EO.encoder_forward(state, images, dtype=torch.float64).reshape(-1, 128)
    # pack_encoder_params folds BatchNorm in fp32, so its buffer carries fp32 roundings of the folded weights that the fp64
    # oracle on the same state does not: the comparison at 1e-12 takes the same packing with the folding done in fp64
    # (L.pack_state), which in fp32 is pack_encoder_params' buffer
    assert (L.pack_state(state, torch.float32) - packed).abs().max() <= 1e-6 * packed.abs().max()
    assert L.pack_state(state, torch.float32).shape == packed.shape
    maps, got = L.restatement(L.pack_state(state, torch.float64), images, torch.float64, rounded=False)
    assert L.rel_norm(got, want) <= 1e-12, L.rel_norm(got, want)
    assert [tuple(m.shape[1:]) for m in maps] == [(L.LAYERS[l][1], s, s) for l, s in enumerate(L.SIDES)]
    # and on the fp32-folded buffer itself only those roundings remain
    _, got32 = L.restatement(packed, images, torch.float64, rounded=False)
    assert L.rel_norm(got32, want) <= 1e-6


def test_the_restatements_distance_from_the_unrounded_oracle(case):
    """What the rounding costs, measured (printed): the codes of the fp64 restatement against the unrounded fp64 oracle.
    The band asserted is a check of the restatement only: one rounding is a relative error of at most 2^-9 (rms 2^-9 /
    sqrt 3 per operand), a sum of products with independent errors keeps that relative size, five rounded layers lie on
    the way: between a tenth of one layer's 2^-9 sqrt(2 / 3) = 1.6e-3 and ten times five layers' worth, 1.6e-4 .. 0.08.
    Measured: 3.7e-3 (2 images)."""
    state, packed, images = case
    exact = EO.encoder_forward(state, images, dtype=torch.float64).reshape(-1, 128)
    _, restated = L.restatement(packed, images, torch.float64)
    _, restated32 = L.restatement(packed, images, torch.float32)
    rel = L.rel_norm(restated, exact)
    print("bf16 restatement (fp64) against the unrounded fp64 oracle: rel_norm of the codes %.4g; the fp32 restatement against "
          "the fp64 one %.3g" % (rel, L.rel_norm(restated32, restated)))
    assert 1.6e-4 <= rel <= 0.08
    # every stored map of the restatement is a bf16 value, and the codes are not rounded
    maps, codes = L.restatement(packed, images[:1], torch.float64)
    assert all(torch.equal(L.round_tensor(m), m) for m in maps) and not torch.equal(L.round_tensor(codes), codes)


class _Bf16Enc(C.RecordingModels):
    enc_precision = "bf16"


class _Fp32Enc(C.RecordingModels):
    enc_precision = "fp32"


class _BothBf16(C.RecordingModels):
    enc_precision = "bf16"
    fm_precision = "bf16"


def test_the_planners_call_sequence_is_the_same_with_both_encoder_precisions():
    b, t, r, th = 2, 4, 4, 2
    g = torch.Generator().manual_seed(0)
    frames = torch.rand(b, t, 3, 128, 128, generator=g) * 2 - 1
    actions = torch.rand(b, t, 4, generator=g) * 2 - 1
    noise = torch.rand(E.mpc_noise_floats(b, t, r, th, 2), generator=g)
    for cem in (None, E.CemSettings(iterations=1)):
        runs = []
        for make in (_Fp32Enc, _Bf16Enc, _BothBf16, C.RecordingModels):
            models = make()
            res = E.mpc_plan(models, frames, actions, r, th, noise=noise, cem=cem, seed=3)
            runs.append((models.calls, res))
        assert runs[0][0] == runs[1][0] == runs[2][0] == runs[3][0] and ("encode", b * r) in runs[0][0]
        for key in runs[0][1]:
            assert torch.equal(runs[0][1][key], runs[1][1][key]), key
    # grad= is allowed with a bf16 encoder (the gradient stage never passes through the encoder) ...
    for make in (_Fp32Enc, _Bf16Enc):
        models = make()
        E.mpc_plan(models, frames, actions, r, th, grad=E.GradSettings(iterations=0, rows=2), seed=1)
        assert models.calls
    # ... and still refused with a bf16 forward model, whatever the encoder
    with pytest.raises(ValueError, match=r"(?s)GradSettings\(.*bf16"):
        E.mpc_plan(_BothBf16(), frames, actions, r, th, grad=E.GradSettings(iterations=1, rows=2))
    state, goal = frames[:, 0].contiguous(), frames[:, 1].contiguous()
    calls = []
    for make in (_Fp32Enc, _Bf16Enc):
        models = make()
        goal_code = models.encode(goal)
        del models.calls[:]
        E.plan_step(models, state, goal, goal_code, r, th, noise=noise[:E.plan_step_noise_floats(b, r, th, 2)])
        calls.append(models.calls)
    assert calls[0] == calls[1] and calls[0]
