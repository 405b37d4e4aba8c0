"""GPU: the image encoder's pass with bf16 MFMA operands and bf16 maps (ndp_encoder_forward_lp with NDP_ENC_BF16,
ndp_encoder_pack_params_lp; k_conv_gemm's bf16 path, k_enc_conv1<., true>, k_splitk_reduce<__bf16> in csrc/ndp_encoder.inc) held to
its definition in include/ndp.h, on EO.init_encoder_state(11, bn_seed=12) and EO.synthetic_images at

  n = 1    every deep layer is K-split; conv5 is a 16-row partial tile
  n = 3    odd row counts
  n = 9    conv3 has 18 row tiles: the XCD order with a padded grid and its early return; conv4 has 4.5 tiles
  n = 17   the ragged case of tests/test_gpu_encoder.py

Bounds.  Layer by layer, so that nothing compounds: every stored map (read through ndp_encoder_lp_act_offset) and the
codes against the fp64 restatement of that layer ALONE on the DEVICE's own stored input and the rounded weights
(tests/enc_bf16_common.py).  A bf16 map is compared with bf16(ref64): the share of elements that differ from it at all is
at most twice the share at which bf16(torch's fp32 convolution of the same operands) differs, plus 1e-4; and no element is
further from it than one bf16 ulp of the reference.  That bound is asserted bare, with counted exceptions: the definition
sums in fp32, and where a sum cancels to (almost) nothing the error of ANY fp32 sum exceeds an ulp of the tiny result --
torch's own fp32 convolution on the CPU leaves 1 of conv1's 786,432 elements (n = 3) four of the reference's ulps away,
another of conv3's two.  An element beyond the bare ulp is an exception; every exception must lie within the ulp plus the
error bound of an fp32 sum of THAT element's own terms (enc_bf16_common.fp32_sum_error_bound: (K + 2) 2^-24 (sum |x w| +
|bias|), any order), torch's exceptions are held to the same (which checks the bound itself), and the share of exceptions
is compared with torch's as the issue compares the share of differing elements, of which the exceptions are a part: at
most twice torch's plus 1e-4.  Both counts are printed.  The codes (fp32) fall under the project's adjudication rule:
relative-norm error at most max(2e-5, 2 x that of torch's fp32 convolution of the same rounded operands).
End to end: the codes against the fp64 restatement of the whole pass at most twice the distance of the same restatement
run in fp32 on the CPU, plus 2e-5 (a stored value that lies at a rounding tie falls either way, in any fp32 arithmetic);
and the distance from the UNROUNDED fp64 oracle at most twice the restatement's.

Measured on one MI355X (printed by the tests): see DESIGN.md 5t."""
import os
import sys

import numpy as np
import pytest
import torch

import enc_bf16_common as L
from oracle import encoder_oracle as EO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SIZES = (1, 3, 9, 17)
FP32, BF16 = 0, 1
NEW_LABELS = ("k_enc_conv1_bf16", "k_conv_gemm_bf16[2]", "k_conv_gemm_bf16[3]", "k_conv_gemm_bf16[4]", "k_conv_gemm_bf16[5]",
              "k_conv_gemm_bf16[6]", "k_splitk_reduce_bf16", "k_enc_pack_lp")


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


class _Device:
    """The packed model on the device and the raw entry points."""

    def __init__(self, packed):
        from ndivplanning_amd import _build, _capi
        _build.build()
        self.capi, self.lib = _capi, _capi.load()
        self.params = packed.to(DEV).contiguous()
        self.lp = torch.empty(self.lib.ndp_encoder_lp_weight_bytes(), dtype=torch.uint8, device=DEV)
        self.pack()
        self.ws = {}

    def pack(self):
        p = self.capi.ptr
        self.capi.check(self.lib.ndp_encoder_pack_params_lp(p(self.params), p(self.lp), self.capi.stream_ptr()), "pack_lp")

    def workspace(self, n):
        if n not in self.ws:
            self.ws[n] = torch.empty(self.lib.ndp_encoder_workspace_floats(n), dtype=torch.float32, device=DEV)
        return self.ws[n]

    def forward_lp(self, x, precision, lp="own", codes=None, check=True):
        """x: float [n,3,128,128] or bytes [n,128,128,3] on the device.  Returns (rc, codes)."""
        n, p = int(x.shape[0]), self.capi.ptr
        u8 = x.dtype == torch.uint8
        codes = torch.empty(n, 128, dtype=torch.float32, device=DEV) if codes is None else codes
        rc = self.lib.ndp_encoder_forward_lp(p(self.params), None if u8 else p(x), p(x) if u8 else None, n, precision,
                                             p(self.lp if isinstance(lp, str) else lp), p(codes), p(self.workspace(n)),
                                             self.capi.stream_ptr())
        if check:
            self.capi.check(rc, "ndp_encoder_forward_lp")
        return rc, codes

    def map(self, n, l):
        """The stored bf16 map behind conv l + 1 of the last pass at n <= 512 images: float32 NCHW on the host."""
        side, ch = L.SIDES[l], L.LAYERS[l][1]
        off = self.lib.ndp_encoder_lp_act_offset(l, n)
        m = self.workspace(n).view(torch.bfloat16)[off:off + n * side * side * ch].view(n, side, side, ch)
        return m.float().permute(0, 3, 1, 2).contiguous().cpu()


def _frames(n):
    """n byte frames from the two of tests/golden/frames_case.npz (mirrored, flipped, rolled copies beyond them) and the
    float tensor the reference's loader builds from them."""
    base, _ = L.byte_frames()
    out = []
    for i in range(n):
        f = base[i % 2]
        k = i // 2
        f = f.flip(1) if k & 1 else f
        f = f.flip(0) if k & 2 else f
        out.append(torch.roll(f, shifts=3 * (k // 4), dims=1))
    frames = torch.stack(out).contiguous()
    lut = (torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255) - 0.5) * 2.0
    return frames, lut[frames.long()].permute(0, 3, 1, 2).contiguous()


@pytest.fixture(scope="module")
def case():
    torch.set_num_threads(8)
    state, packed, images = L.model_case(max(SIZES))
    # the references, computed once and left alone
    exact = EO.encoder_forward(state, images, dtype=torch.float64).reshape(-1, 128)
    _, restated = L.restatement(packed, images, torch.float64)
    _, restated32 = L.restatement(packed, images, torch.float32)
    return {"state": state, "packed": packed, "images": images, "dev": _Device(packed), "exact": exact, "restated": restated,
            "restated32": restated32, "runs": {}}


def _run(case, n):
    """One bf16 pass on the first n synthetic images: the codes and the five stored maps, on the host."""
    if n not in case["runs"]:
        dev = case["dev"]
        _, codes = dev.forward_lp(case["images"][:n].contiguous().to(DEV), BF16)
        torch.cuda.synchronize()
        case["runs"][n] = {"codes": codes.cpu(), "maps": [dev.map(n, l) for l in range(5)]}
    return case["runs"][n]


def test_fp32_precision_gives_the_bits_of_ndp_encoder_forward(case):
    dev = case["dev"]
    p = dev.capi.ptr
    for n in SIZES:
        frames, floats = _frames(n)
        for x, fn in ((case["images"][:n].contiguous(), dev.lib.ndp_encoder_forward), (floats, dev.lib.ndp_encoder_forward),
                      (frames, dev.lib.ndp_encoder_forward_u8)):
            x = x.to(DEV)
            want = torch.empty(n, 128, dtype=torch.float32, device=DEV)
            dev.capi.check(fn(p(dev.params), p(x), n, p(want), p(dev.workspace(n)), dev.capi.stream_ptr()), "ndp_encoder_forward")
            _, got = dev.forward_lp(x, FP32, lp=None)                  # lp_weights may be NULL
            _, got2 = dev.forward_lp(x, FP32)
            assert _bits(got) == _bits(want) == _bits(got2), (n, x.dtype)
            _, lp = dev.forward_lp(x, BF16)
            assert _bits(lp) != _bits(want)                            # and bf16 is another computation


@pytest.mark.parametrize("n", SIZES)
def test_every_stored_map_and_the_codes_against_fp64_on_the_devices_own_input(case, n):
    run, packed = _run(case, n), case["packed"]
    report = []
    x = case["images"][:n]
    for l in range(5):
        got = run["maps"][l].double()
        r64 = L.layer_forward(packed, l, x, torch.float64)
        r32 = L.layer_forward(packed, l, x, torch.float32)
        want, torchs = L.round_tensor(r64), L.round_tensor(r32).double()
        assert got.shape == want.shape and torch.isfinite(got).all(), l
        ulp = L.bf16_ulp(r64)
        d = (got - want).abs()
        share, share_torch = float((got != want).double().mean()), float((torchs != want).double().mean())
        d_torch = (torchs - want).abs()
        exc, exc_torch = d > ulp, d_torch > ulp                        # beyond the bare ulp: the counted exceptions
        beyond, beyond_torch = int(exc.sum()), int(exc_torch.sum())
        report.append("conv%d differ %.3g (torch fp32 %.3g), beyond one ulp %d (torch %d) of %d"
                      % (l + 1, share, share_torch, beyond, beyond_torch, got.numel()))
        print("n %d: %s" % (n, report[-1]))
        if beyond or beyond_torch:
            allowed = ulp + L.fp32_sum_error_bound(packed, l, x)
            assert bool((d_torch[exc_torch] <= allowed[exc_torch]).all()), (n, l, "torch's fp32 sum outside the bound of one")
            worst = int((d - allowed).argmax())
            assert bool((d[exc] <= allowed[exc]).all()), (n, l, float(d.view(-1)[worst]), float(ulp.view(-1)[worst]),
                                                          float(allowed.view(-1)[worst]), float(r64.view(-1)[worst]))
        assert beyond / got.numel() <= 2.0 * beyond_torch / got.numel() + 1e-4, (n, l, beyond, beyond_torch, got.numel())
        assert share <= 2.0 * share_torch + 1e-4, (n, l, share, share_torch)
        x = run["maps"][l]                                             # the next layer's input: what the device stored
    r64 = L.layer_forward(packed, 5, x, torch.float64).reshape(n, 128)
    r32 = L.layer_forward(packed, 5, x, torch.float32).reshape(n, 128)
    err, err_torch = L.rel_norm(run["codes"], r64), L.rel_norm(r32, r64)
    print("n %d: codes rel_norm %.3g (torch fp32 %.3g)" % (n, err, err_torch))
    assert torch.isfinite(run["codes"]).all() and err <= max(2e-5, 2.0 * err_torch), (n, err, err_torch)


@pytest.mark.parametrize("n", SIZES)
def test_end_to_end_against_the_restatement_and_the_unrounded_oracle(case, n):
    got = _run(case, n)["codes"].double()
    restated, restated32, exact = case["restated"][:n], case["restated32"][:n], case["exact"][:n]
    mine, ref = L.rel_norm(got, restated), L.rel_norm(restated32, restated)
    far, far_ref = L.rel_norm(got, exact), L.rel_norm(restated, exact)
    print("n %d: codes against the fp64 restatement %.4g (the fp32 restatement on the CPU %.4g); against the unrounded fp64 "
          "oracle %.4g (the fp64 restatement %.4g)" % (n, mine, ref, far, far_ref))
    assert mine <= 2.0 * ref + 2e-5, (n, mine, ref)
    assert far_ref > 0 and far <= 2.0 * far_ref, (n, far, far_ref)


def test_two_runs_and_byte_and_float_frames_give_identical_bits(case):
    dev = case["dev"]
    for n in SIZES:
        first = _run(case, n)
        _, again = dev.forward_lp(case["images"][:n].contiguous().to(DEV), BF16)
        torch.cuda.synchronize()
        assert _bits(again) == _bits(first["codes"]), n
        assert all(_bits(dev.map(n, l)) == _bits(first["maps"][l]) for l in range(5)), n
        frames, floats = _frames(n)
        _, from_bytes = dev.forward_lp(frames.to(DEV), BF16)
        torch.cuda.synchronize()
        maps_b = [dev.map(n, l) for l in range(5)]
        _, from_floats = dev.forward_lp(floats.to(DEV), BF16)
        torch.cuda.synchronize()
        assert _bits(from_bytes) == _bits(from_floats) and bool(torch.isfinite(from_bytes).all()), n
        assert all(_bits(dev.map(n, l)) == _bits(maps_b[l]) for l in range(5)), n


def test_a_nan_pixel_gives_nan_codes_for_that_image_only(case):
    dev, n = case["dev"], 3
    x = case["images"][:n].clone()
    x[1, 2, 77, 5] = float("nan")
    _, got = dev.forward_lp(x.to(DEV), BF16)
    got, clean = got.cpu(), _run(case, n)["codes"]
    assert torch.isnan(got[1]).any() and not torch.isnan(got[0]).any() and not torch.isnan(got[2]).any()
    assert _bits(got[0]) == _bits(clean[0]) and _bits(got[2]) == _bits(clean[2])


def test_513_images_are_a_pass_of_512_and_a_pass_of_one(case):
    """The pass boundary without a 513-image oracle: byte frames (a quarter of the upload), every one different."""
    dev = case["dev"]
    gen = torch.Generator().manual_seed(5)
    frames = torch.randint(0, 256, (513, 128, 128, 3), generator=gen, dtype=torch.uint8).to(DEV)
    _, whole = dev.forward_lp(frames, BF16)
    _, head = dev.forward_lp(frames[:512].contiguous(), BF16)
    _, tail = dev.forward_lp(frames[512:].contiguous(), BF16)
    assert bool(torch.isfinite(whole).all())
    assert _bits(whole[:512]) == _bits(head) and _bits(whole[512:]) == _bits(tail)
    assert _bits(whole[0]) != _bits(whole[512])


def _timed(dev, fn):
    dev.capi.timing_enable(True)
    try:
        result = fn()
        torch.cuda.synchronize()
        seen = dev.capi.timing_collect()
    finally:
        dev.capi.timing_enable(False)
    return result, {k: v[1] for k, v in seen.items()}


def test_refused_arguments_launch_nothing(case):
    dev, n = case["dev"], 3
    p = dev.capi.ptr
    x = case["images"][:n].contiguous().to(DEV)
    xb = _frames(n)[0].to(DEV)
    ws = dev.workspace(n)
    codes = torch.full((n, 128), -7.0, device=DEV)
    lp_copy = dev.lp.clone()

    def refused():
        lib, st = dev.lib, dev.capi.stream_ptr()
        odd = lambda t: dev.capi.c_void_p(t.data_ptr() + 4)            # noqa: E731
        full = dict(params=p(dev.params), x=p(x), xb=None, n=n, prec=BF16, lp=p(dev.lp), codes=p(codes), ws=p(ws))
        rcs = []
        for over in ({"prec": 2}, {"prec": -1}, {"prec": 7, "lp": None}, {"lp": None}, {"xb": p(xb)}, {"x": None}, {"n": 0},
                     {"lp": odd(dev.lp)}, {"ws": odd(ws)}, {"codes": odd(codes)}, {"x": odd(x)}, {"params": odd(dev.params)},
                     {"params": None}, {"codes": None}, {"ws": None}, {"prec": FP32, "xb": p(xb)}, {"prec": FP32, "x": None}):
            k = dict(full, **over)
            rcs.append(lib.ndp_encoder_forward_lp(k["params"], k["x"], k["xb"], k["n"], k["prec"], k["lp"], k["codes"], k["ws"], st))
            assert b"ndp_encoder_forward_lp" in lib.ndp_last_error(), over
        rcs.append(lib.ndp_encoder_pack_params_lp(p(dev.params), None, st))
        rcs.append(lib.ndp_encoder_pack_params_lp(None, p(dev.lp), st))
        rcs.append(lib.ndp_encoder_pack_params_lp(p(dev.params), odd(dev.lp), st))
        return rcs

    rcs, counts = _timed(dev, refused)
    assert rcs == [1] * len(rcs) and counts == {}, (rcs, counts)
    assert bool((codes == -7.0).all()) and _bits(dev.lp) == _bits(lp_copy)


def test_the_bf16_weights_are_the_rounded_packed_weights_in_the_packed_order(case):
    dev, packed = case["dev"], case["packed"]
    lp = dev.lp.view(torch.bfloat16).float().cpu()
    assert lp.numel() == L.LP_WEIGHT_VALUES
    o = po = 0
    for l, (cin, cout, k, _, _) in enumerate(L.LAYERS):
        nw = cout * k * k * cin
        if l >= 1:
            assert torch.equal(lp[o:o + nw], L.round_tensor(packed[po:po + nw])), l
            o += nw
        po += nw + cout


def test_a_bf16_pass_shows_the_new_labels_and_an_fp32_pass_none_of_them(case):
    dev = case["dev"]
    for n in (1, 17):
        x = case["images"][:n].contiguous().to(DEV)
        dev.workspace(n)
        _, counts = _timed(dev, lambda: dev.forward_lp(x, BF16))
        print(n, sorted(counts.items()))
        assert counts["k_enc_conv1_bf16"] == 1 and all(counts.get("k_conv_gemm_bf16[%d]" % i) == 1 for i in range(2, 7)), counts
        assert not [k for k in counts if k.startswith("k_conv_gemm[") or k == "k_enc_conv1"], counts
        assert set(counts) <= set(NEW_LABELS) | {"k_splitk_reduce"}, counts          # (conv6's reduction keeps the fp32 kernel)
        assert counts.get("k_splitk_reduce", 0) == 1                                 # conv6 is split at both sizes
        if n == 1:
            assert counts.get("k_splitk_reduce_bf16") == 4, counts                    # conv2..conv5 are all split at one image
        _, fp32 = _timed(dev, lambda: dev.forward_lp(x, FP32))
        assert not set(fp32) & set(NEW_LABELS) and fp32["k_enc_conv1"] == 1 and fp32["k_conv_gemm[2]"] == 1, fp32
    _, pack = _timed(dev, dev.pack)
    assert pack == {"k_enc_pack_lp": 1}                                # one launch


# ------------------------------------------------------------------------------------------------ the Python surface
@pytest.fixture(scope="module")
def planner():
    from test_gpu_eval import _modules
    from ndivplanning_amd import evaluation as E
    enc, fm, gen = _modules()
    return E, (enc, fm, gen), E.EvalModels(enc, fm, gen, DEV, enc_precision="bf16"), E.EvalModels(enc, fm, gen, DEV)


def test_evalmodels_encode_is_the_direct_call(planner):
    E, (enc, _, _), models, models32 = planner
    from ndivplanning_amd import _capi
    from ndivplanning_amd.models.image_autoencoder import pack_encoder_params
    assert models.enc_precision == "bf16" and models32.enc_precision == "fp32" and models32._enc_lp is None
    x = EO.synthetic_images(31, 5).to(DEV)
    dev = _Device(pack_encoder_params(enc).detach().cpu())
    _, want = dev.forward_lp(x, BF16)
    got = models.encode(x)
    assert _bits(got) == _bits(want)
    _, want32 = dev.forward_lp(x, FP32)
    assert _bits(models32.encode(x)) == _bits(want32) != _bits(want)
    with torch.no_grad():
        assert _bits(models32.encode(x)) == _bits(enc(x).reshape(5, 128))            # the default path: the module's own bits
    _capi.timing_enable(True)
    models.encode(x)
    torch.cuda.synchronize()
    names = set(_capi.timing_collect())
    _capi.timing_enable(False)
    assert "k_conv_gemm_bf16[2]" in names and "k_enc_pack_lp" not in names           # packed once, at construction


def test_plan_step_is_the_chain_by_hand_and_grad_runs_with_a_bf16_encoder(planner):
    E, (enc, fm, gen), models, models32 = planner
    from test_gpu_eval import _mpc_inputs
    b, r, th = 1, 4, 2
    frames, _ = _mpc_inputs(b, 3)
    imgs = models.images(frames.view(-1, *frames.shape[2:])).view(b, 3, 3, 128, 128)
    state, goal = imgs[:, 0].contiguous(), imgs[:, 2].contiguous()
    nz = models.noise_dim
    noise = torch.rand(E.plan_step_noise_floats(b, r, th, nz), generator=torch.Generator().manual_seed(6)).to(DEV)
    goal_code = models.encode(goal)                                    # the goal code comes from the same precision
    assert _bits(goal_code) != _bits(models32.encode(goal))
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
    assert _bits(err) == _bits(by_hand) and _bits(actions0) == _bits(first)
    _, _, err32, _ = E.plan_step(models32, state, goal, models32.encode(goal), r, th, noise=noise)
    # (this model's actions hang on the noise far more than on the codes: the fp32 encoder's errors may even be the same bits)
    assert torch.allclose(err32, err, rtol=0.05)
    # both precisions together, and the gradient stage with a bf16 encoder and an fp32 forward model
    both = E.EvalModels(enc, fm, gen, DEV, fm_precision="bf16", enc_precision="bf16")
    out = E.plan_step(both, state, goal, both.encode(goal), r, th, noise=noise)
    assert _bits(both.encode(goal)) == _bits(goal_code) and bool(torch.isfinite(out[2]).all())
    out = E.plan_step(models, state, goal, goal_code, r, th, noise=noise, grad=E.GradSettings(iterations=1, rows=2))
    assert bool(torch.isfinite(out[2]).all()) and out[3].shape == (b, r, 4)
    with pytest.raises(ValueError, match=r"(?s)GradSettings\(.*bf16"):
        E.plan_step(both, state, goal, goal_code, r, th, noise=noise, grad=E.GradSettings(iterations=1, rows=2))


def test_the_mpc_eval_command_line_takes_the_precision(planner, tmp_path, capsys, monkeypatch):
    import yaml
    E, (enc, fm, gen), _, _ = planner
    from ndivplanning_amd import mpc_eval
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
    for flag in ((), ("--enc-precision", "bf16"), ("--enc-precision", "fp32")):
        capsys.readouterr()
        result = mpc_eval.main(["--config-file", str(yml)] + list(flag))
        text = capsys.readouterr().out
        last = [ln for ln in text.splitlines() if ln.startswith("avg_action_error, avg_image_loss:")]
        assert len(last) == 1 and all(np.isfinite(result)), text
        outs[flag] = result
    assert outs[()] == outs[("--enc-precision", "fp32")] and outs[()] != outs[("--enc-precision", "bf16")]
    cfg["evaluation"]["enc_precision"] = "bf16"                         # the config key, without the flag
    yml.write_text(yaml.safe_dump(cfg))
    assert mpc_eval.main(["--config-file", str(yml)]) == outs[("--enc-precision", "bf16")]
    cfg["evaluation"]["enc_precision"] = "fp16"
    yml.write_text(yaml.safe_dump(cfg))
    with pytest.raises(ValueError, match="'fp32' or 'bf16'"):
        mpc_eval.main(["--config-file", str(yml)])
    for m in (enc, fm, gen):                                           # (the fixture's modules live on the device)
        m.to(DEV)
