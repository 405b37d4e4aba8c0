"""CPU-only: the definition of ndp_image_quality restated in numpy against the golden file
(tests/golden/image_quality_case.npz, written by tests/golden/make_golden_image_quality.py), and the argument errors of the
Python layer that need no GPU.  The kernels' own arithmetic on the CPU: tests/test_image_quality_host.py; on the GPU:
tests/test_gpu_image_quality.py."""
import numpy as np
import pytest
import torch

import quality_common as Q


@pytest.fixture(scope="module")
def rec(golden):
    return golden("image_quality_case")


@pytest.fixture(scope="module")
def pairs(rec):
    return Q.golden_pairs(rec)


def test_the_file_holds_the_stated_pairs(rec, pairs):
    assert tuple(p[0] for p in pairs) == Q.NAMES and len(rec["ssim64"]) == len(Q.NAMES)
    by = {name: (a, b) for name, a, b in pairs}
    assert np.array_equal(by["identical"][0], by["identical"][1])
    assert (by["black_white"][0] == 0).all() and (by["black_white"][1] == 255).all()
    assert np.array_equal(by["inverse"][1], 255 - by["inverse"][0])
    for name in ("outside_1", "outside_2"):                      # values leave [-1, 1] on both sides of the pair
        a, b = by[name]
        assert a.dtype == b.dtype == np.float32 and max(a.max(), b.max()) > 1.0 and min(a.min(), b.min()) < -1.0
    assert np.isnan(by["one_nan"][0]).sum() == 1 and not np.isnan(by["one_nan"][1]).any()
    assert float(rec["ssim64"][0]) == 1.0 and np.isinf(rec["psnr64"][0]) and np.isnan(rec["ssim64"][-1])


def test_the_direct_fp64_route_equals_the_scipy_route(rec, pairs):
    for k, (name, a, b) in enumerate(pairs):
        got = Q.ssim_direct(Q.as_unit(a), Q.as_unit(b), np.float64)[0]
        want = float(rec["ssim64"][k])
        if np.isnan(want):
            assert np.isnan(got), name
        else:
            assert abs(got - want) <= 1e-12, (name, got, want)
            assert abs(got - float(rec["ssim64_direct"][k])) <= 1e-13, name
        psnr = Q.psnr64(Q.as_unit(a), Q.as_unit(b))
        wantp = float(rec["psnr64"][k])
        assert (np.isnan(psnr) and np.isnan(wantp)) or psnr == wantp or abs(psnr - wantp) <= 1e-12 * abs(wantp), name


def test_the_fp32_restatement_reproduces_the_stored_distance(rec, pairs):
    worst = 0.0
    for k, (name, a, b) in enumerate(pairs):
        got, s_map = Q.ssim_direct(Q.as_unit(a), Q.as_unit(b), np.float32)
        if name == "one_nan":
            assert np.isnan(got)
            continue
        # numpy's fp32 elementwise operations are IEEE; only the fp64 order of the final mean could differ
        assert abs(got - float(rec["ssim32"][k])) <= 1e-12, (name, got, rec["ssim32"][k])
        worst = max(worst, abs(got - float(rec["ssim64"][k])))
        if name == "identical":
            assert (s_map == 1).all() and got == 1.0             # exact self-similarity of the plain restatement
    assert abs(worst - float(rec["d32"])) <= 1e-12 and 1e-7 < float(rec["d32"]) < 3e-6


def test_scale_clamps_and_keeps_nan():
    x = np.array([-np.inf, -3.0, -1.0, 0.0, 1.0, 3.0, np.inf, np.nan], np.float32)
    u = Q.unit(x)
    assert u[:7].tolist() == [0.0, 0.0, 0.0, 0.5, 1.0, 1.0, 1.0] and np.isnan(u[7])
    # a byte frame and the float image of the same bytes: the same unit image
    frame = np.arange(128 * 128 * 3, dtype=np.int64).reshape(128, 128, 3).astype(np.uint8)
    assert np.array_equal(Q.as_unit(frame), Q.as_unit(Q.as_float(frame)))
    assert abs(float(Q.taps(np.float32).astype(np.float64).sum()) - 1.0) < 1e-7 and Q.taps(np.float32)[5] == Q.taps(np.float32).max()


def test_python_layer_argument_errors_need_no_gpu():
    from ndivplanning_amd import _capi
    from ndivplanning_amd.image_quality import image_quality
    img, frame = torch.zeros(2, 3, 128, 128), torch.zeros(2, 128, 128, 3, dtype=torch.uint8)
    for a, b in ((img, img), (frame, img), (img, frame)):
        with pytest.raises(_capi.NdpError, match="no CPU fallback"):
            image_quality(a, b)
    for bad in (torch.zeros(2, 3, 64, 64), torch.zeros(2, 128, 128, 3), torch.zeros(2, 3, 128, 128, dtype=torch.uint8),
                torch.zeros(2, 3, 128, 128, dtype=torch.int32), torch.zeros(128, 128)):
        with pytest.raises(_capi.NdpError, match="must be"):
            image_quality(bad, img)
        with pytest.raises(_capi.NdpError, match="must be"):
            image_quality(img, bad)
    with pytest.raises(_capi.NdpError, match="nothing to compute"):
        image_quality(img, img, ssim=False, psnr=False)
    with pytest.raises(TypeError):
        image_quality(img.numpy(), img)


def test_evaluations_take_the_keyword_and_default_to_off():
    import inspect
    from ndivplanning_amd import autoencoder_eval, forward_model_eval, train_autoencoder
    for fn in (forward_model_eval.evaluate, forward_model_eval.predict, forward_model_eval.rollout, autoencoder_eval.evaluate):
        assert inspect.signature(fn).parameters["quality"].default is False
    assert inspect.signature(train_autoencoder.train).parameters["val_quality"].default is False
    assert forward_model_eval.make_parser().parse_args(["--model", "m", "--data", "d"]).quality is False
    assert forward_model_eval.make_parser().parse_args(["--model", "m", "--data", "d", "--quality"]).quality is True
    assert autoencoder_eval.make_parser().parse_args(["--encoder", "e", "--decoder", "d", "--data", "x", "--quality"]).quality
    assert train_autoencoder.make_parser().parse_args(["--val-quality"]).val_quality is True
    assert train_autoencoder.make_parser().parse_args([]).val_quality is False
