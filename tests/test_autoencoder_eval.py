"""CPU-only: the eval-mode image autoencoder's host side -- the fixture from the reference's modules is reproduced by the
mirror's PyTorch forward, the BatchNorm fold is exact, the folded vector and its cache behave, the CLI parses.  The
kernels themselves are tested in tests/test_gpu_autoencoder_eval.py."""
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "autoencoder_eval_case.npz")


def recipe():
    """tests/golden/make_golden_autoencoder_eval.py as a module: the fixture's recipe (build_modules, images, codes)."""
    spec = importlib.util.spec_from_file_location(
        "make_golden_autoencoder_eval", os.path.join(ROOT, "tests", "golden", "make_golden_autoencoder_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _sums(t):
    t = t.detach().double()
    return np.array([t.sum().item(), t.abs().sum().item(), (t * t).sum().item()])


def build_checked():
    """(recipe module, fixture, encoder, decoder): the fixture's state through the mirror's classes, checksums checked."""
    from ndivplanning_amd.models.image_autoencoder import Decoder, Encoder
    mk, g = recipe(), np.load(GOLDEN)
    assert (int(g["seed"]), int(g["bn_seed"]), int(g["data_seed"]), int(g["code_seed"]), int(g["n"])) == \
        (mk.SEED, mk.BN_SEED, mk.DATA_SEED, mk.CODE_SEED, mk.N) and float(g["weight_std"]) == mk.WEIGHT_STD
    enc, dec = mk.build_modules(Encoder, Decoder)
    for pre, m in (("encoder.", enc), ("decoder.", dec)):
        for k, v in m.state_dict().items():
            if v.is_floating_point():
                np.testing.assert_allclose(_sums(v), g["state/" + pre + k], rtol=1e-6, atol=1e-6, err_msg=pre + k)
    return mk, g, enc, dec


def test_fixture_is_meaningful():
    g = np.load(GOLDEN)
    assert 0.2 <= g["out_std"].min() and g["out_std"].max() <= 0.8        # tanh, the bytes and the error away from zero
    assert len(set(g["decode_u8"].tolist())) > 20 and len(set(g["recon_u8"].tolist())) > 20


def test_forward_torch_reproduces_reference_fixture():
    mk, g, enc, dec = build_checked()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    x, z = mk.images(), mk.codes()
    np.testing.assert_array_equal(z.reshape(-1, 128).numpy(), g["codes"])
    with torch.no_grad():
        out = dec._forward_torch(z)
        rec = dec._forward_torch(enc._forward_torch(x))
        assert torch.equal(dec(z), out)                                     # a CPU tensor keeps the PyTorch forward
    idx = g["sample_idx"]
    np.testing.assert_allclose(out.reshape(-1)[idx].double().numpy(), g["decode"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(rec.reshape(-1)[idx].double().numpy(), g["recon"], rtol=0, atol=1e-6)
    err = ((rec.double() - x.double()) ** 2).reshape(mk.N, -1).mean(dim=1)
    np.testing.assert_allclose(err.numpy(), g["mse"], rtol=1e-6)
    np.testing.assert_allclose(err.mean().item(), float(g["mean_mse"]), rtol=1e-6)
    assert np.abs(mk.denorm_bytes(out).reshape(-1)[idx].astype(int) - g["decode_u8"].astype(int)).max() <= 1


def test_fold_equals_batchnorm_in_fp64():
    """relu(conv_transpose2d(x, w', b')) == relu(bn(deconv(x))) through all five layers, to 1e-12 relative."""
    from ndivplanning_amd.models.image_autoencoder import fold_decoder_layers
    mk, g, enc, dec = build_checked()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dec = dec.double()
    folded = fold_decoder_layers(dec, torch.float64)
    assert len(folded) == 6 and torch.equal(folded[5][0], dec.deconv6.weight) and torch.equal(folded[5][1], dec.deconv6.bias)
    a = b = mk.codes().double()
    with torch.no_grad():
        for i in range(1, 6):
            deconv, (w, bias) = getattr(dec, "deconv%d" % i), folded[i - 1]
            a = F.relu(getattr(dec, "deconv%d_bn" % i)(deconv(a)))
            b = F.relu(F.conv_transpose2d(b, w, bias, stride=deconv.stride, padding=deconv.padding))
            assert (a - b).abs().max().item() <= 1e-12 * a.abs().max().item(), i
        assert a.abs().max().item() > 0.1


def test_fold_decoder_params_fp32_vs_fp64():
    """The flat fp32 vector holds fold_decoder_layers' values at the layout's positions; each differs from the fp64 fold
    by fp32 rounding: the fold is a division, a square root, two products and two sums -- a few ulp of the operands."""
    from ndivplanning_amd import _build, _capi
    from ndivplanning_amd.models import image_autoencoder as IA
    _build.build()
    lib = _capi.load()
    _, _, _, dec = build_checked()
    flat = IA.fold_decoder_params(dec)
    assert flat.dtype == torch.float32 and flat.numel() == lib.ndp_ae_decoder_param_floats()
    want = IA.fold_decoder_layers(dec.double(), torch.float64)
    dec.float()
    cover = np.zeros(flat.numel(), dtype=np.int32)
    eps32 = 2.0 ** -24
    for i, (w, b) in enumerate(want):
        off, d = IA._DEC_FLAT.layout(0, i)
        cover[off:off + d[0] * d[1] * d[2]] += 1
        assert d[3] == 1 and (d[4], d[5]) == (w.shape[0], w.shape[1]) and d[1] == 16
        got = flat[off:off + d[0] * d[1] * d[2]].view(d[0], 4, 4, d[2])
        assert torch.count_nonzero(got[:, :, :, w.shape[1]:]) == 0          # (deconv6's padded output channel)
        got = got[: w.shape[0], :, :, : w.shape[1]].permute(0, 3, 1, 2).double()
        assert ((got - w).abs() <= 4 * eps32 * w.abs() + 1e-30).all(), i
        boff, bd = IA._DEC_FLAT.layout(1, i)
        cover[boff:boff + bd[0]] += 1
        gb = flat[boff:boff + b.numel()].double()
        # (b - mean) * scale + beta: absolute in the magnitudes of its terms
        assert ((gb - b).abs() <= 8 * eps32 * (b.abs() + 2.0)).all(), i
    assert (cover == 1).all()
    import ctypes
    off, dims = ctypes.c_int64(), (ctypes.c_int64 * 6)()
    assert lib.ndp_ae_decoder_layout(2, 0, ctypes.byref(off), dims) == 1    # no BatchNorm in this network: NDP_E_ARG
    assert lib.ndp_ae_decoder_layout(0, 6, ctypes.byref(off), dims) == 1
    # the training network's layout is untouched: its decoder layers have the same shapes
    for i in range(6):
        assert IA._DEC_FLAT.layout(0, i)[1] == IA.ae_layout(lib, 0, 6 + i)[1]


def test_state_key_sees_in_place_changes():
    from ndivplanning_amd.models import image_autoencoder as IA
    dec = IA.Decoder().eval()
    k0 = IA._decoder_state_key(dec)
    assert IA._decoder_state_key(dec) == k0
    with torch.no_grad():
        dec.deconv3.weight.mul_(1.5)
    k1 = IA._decoder_state_key(dec)
    assert k1 != k0
    dec.deconv2_bn.running_var.add_(0.25)
    k2 = IA._decoder_state_key(dec)
    assert k2 != k1
    dec.deconv5_bn.running_mean.zero_()
    assert IA._decoder_state_key(dec) != k2


def test_pickle_drops_kernel_scratch():
    import pickle
    from ndivplanning_amd.models import image_autoencoder as IA
    dec = IA.Decoder().eval()
    dec.__dict__["_ndp_packed"] = ("key", torch.zeros(3))
    dec.__dict__["_ndp_ws"] = torch.zeros(5)
    back = pickle.loads(pickle.dumps(dec))
    assert "_ndp_packed" not in back.__dict__ and "_ndp_ws" not in back.__dict__
    assert "_ndp_ws" in dec.__dict__                                        # (the live module keeps its scratch)
    assert torch.equal(back.deconv1.weight, dec.deconv1.weight)


def test_cpu_tensors_raise():
    from ndivplanning_amd import _capi, autoencoder_eval as AE
    from ndivplanning_amd.models import image_autoencoder as IA
    enc, dec = IA.Encoder().eval(), IA.Decoder().eval()
    with pytest.raises(_capi.NdpError):
        AE.decode(dec, torch.zeros(1, 128))
    with pytest.raises(_capi.NdpError):
        AE.reconstruct(enc, dec, torch.zeros(1, 3, 128, 128))
    with pytest.raises(_capi.NdpError):
        AE.reconstruct(enc, dec, torch.zeros(1, 128, 128, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        AE.decode(dec, torch.zeros(1, 128), out="png")
    # the module itself keeps the PyTorch forward on the CPU
    with torch.no_grad():
        assert dec(torch.zeros(1, 128, 1, 1)).shape == (1, 3, 128, 128)


def test_cli_parsing():
    from ndivplanning_amd import autoencoder_eval as AE, train_autoencoder as T
    args = AE.make_parser().parse_args(["--encoder", "e.pt", "--decoder", "d.pt", "--data", "synthetic:2:jpeg"])
    assert (args.encoder, args.decoder, args.data, args.save_dir, args.batch_size, args.num_save) == \
        ("e.pt", "d.pt", "synthetic:2:jpeg", None, 16, 8)
    args = AE.make_parser().parse_args(["--encoder", "e", "--decoder", "d", "--data", "x", "--save-dir", "out", "--num-save", "3",
                                        "--batch-size", "4", "--raw-jpeg"])
    assert (args.save_dir, args.num_save, args.batch_size, args.raw_jpeg) == ("out", 3, 4, True)
    with pytest.raises(SystemExit):
        AE.make_parser().parse_args(["--encoder", "e.pt"])
    args = T.make_parser().parse_args([])
    assert args.val_data is None and args.val_every == 1
    args = T.make_parser().parse_args(["--val-data", "synthetic:2:images", "--val-every", "5"])
    assert (args.val_data, args.val_every) == ("synthetic:2:images", 5)


def test_train_validation_arguments(monkeypatch):
    from ndivplanning_amd import train_autoencoder as T
    sig = inspect.signature(T.train)
    assert sig.parameters["val_data"].default is None and sig.parameters["val_every"].default == 1
    with pytest.raises(ValueError):                                         # (before any GPU is touched)
        T.train("synthetic:2:images", val_data="synthetic:2:images", val_every=0, device="cpu")
    seen = {}
    monkeypatch.setattr(T, "train", lambda *a, **kw: seen.update(kw, data=a[0]))
    T.main(["--data", "synthetic:4:images", "--val-data", "synthetic:2:images", "--val-every", "3"])
    assert (seen["data"], seen["val_data"], seen["val_every"]) == ("synthetic:4:images", "synthetic:2:images", 3)
    T.main([])
    assert seen["val_data"] is None and seen["val_every"] == 1


def test_save_pairs_writes_png(tmp_path):
    from PIL import Image
    from ndivplanning_amd import autoencoder_eval as AE
    a = torch.arange(2 * 128 * 128 * 3, dtype=torch.int64).remainder(251).to(torch.uint8).view(2, 128, 128, 3)
    paths = AE.save_pairs(a, 255 - a, str(tmp_path / "pairs"))
    assert [os.path.basename(p) for p in paths] == ["input_000.png", "recon_000.png", "input_001.png", "recon_001.png"]
    np.testing.assert_array_equal(np.array(Image.open(paths[3])), (255 - a[1]).numpy())
