"""GPU: the eval-mode image Decoder and the reconstruction error on the gfx950 kernels (ndp_ae_decode, csrc/
ndp_autoencoder.inc) against the fixture made from the reference's modules and against an fp64 torch-CPU evaluation of
the same module, under the project's adjudication rule:
    |hip - fp64| <= max(1e-5, 4 * |fp32 torch-CPU - fp64|)   elementwise.
Batch sizes 1, 2, 3, 17 and one pass + 1: k_fm_rows_cls (n * 16 <= 64 rows), split-K at small n, both sides of the
16-image k_fm_deconv32 switch, an odd count, one pass boundary."""
import io
import os
import pickle

import numpy as np
import pytest
import torch

from test_autoencoder_eval import build_checked

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_ORACLE = 17


@pytest.fixture(scope="module")
def case():
    """The fixture's modules on the GPU (eval mode), 17 seeded codes (the fixture's two first) and the decoder's output
    for them from torch on the CPU in fp64 and fp32 -- computed once, shared, never written to."""
    from ndivplanning_amd import _build
    _build.build()
    mk, g, enc, dec = build_checked()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    codes = torch.cat([mk.codes().reshape(-1, 128),
                       torch.randn(N_ORACLE - mk.N, 128, generator=torch.Generator().manual_seed(11))])
    with torch.no_grad():
        f32 = dec._forward_torch(codes.view(-1, 128, 1, 1))
        dec.double()
        f64 = dec._forward_torch(codes.double().view(-1, 128, 1, 1))
        dec.float()
    bound = torch.clamp(4 * (f32.double() - f64).abs(), min=1e-5)
    return {"mk": mk, "g": g, "enc": enc.to(DEV).eval(), "dec": dec.to(DEV).eval(), "codes": codes.to(DEV),
            "f64": f64.to(DEV), "bound": bound.to(DEV), "images": mk.images().to(DEV)}


def _within(got, idx, case):
    err = (got.double() - case["f64"][idx]).abs()
    worst = (err / case["bound"][idx]).max().item()
    print("n=%d max |hip - fp64| = %.3e, worst error / bound = %.3f" % (got.shape[0], err.max().item(), worst))
    return worst <= 1.0


def raw_decode(dec, codes, f32=True, u8=False, target=None, sq=True, mean=True):
    """One ndp_ae_decode call with any combination of outputs: (rc, recon_f32, recon_u8, sq_err, mean_err); every
    output starts as a sentinel, so that a call that must launch nothing can be seen to have written nothing."""
    from ndivplanning_amd import _capi
    from ndivplanning_amd.models import image_autoencoder as IA
    lib = _capi.load()
    n = codes.shape[0]
    params, ws = IA._decoder_packed(dec, codes.device, n)
    rf = torch.full((n, 3, 128, 128), 7.0, device=DEV) if f32 else None
    ru = torch.full((n, 128, 128, 3), 77, device=DEV, dtype=torch.uint8) if u8 else None
    sq_t = torch.full((n,), -1.0, device=DEV) if sq else None
    mean_t = torch.full((1,), -1.0, device=DEV) if mean else None
    tf = target if target is not None and target.dtype == torch.float32 else None
    tu = target if target is not None and target.dtype == torch.uint8 else None
    p = _capi.ptr
    rc = lib.ndp_ae_decode(p(params), p(codes.contiguous()), n, p(rf), p(ru), p(tf), p(tu), p(sq_t), p(mean_t), p(ws),
                           _capi.stream_ptr())
    torch.cuda.synchronize()
    return rc, rf, ru, sq_t, mean_t


def loader_floats(frames_u8):
    """utils/hdf5_load.py:9-11 on byte frames [n,128,128,3] -> float NCHW, computed where the loader computes it (CPU)."""
    return ((frames_u8.cpu().permute(0, 3, 1, 2).to(torch.float32).div(255) - 0.5) * 2.0).contiguous().to(DEV)


def to_hwc_bytes(recon_f32):
    return (((recon_f32 + 1) / 2) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def test_decode_matches_reference_fixture(case):
    from ndivplanning_amd import autoencoder_eval as AE
    g, idx = case["g"], torch.from_numpy(case["g"]["sample_idx"]).to(DEV)
    z = case["codes"][:2]
    out = AE.decode(case["dec"], z)
    assert out.shape == (2, 3, 128, 128) and out.dtype == torch.float32
    assert _within(out, slice(0, 2), case)
    got = out.reshape(-1)[idx].double().cpu().numpy()
    ref = g["decode"]
    f64 = case["f64"][:2].reshape(-1)[idx].cpu().numpy()
    assert (np.abs(got - f64) <= np.maximum(1e-5, 4 * np.abs(ref - f64))).all()     # the reference's own fp32 as the arbiter
    # bytes: the same call's float output, bit for bit; the reference's bytes at the sample positions within 1
    b = AE.decode(case["dec"], z, out="bytes")
    assert b.shape == (2, 128, 128, 3) and b.dtype == torch.uint8
    assert torch.equal(b, to_hwc_bytes(out))
    got_u8 = b.permute(0, 3, 1, 2).reshape(-1)[idx].cpu().numpy().astype(int)
    assert np.abs(got_u8 - g["decode_u8"].astype(int)).max() <= 1


@pytest.mark.parametrize("n", [1, 3, 17])
def test_decode_against_fp64_oracle(case, n):
    from ndivplanning_amd import autoencoder_eval as AE
    out = AE.decode(case["dec"], case["codes"][:n].view(n, 128, 1, 1))
    assert _within(out, slice(0, n), case)


def test_decode_across_a_pass_boundary(case):
    from ndivplanning_amd import _capi, autoencoder_eval as AE
    lib = _capi.load()
    n = int(lib.ndp_ae_decode_pass_images()) + 1
    assert lib.ndp_ae_decode_workspace_floats(n) == lib.ndp_ae_decode_workspace_floats(n - 1)   # bounded by the pass
    assert lib.ndp_ae_decode_workspace_floats(0) == 0
    which = torch.arange(n, device=DEV) % N_ORACLE
    out = AE.decode(case["dec"], case["codes"][which])
    err = (out.double() - case["f64"][which]).abs()
    worst = (err / case["bound"][which]).reshape(n, -1).max(dim=1).values
    print("pass boundary: worst error / bound %.3f (image %d)" % (worst.max().item(), int(worst.argmax())))
    assert (worst <= 1.0).all()
    # the image behind the boundary (a pass of one: k_fm_rows_cls, mode-1 deconv5) and the bytes of the whole batch
    b = AE.decode(case["dec"], case["codes"][which], out="bytes")
    assert torch.equal(b, to_hwc_bytes(out))


@pytest.mark.parametrize("n", [3, 17])
def test_bytes_and_floats_of_one_call(case, n):
    rc, rf, ru, _, _ = raw_decode(case["dec"], case["codes"][:n], f32=True, u8=True, sq=False, mean=False)
    assert rc == 0
    assert _within(rf, slice(0, n), case)
    assert torch.equal(ru, to_hwc_bytes(rf))
    assert ru.min().item() < 40 and ru.max().item() > 215                  # (not a constant image)


def _check_errors(rf, target_f32, sq, mean):
    n = rf.shape[0]
    want = ((rf.double() - target_f32.double()) ** 2).reshape(n, -1).mean(dim=1)
    rel = ((sq.double() - want).abs() / want).max().item()
    rel_mean = abs(mean.double().item() - sq.double().mean().item()) / sq.double().mean().item()
    print("n=%d per-image MSE rel %.3e (bound 1e-5), mean rel %.3e (bound 1e-6)" % (n, rel, rel_mean))
    # fp32 sums in the stated order: 3 per thread + 8 levels of the workgroup's tree + 64 partial sums: 75 * 2^-24 = 4.5e-6
    assert rel <= 1e-5
    assert rel_mean <= 1e-6


@pytest.mark.parametrize("n", [1, 2, 17])
def test_errors_float_and_byte_targets(case, n):
    gen = torch.Generator().manual_seed(21)
    frames = torch.randint(0, 256, (n, 128, 128, 3), generator=gen, dtype=torch.uint8).to(DEV)
    target = loader_floats(frames)
    z = case["codes"][:n]
    rc, rf, _, sq, mean = raw_decode(case["dec"], z, target=target)
    assert rc == 0
    _check_errors(rf, target, sq, mean)
    # the byte frames the floats were made from: the same bits
    rc, rf_u, _, sq_u, mean_u = raw_decode(case["dec"], z, target=frames)
    assert rc == 0 and torch.equal(rf_u, rf) and torch.equal(sq_u, sq) and torch.equal(mean_u, mean)
    # a second run: the same bits; errors alone (no reconstruction kept): the same bits
    rc, rf2, _, sq2, mean2 = raw_decode(case["dec"], z, target=target)
    assert rc == 0 and torch.equal(rf2, rf) and torch.equal(sq2, sq) and torch.equal(mean2, mean)
    rc, _, _, sq3, mean3 = raw_decode(case["dec"], z, f32=False, target=frames)
    assert rc == 0 and torch.equal(sq3, sq) and torch.equal(mean3, mean)
    rc, _, _, _, mean4 = raw_decode(case["dec"], z, f32=False, target=frames, sq=False)
    assert rc == 0 and torch.equal(mean4, mean)


def test_errors_across_a_pass_boundary(case):
    from ndivplanning_amd import _capi
    n = int(_capi.load().ndp_ae_decode_pass_images()) + 1
    which = torch.arange(n, device=DEV) % N_ORACLE
    gen = torch.Generator().manual_seed(22)
    frames = torch.randint(0, 256, (n, 128, 128, 3), generator=gen, dtype=torch.uint8).to(DEV)
    rc, rf, _, sq, mean = raw_decode(case["dec"], case["codes"][which], target=frames)
    assert rc == 0
    _check_errors(rf, loader_floats(frames), sq, mean)
    rc, rf2, _, sq2, mean2 = raw_decode(case["dec"], case["codes"][which], target=frames)
    assert torch.equal(rf2, rf) and torch.equal(sq2, sq) and torch.equal(mean2, mean)


def test_bad_arguments_launch_nothing(case):
    from ndivplanning_amd import _capi
    lib = _capi.load()
    z = case["codes"][:2]
    target = torch.zeros(2, 3, 128, 128, device=DEV)
    for kw in ({"sq": True, "mean": False}, {"sq": False, "mean": True}, {"sq": True, "mean": True}):
        rc, rf, _, sq, mean = raw_decode(case["dec"], z, target=None, **kw)
        assert rc == 1 and b"target" in lib.ndp_last_error()                # NDP_E_ARG
        assert (rf == 7.0).all() and (sq is None or (sq == -1.0).all()) and (mean is None or (mean == -1.0).all())
    # two targets, no output, no image
    from ndivplanning_amd.models import image_autoencoder as IA
    params, ws = IA._decoder_packed(case["dec"], z.device, 2)
    p = _capi.ptr
    frames = torch.zeros(2, 128, 128, 3, device=DEV, dtype=torch.uint8)
    out = torch.full((2, 3, 128, 128), 7.0, device=DEV)
    st = _capi.stream_ptr()
    assert lib.ndp_ae_decode(p(params), p(z), 2, p(out), None, p(target), p(frames), None, None, p(ws), st) == 1
    assert lib.ndp_ae_decode(p(params), p(z), 2, None, None, None, None, None, None, p(ws), st) == 1
    assert lib.ndp_ae_decode(p(params), p(z), 0, p(out), None, None, None, None, None, p(ws), st) == 1
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def test_reconstruct_is_decode_of_encode(case):
    from ndivplanning_amd import autoencoder_eval as AE
    enc, dec, x = case["enc"], case["dec"], case["images"]
    g, idx = case["g"], torch.from_numpy(case["g"]["sample_idx"]).to(DEV)
    with torch.no_grad():
        z = enc(x)
    recon, sq, mean = AE.reconstruct(enc, dec, x)
    assert torch.equal(recon, AE.decode(dec, z))
    rb, sq_b, mean_b = AE.reconstruct(enc, dec, x, out="bytes")
    assert torch.equal(rb, AE.decode(dec, z, out="bytes")) and torch.equal(sq_b, sq) and torch.equal(mean_b, mean)
    r2, none1, none2 = AE.reconstruct(enc, dec, x, errors=False)
    assert torch.equal(r2, recon) and none1 is None and none2 is None
    # against the reference (two networks deep, the encoder's rounding passes through the decoder): its bytes within 1
    # at the sample positions; its errors under the adjudication rule with a relative floor, the fp64 value from the
    # same modules on the CPU
    print("reconstruction samples: max |hip - reference| = %.3e"
          % np.abs(recon.reshape(-1)[idx].double().cpu().numpy() - g["recon"]).max())
    got_u8 = rb.permute(0, 3, 1, 2).reshape(-1)[idx].cpu().numpy().astype(int)
    assert np.abs(got_u8 - g["recon_u8"].astype(int)).max() <= 1
    enc64, dec64 = (pickle.loads(pickle.dumps(m)).cpu().double() for m in (enc, dec))
    with torch.no_grad():
        x64 = x.cpu().double()
        mse64 = ((dec64._forward_torch(enc64._forward_torch(x64)) - x64) ** 2).reshape(2, -1).mean(dim=1).numpy()
    got = sq.double().cpu().numpy()
    print("per-image MSE: hip", got, "fp64", mse64, "reference", g["mse"])
    assert (np.abs(got - mse64) <= np.maximum(1e-5 * mse64, 4 * np.abs(g["mse"] - mse64))).all()
    _check_errors(recon, x, sq, mean)
    # byte frames: reconstruct == decode(encoder(frames)), the error against the frames' own floats
    gen = torch.Generator().manual_seed(23)
    frames = torch.randint(0, 256, (3, 128, 128, 3), generator=gen, dtype=torch.uint8).to(DEV)
    with torch.no_grad():
        zf = enc(frames)
    rf, sq_f, mean_f = AE.reconstruct(enc, dec, frames)
    assert torch.equal(rf, AE.decode(dec, zf))
    _check_errors(rf, loader_floats(frames), sq_f, mean_f)
    rfb, _, _ = AE.reconstruct(enc, dec, frames, out="bytes")
    assert torch.equal(rfb, AE.decode(dec, zf, out="bytes"))


def test_module_forward_takes_the_kernels_only_without_a_graph(case, monkeypatch):
    from ndivplanning_amd import autoencoder_eval as AE
    from ndivplanning_amd.models import image_autoencoder as IA
    dec = pickle.loads(pickle.dumps(case["dec"]))                            # a copy: the shared case stays as it is
    z = case["codes"][:3].view(3, 128, 1, 1)
    want = AE.decode(dec, z)
    assert torch.equal(want, AE.decode(case["dec"], z))
    torch_calls = []
    real = IA.Decoder._forward_torch

    def spy(self, x):
        torch_calls.append(tuple(x.shape))
        return real(self, x)

    def boom(self, x):
        raise AssertionError("_forward_torch called on the kernel path")

    monkeypatch.setattr(IA.Decoder, "_forward_torch", boom)
    with torch.no_grad():
        out = dec(z)
    assert torch.equal(out, want) and out.grad_fn is None and not out.requires_grad
    for p in dec.parameters():
        p.requires_grad_(False)
    out = dec(z)                                                            # grad mode on, nothing to differentiate
    assert torch.equal(out, want) and out.grad_fn is None
    for p in dec.parameters():
        p.requires_grad_(True)
    monkeypatch.setattr(IA.Decoder, "_forward_torch", spy)
    # grad enabled and parameters requiring grad: PyTorch, with a graph
    out = dec(z)
    assert len(torch_calls) == 1 and out.grad_fn is not None and out.shape == (3, 3, 128, 128)
    out.sum().backward()
    assert dec.deconv1.weight.grad is not None
    dec.zero_grad(set_to_none=True)
    with torch.no_grad():
        # training mode, a CPU tensor on a CPU copy, another dtype, another shape: PyTorch
        dec.train()
        dec(z)                                                              # (moves this copy's running statistics)
        dec.eval()
        assert len(torch_calls) == 2
        cpu = pickle.loads(pickle.dumps(dec)).cpu()
        assert cpu(z.cpu()).device.type == "cpu" and len(torch_calls) == 3
        with pytest.raises(RuntimeError):
            dec(z.half())
        assert len(torch_calls) == 4
        assert dec(torch.zeros(2, 128, 2, 2, device=DEV)).shape[:2] == (2, 3) and len(torch_calls) == 5


def test_in_place_changes_reach_the_next_call(case):
    """The folded vector is cached by the versions of the parameters and buffers: a weight and a running variance
    changed in place are seen by the next call (within the oracle's bound of the CHANGED module)."""
    dec = pickle.loads(pickle.dumps(case["dec"]))                            # a copy: the shared case stays as it is
    z = case["codes"][:2].view(2, 128, 1, 1)
    cpu = pickle.loads(pickle.dumps(dec)).cpu()

    def oracle():
        with torch.no_grad():
            f32 = cpu._forward_torch(z.cpu())
            cpu.double()
            f64 = cpu._forward_torch(z.cpu().double())
            cpu.float()
        return f64.to(DEV), torch.clamp(4 * (f32.double() - f64).abs(), min=1e-5).to(DEV)

    with torch.no_grad():
        before = dec(z)
        assert "_ndp_packed" in dec.__dict__
        dec.deconv3.weight.mul_(1.25)
        cpu.deconv3.weight.mul_(1.25)
        f64, bound = oracle()
        after = dec(z)
        assert not torch.equal(after, before)
        assert ((after.double() - f64).abs() <= bound).all()
        dec.deconv2_bn.running_var.mul_(2.0)
        cpu.deconv2_bn.running_var.mul_(2.0)
        f64, bound = oracle()
        again = dec(z)
        assert not torch.equal(again, after)
        assert ((again.double() - f64).abs() <= bound).all()


def test_pickle_of_a_decoder_that_has_run(case):
    import models.image_autoencoder  # noqa: F401  (binds the reference's class path)
    dec = case["dec"]
    with torch.no_grad():
        dec(case["codes"][:1].view(1, 128, 1, 1))
    assert "_ndp_packed" in dec.__dict__ and "_ndp_ws" in dec.__dict__
    buf = io.BytesIO()
    torch.save(dec, buf)
    raw = buf.getvalue()
    assert b"models.image_autoencoder" in raw and b"_ndp_ws" not in raw and b"_ndp_packed" not in raw
    assert len(raw) < 4 * sum(p.numel() for p in dec.state_dict().values()) + (1 << 20)    # parameters, no workspace
    back = torch.load(io.BytesIO(raw), map_location=DEV, weights_only=False)
    with torch.no_grad():
        assert torch.equal(back.eval()(case["codes"][:1].view(1, 128, 1, 1)), dec(case["codes"][:1].view(1, 128, 1, 1)))


def test_evaluate_walks_datasets(case, tmp_path):
    from ndivplanning_amd import autoencoder_eval as AE
    from ndivplanning_amd.jpeg import JpegDecoder, pack_jpegs
    from ndivplanning_amd.train_autoencoder import make_dataset
    enc, dec = case["enc"], case["dec"]
    ds = make_dataset("synthetic:3:images", seed=4)
    state = torch.random.get_rng_state()
    mean, per_image = AE.evaluate(enc, dec, ds, batch_size=2)
    assert torch.equal(torch.random.get_rng_state(), state)                 # no random number drawn
    assert per_image.shape == (45,) and mean.shape == (1,) and per_image.is_cuda
    frames = torch.cat([ds[i][0] for i in range(3)]).to(DEV)
    _, sq, _ = AE.reconstruct(enc, dec, frames[:30])
    assert torch.equal(per_image[:30], sq)
    assert abs(mean.item() - per_image.double().mean().item()) <= 1e-6 * mean.item()
    # JPEG streams: decoded on the device, the error against the decoded bytes
    dj = make_dataset("synthetic:1:jpeg", seed=4)
    mean_j, per_j, (inputs, recons) = AE.evaluate(enc, dec, dj, batch_size=1, keep=2)
    u8 = JpegDecoder(DEV).decode(*pack_jpegs(dj[0][0]))
    rb, sq_j, mj = AE.reconstruct(enc, dec, u8, out="bytes")
    assert torch.equal(per_j, sq_j) and torch.equal(mean_j, mj)
    assert torch.equal(inputs, u8[:2]) and torch.equal(recons, rb[:2])
    # the command line: whole-module checkpoints in, the mean and PNG pairs out
    import models.image_autoencoder  # noqa: F401
    torch.save(enc, str(tmp_path / "encoder_1.pt"))
    torch.save(dec, str(tmp_path / "decoder_1.pt"))
    lines = []
    got = AE.main(["--encoder", str(tmp_path / "encoder_1.pt"), "--decoder", str(tmp_path / "decoder_1.pt"), "--data",
                   "synthetic:1:jpeg", "--batch-size", "1", "--save-dir", str(tmp_path / "png"), "--num-save", "2"],
                  log=lambda *a: lines.append(a))
    dj1 = make_dataset("synthetic:1:jpeg")
    want = AE.evaluate(enc, dec, dj1, batch_size=1)[0].item()
    assert got == want and lines[0][0] == "val_recon_loss:" and lines[0][1] == want
    assert sorted(os.listdir(str(tmp_path / "png"))) == ["input_000.png", "input_001.png", "recon_000.png", "recon_001.png"]
    from PIL import Image
    u8 = JpegDecoder(DEV).decode(*pack_jpegs(dj1[0][0][:2]))
    np.testing.assert_array_equal(np.array(Image.open(str(tmp_path / "png" / "input_001.png"))), u8[1].cpu().numpy())


def test_training_with_validation(tmp_path):
    from ndivplanning_amd import autoencoder_eval as AE, train_autoencoder as T
    plain_log, val_log = [], []
    _, _, plain = T.train("synthetic:4:images", batch_size=2, num_epochs=2, save_dir=str(tmp_path / "a"),
                          log=lambda *a: plain_log.append(a))
    enc, dec, losses = T.train("synthetic:4:images", batch_size=2, num_epochs=2, val_data="synthetic:2:images",
                               save_dir=str(tmp_path / "b"), log=lambda *a: val_log.append(a))
    assert len(plain) == 4 and losses == plain                              # bit-identical step losses
    assert not any(len(line) == 3 and line[1] == "val_recon_loss:" for line in plain_log)
    vals = [line for line in val_log if len(line) == 3 and line[1] == "val_recon_loss:"]
    assert [line[0] for line in vals] == [0, 1]
    assert [v for _, v in T.train.last_val_losses] == [line[2] for line in vals]
    assert enc.training and dec.training and "_ndp_ws" not in dec.__dict__
    want = AE.evaluate(enc.eval(), dec.eval(), T.make_dataset("synthetic:2:images", seed=2), batch_size=2)[0].item()
    assert abs(vals[1][2] - want) <= 1e-5 * want
    assert all(np.isfinite(line[2]) and line[2] > 0 for line in vals)
    # every other epoch
    log3 = []
    T.train("synthetic:2:images", batch_size=2, num_epochs=2, val_data="synthetic:1:images", val_every=2,
            save_dir=str(tmp_path / "c"), log=lambda *a: log3.append(a))
    assert [line[0] for line in log3 if len(line) == 3 and line[1] == "val_recon_loss:"] == [1]
