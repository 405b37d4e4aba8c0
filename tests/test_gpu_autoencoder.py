"""GPU: one autoencoder training iteration on the gfx950 kernels (ndp_ae_train_grads + ndp_ae_apply_adam) against the
fp64 restatement (the repo's Encoder._forward_torch + Decoder, float64 on the CPU, torch's Adam), elementwise; the
reference's two iterations (tests/golden/autoencoder_case.npz); determinism; the training script end to end; the
hand-off of the saved encoder to the GAN path."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "autoencoder_case.npz")
NOISE_BIASES = tuple("encoder.conv%d.bias" % i for i in (1, 2, 3)) + tuple("decoder.deconv%d.bias" % i for i in range(1, 6))
DEV = "cuda:0"

pytestmark = pytest.mark.gpu


def _models(seed, trained=False):
    """trained: from a mid-training state (tests/trained_state.py) -- non-zero biases (deconv6's, which no BatchNorm
    follows, among them: the k_ae_out_fwd_loss / k_ae_out_dgrad epilogues), BatchNorm weight / bias / running statistics
    off 1 / 0 / 0 / 1, batch counters at 7."""
    from ndivplanning_amd.models.image_autoencoder import Decoder, Encoder
    torch.manual_seed(seed)
    enc, dec = Encoder(), Decoder()
    dec.weight_init(0.0, 0.02)
    enc.weight_init(0.0, 0.02)
    if trained:
        from trained_state import trained_like
        enc.load_state_dict(trained_like(enc.state_dict(), seed))
        dec.load_state_dict(trained_like(dec.state_dict(), seed + 1))
    return enc, dec


def _images(n, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, 128, 128, generator=gen) * 2 - 1


def _masked_forward(enc, dec, x, masks):
    """Encoder._forward_torch + Decoder.forward with every ReLU's decision taken from `masks` (the run under test): among
    10^7 pre-activations some lie within rounding of zero, and one decided the other way moves a small map's gradients
    far more than rounding does (as in test_gpu_forward_model.py)."""
    m = {k: v.to(x.dtype) for k, v in masks.items()}
    h = x
    for i in (1, 2, 3):
        h = getattr(enc, "conv%d_bn" % i)(getattr(enc, "conv%d" % i)(h)) * m["feat%d" % i]
    h = enc.conv4(h) * m["feat4"]
    h = enc.conv5(h) * m["feat5"]
    h = enc.conv6(h)
    for i in range(1, 6):
        h = getattr(dec, "deconv%d_bn" % i)(getattr(dec, "deconv%d" % i)(h)) * m["up%d" % i]
    return torch.tanh(dec.deconv6(h))


def _cpu_step(enc, dec, x, dtype, masks=None):
    """loss, gradients, running statistics and post-Adam parameters of one reference iteration on the CPU."""
    enc, dec = enc.to(dtype).train(), dec.to(dtype).train()
    opt = torch.optim.Adam([{"params": dec.parameters()}, {"params": enc.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    x = x.to(dtype)
    recon = _masked_forward(enc, dec, x, masks) if masks is not None else dec(enc._forward_torch(x))
    loss = ((recon - x) ** 2).mean()
    opt.zero_grad()
    loss.backward()
    mods = (("encoder.", enc), ("decoder.", dec))
    grads = {p + k: v.grad.detach().double().clone() for p, m in mods for k, v in m.named_parameters() if v.grad is not None}
    opt.step()
    post = {p + k: v.detach().double().clone() for p, m in mods for k, v in m.state_dict().items()}
    return loss.item(), grads, post


def _hip_step(enc, dec, x, batch=None):
    from ndivplanning_amd.autoencoder_trainer import AutoencoderTrainer
    tr = AutoencoderTrainer(enc.to(DEV).train(), dec.to(DEV).train(), batch=batch or x.shape[0], keep_reconstruction=True)
    tr.grads(x.to(DEV))
    tr.masks = {k: (tr.activation(k, x.shape[0]) > 0).cpu() for k in tr._MAPS}
    loss = tr.loss.item()
    grads = {k: v.double().cpu() for k, v in tr.named_gradients().items()}
    tr.apply()
    tr.sync_to_modules()
    mods = (("encoder.", enc), ("decoder.", dec))
    post = {p + k: v.detach().double().cpu() for p, m in mods for k, v in m.state_dict().items()}
    torch.cuda.synchronize()
    return tr, loss, grads, post


def _check(name, hip, f32, f64, floor):
    """fp64-adjudicated: the HIP value may be off the fp64 one by a few times what torch's own fp32 run is off it."""
    err = (hip - f64).abs().max().item()
    ref_err = (f32 - f64).abs().max().item()
    scale = f64.abs().max().item()
    print("%s: |hip - fp64| %.3e, |fp32 - fp64| %.3e, scale %.3e" % (name, err, ref_err, scale))
    assert err <= 8 * ref_err + floor * max(scale, 1e-30), "%s: |hip - fp64| %.3e, |fp32 - fp64| %.3e, scale %.3e" % (
        name, err, ref_err, scale)


@pytest.mark.parametrize("n,trained", [pytest.param(n, False, id=str(n)) for n in (1, 3, 16, 65, 240)]
                         + [pytest.param(n, True, id="trained-%d" % n) for n in (1, 3, 16)])
def test_step_matches_fp64_elementwise(n, trained):
    torch.set_num_threads(16)
    x = _images(n, 100 + n)
    tracked = 7 if trained else 0                                      # the batch counters before the step
    tr, lh, gh, ph = _hip_step(*_models(7, trained), x)
    l64, g64, p64 = _cpu_step(*_models(7, trained), x, torch.float64, tr.masks)
    l32, g32, p32 = _cpu_step(*_models(7, trained), x, torch.float32, tr.masks)
    assert abs(lh - l64) <= 8 * abs(l32 - l64) + 2e-6 * l64
    recon = tr.recon.cpu().double()
    with torch.no_grad():
        enc, dec = _models(7, trained)
        want = dec.double().train()(enc.double().train()._forward_torch(x.double()))
    assert (recon - want).abs().max().item() <= 1e-4
    assert set(gh) == set(g64)
    for k in g64:
        if k in NOISE_BIASES:
            # rounding noise: as small as the fp32 restatement's noise, relative to the layer's weight gradient
            wscale = g64[k.replace(".bias", ".weight")].abs().max().item()
            assert gh[k].abs().max().item() <= 8 * g32[k].abs().max().item() + 1e-5 * wscale, k
            continue
        _check("grad " + k, gh[k], g32[k], g64[k], 2e-5)
    lr = 2e-4
    for k in p64:
        if k.endswith("num_batches_tracked"):
            assert ph[k].item() == p64[k].item() == tracked + (0 if k.startswith(("encoder.conv4_bn", "encoder.conv5_bn")) else 1), k
        elif k.startswith(("encoder.conv4_bn", "encoder.conv5_bn")):
            assert torch.equal(ph[k], p64[k]), k                       # never applied: untouched
        elif k in NOISE_BIASES or k.endswith("running_mean"):
            # a noise gradient's Adam step is +-lr whatever its size; running means see the noise biases
            assert (ph[k] - p64[k]).abs().max().item() <= 2.5 * lr + 1e-5 * p64[k].abs().max().item(), k
        else:
            _check("post " + k, ph[k], p32[k], p64[k], 1e-6)


def test_two_iterations_match_reference_golden():
    g = np.load(GOLDEN)
    enc, dec = _models(int(g["seed"]))
    from ndivplanning_amd.autoencoder_trainer import AutoencoderTrainer
    n = int(g["n"])
    tr = AutoencoderTrainer(enc.to(DEV).train(), dec.to(DEV).train(), batch=n, keep_reconstruction=True)
    gen = torch.Generator().manual_seed(int(g["data_seed"]))
    xs = [torch.rand(n, 3, 128, 128, generator=gen) * 2 - 1 for _ in range(2)]
    for it, x in enumerate(xs):
        tr.step(x.to(DEV))
        assert abs(tr.loss.item() - g["losses"][it]) <= 1e-4 * g["losses"][it], it
        np.testing.assert_allclose(tr.recon.reshape(-1)[torch.from_numpy(g["sample_idx"]).to(DEV)].double().cpu().numpy(),
                                   g["recon%d" % it], atol=1e-3 if it else 5e-5)


def test_step_is_bit_reproducible_and_runs_smaller_batches():
    from ndivplanning_amd import _capi
    from ndivplanning_amd.autoencoder_trainer import AutoencoderTrainer
    x = _images(240, 5).to(DEV)
    outs = []
    for _ in range(2):
        enc, dec = _models(3)
        tr = AutoencoderTrainer(enc.to(DEV).train(), dec.to(DEV).train(), batch=240)
        tr.step(x)
        tr.grads(x[:17].contiguous())                                # a trainer built for 240 runs 17
        outs.append((tr.loss.clone(), tr.grad.clone(), tr.params.clone(), tr.stats.clone()))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    assert torch.isfinite(outs[0][1]).all()
    # the HIP kernels are what ran: per-kernel timing labels of one step
    _capi.timing_enable(True)
    try:
        tr.step(x[:16].contiguous())
        names = dict(_capi.timing_collect())
    finally:
        _capi.timing_enable(False)
    for k in ("k_ae_out_fwd_loss", "k_ae_out_dgrad", "k_ae_out_wgrad", "k_fm_gemm[ae.conv1]", "k_fm_gemm[ae.deconv5]",
              "k_fm_wgrad[ae.deconv2]", "k_fm_bn_bwd_apply", "k_fm_adam_pack"):
        assert k in names, (k, sorted(names))
    with pytest.raises(_capi.NdpError):
        tr.grads(_images(241, 0).to(DEV))


def test_the_optimizer_launch_leaves_the_second_weight_order_a_full_repack_would():
    """ndp_ae_apply_adam writes the new weights in both orders in one launch (k_fm_adam_pack with this network's segments:
    32 x 32 tiles of conv2 .. deconv5 transposed through LDS, conv1's compact [64][32] copy element by element, no
    refinement segment, deconv6 without a second order).  ndp_ae_pack_params rebuilds the second order from the parameters
    alone: after a training step it must change nothing.  The second order does not depend on the batch: one image."""
    from ndivplanning_amd import _capi
    from ndivplanning_amd.autoencoder_trainer import AutoencoderTrainer
    from ndivplanning_amd.models import image_autoencoder as IA
    enc, dec = _models(3)
    tr = AutoencoderTrainer(enc.to(DEV).train(), dec.to(DEV).train(), batch=1)
    tr.step(_images(1, 5).to(DEV))
    torch.cuda.synchronize()
    # the second-order region, from the layout: conv1 as [rows][27 -> 32 columns], conv2 .. deconv5 at their full size
    sizes = [IA.ae_layout(tr.lib, 0, l)[1][:3] for l in range(len(IA.AE_LAYERS) - 1)]
    p2 = sizes[0][0] * 32 + sum(r * t * c for r, t, c in sizes[1:])
    assert 18_000_000 < p2 < tr.lib.ndp_ae_workspace_offset(1, 0)  # (most of the 21.6 M parameters; ahead of the first map)
    before = tr.workspace[:p2].clone()
    assert int((before != 0).sum()) > p2 // 2                       # (it is in use)
    _capi.check(tr.lib.ndp_ae_pack_params(_capi.ptr(tr.params), _capi.ptr(tr.workspace), _capi.stream_ptr(DEV)),
                "ndp_ae_pack_params")
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int32), tr.workspace[:p2].view(torch.int32))


def test_training_script_and_gan_handoff(tmp_path):
    """python train_autoencoder.py on synthetic images for one epoch in a fresh interpreter; pickles with the reference
    class paths; the loss sequence equals a CPU replay of the same loop; the saved encoder feeds ndp_encoder_forward."""
    code = ("import sys, json; sys.argv = ['train_autoencoder.py', '--data', 'synthetic:2:images', '--batch-size', '1', "
            "'--epochs', '2', '--save-dir', %r]\n"
            "import runpy; g = runpy.run_path(%r, run_name='not_main')\n"
            "enc, dec, losses = g['main']()\nprint('LOSSES', json.dumps(losses))\n") % (str(tmp_path / "models"),
                                                                               os.path.join(ROOT, "train_autoencoder.py"))
    res = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, PYTHONPATH=ROOT))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    losses = [float(v) for v in res.stdout.split("LOSSES")[1].strip()[1:-1].split(",")]
    assert len(losses) == 4
    for name in ("encoder_1.pt", "decoder_1.pt"):
        raw = open(tmp_path / "models" / name, "rb").read()
        assert b"models.image_autoencoder" in raw
    # CPU replay of the same loop (seeds, loader order, modules, Adam) in float64
    from ndivplanning_amd.train_autoencoder import build_models, make_dataset
    from torch.utils import data
    torch.manual_seed(1)
    np.random.seed(1)
    loader = data.DataLoader(make_dataset("synthetic:2:images"), batch_size=1, shuffle=True)
    enc, dec = build_models(DEV)                       # (initialised on the GPU's generator, as the reference does)
    enc, dec = enc.cpu().double().train(), dec.cpu().double().train()
    opt = torch.optim.Adam([{"params": dec.parameters()}, {"params": enc.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    replay = []
    for _ in range(2):
        for images, _, _, _ in loader:
            x = images.view(-1, 3, 128, 128).double()
            loss = ((dec(enc._forward_torch(x)) - x) ** 2).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
            replay.append(loss.item())
    np.testing.assert_allclose(losses, replay, rtol=2e-4)
    # hand-off to train_gan.py: torch.load, eval mode, ndp_encoder_forward against PyTorch's eval forward
    sys.path.insert(0, ROOT)
    import models.image_autoencoder  # noqa: F401
    enc = torch.load(str(tmp_path / "models" / "encoder_1.pt"), map_location=DEV, weights_only=False).eval()
    assert type(enc).__module__ == "models.image_autoencoder" and enc.conv1_bn.num_batches_tracked.item() == 4
    x = _images(8, 9).to(DEV)
    with torch.no_grad():
        codes = enc(x)
        want = enc._forward_torch(x)
    assert (codes - want).abs().max().item() <= 1e-4 * max(1.0, want.abs().max().item())
