"""CPU: the "trained-like" state recipe (tests/trained_state.py) that the mid-training GPU tests start from: it is
deterministic, leaves no floating tensor at its initial value, produces the state the reference-generated fixture
(tests/golden/forward_model_case_trained.npz) was recorded from, stays far from the cancellation regime of
E[x^2] - mean^2, and does not turn the biases in front of a BatchNorm into something with a gradient."""
import numpy as np
import torch

import trained_state as TS
from conftest import load_golden
from oracle import forward_model_oracle as FO

# biases of the layers a BatchNorm follows (tests/test_gpu_forward_model.py): the batch mean removes them from the function
NOISE_BIASES = tuple("%s.bias" % n for n in ("encoder.conv1", "encoder.conv2", "encoder.conv3", "decoder.deconv1",
                                             "decoder.deconv2", "decoder.deconv3", "decoder.deconv4", "decoder.deconv5",
                                             "decoder.deconv6", "decoder.conv_refine_1"))


def _case():
    g = load_golden("forward_model_case_trained")
    seed, data_seed, n = (int(v) for v in g["meta"])
    return g, seed, data_seed, FO.init_forward_model_state(seed)


def test_the_recipe_is_deterministic_and_moves_every_tensor():
    g, seed, _, init = _case()
    a, b = TS.trained_like(init, seed), TS.trained_like(init, seed)
    other = TS.trained_like(init, seed + 1)
    assert list(a) == list(init)
    scales = []
    for k, v in init.items():
        assert a[k].dtype == v.dtype and a[k].shape == v.shape, k
        assert torch.equal(a[k], b[k]), k                              # same seed, same bits
        if k.endswith("num_batches_tracked"):
            assert int(a[k]) == TS.BATCHES_TRACKED == 7, k
            continue
        # no element left at its initial value (but a weight that was drawn as exactly 0: one of deconv2's 16 M is)
        assert not bool(((a[k] == v) & (v != 0 if v.dim() == 4 else True)).any()), k
        assert not torch.equal(a[k], other[k]), k
        if "_bn." not in k and k.endswith(".weight"):
            ratio = (a[k].double() / v.double())[v != 0]
            assert float(ratio.max() - ratio.min()) <= 1e-6 and 1.0 <= float(ratio.mean()) < 2.5, k   # one scalar per tensor
            scales.append(round(float(ratio.mean()), 6))
        elif k.endswith(("running_var", "_bn.weight")):
            assert 0.5 <= float(a[k].min()) and float(a[k].max()) < 1.5, k
        elif k.endswith("_bn.bias"):
            assert -0.2 <= float(a[k].min()) and float(a[k].max()) < 0.2, k
    assert len(set(scales)) == len(scales) == 14                       # no two layers share a scale
    # the state the fixture's reference run started from (the fixture stores checksums, not 33 M weights)
    np.testing.assert_allclose(np.array(TS.state_checksum(a)), g["state_checksum"], rtol=1e-12)
    assert "trained" in g and not torch.equal(a["encoder.conv4_bn.weight"], init["encoder.conv4_bn.weight"])


def test_the_recipe_works_on_the_autoencoder_modules():
    from ndivplanning_amd.models.image_autoencoder import Decoder, Encoder
    torch.manual_seed(0)
    for module in (Encoder(), Decoder()):
        sd = {k: v.clone() for k, v in module.state_dict().items()}
        new = TS.trained_like(sd, 4)
        module.load_state_dict(new)                                   # every key, shape and dtype as the module's own
        for k, v in sd.items():
            if v.dtype.is_floating_point:
                assert float((new[k] == v).float().mean()) <= 1e-5, k   # (a scale within an ulp of 1 keeps tiny elements)
            else:
                assert int(new[k]) == 7, k


def test_one_step_stays_off_the_cancellation_regime_and_noise_biases_stay_noise():
    """n = 1, fp64: at all ten BatchNorm sites mean^2 / var <= 50 (measured at most 9.3), and the gradient of a bias in
    front of a BatchNorm is still rounding noise: <= 1e-12 of its layer's weight-gradient scale (measured 1e-16 .. 1e-20
    against weight-gradient norms of 1e-2) -- the N(0, 0.1) biases change running_mean, not the function."""
    torch.set_num_threads(8)
    _, seed, data_seed, init = _case()
    state = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in TS.trained_like(init, seed).items()}
    gen = torch.Generator().manual_seed(data_seed)
    frames = torch.rand(1, 3, 3, 128, 128, generator=gen) * 2.0 - 1.0
    actions = torch.rand(1, 3, 4, generator=gen) * 2.0 - 1.0
    before = {k: v.clone() for k, v in state.items()}
    with TS.record_mean2_over_var(FO) as seen:
        out = FO.ForwardModelTrainer(state, lr=2e-4).step(frames[:, 0].double(), frames[:, 1].double(), actions[:, 0].double())
    print("mean^2 / var per BatchNorm site:", ["%.2f" % s for s in seen])
    TS.assert_guard(seen, 10)
    for name in NOISE_BIASES:
        wscale = float(out["grads"][name[:-4] + "weight"].norm())
        got = float(out["grads"][name].abs().max())
        print("%s: |grad| max %.2e, weight-gradient norm %.2e" % (name, got, wscale))
        assert wscale > 0 and got <= 1e-12 * wscale, (name, got, wscale)
    # the running means carry the biases: moved by 0.1 x (batch mean - old), the batch mean containing the bias
    for k in ("encoder.conv1_bn", "decoder.deconv4_bn"):
        assert int(state[k + ".num_batches_tracked"]) == 8
        assert not torch.equal(state[k + ".running_mean"], before[k + ".running_mean"])
    for k in ("encoder.conv4_bn", "encoder.conv5_bn"):                # constructed, never applied: untouched, the 7 included
        for leaf in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
            assert torch.equal(state[k + "." + leaf].detach(), before[k + "." + leaf]), (k, leaf)
