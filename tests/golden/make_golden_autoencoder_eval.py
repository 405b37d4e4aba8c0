#!/usr/bin/env python3
"""Golden vector for the EVAL-mode image autoencoder (decode, reconstruct, reconstruction error), from the REFERENCE's
own `models.image_autoencoder.Encoder` / `Decoder` in eval mode.  Runs only in the build container (needs
/root/reference); the .npz travels.

Recipe (`build_modules`, which tests/test_autoencoder_eval.py and tests/test_gpu_autoencoder_eval.py replay through the
mirror's classes): torch.manual_seed(SEED), Encoder() then Decoder(), weight_init of the decoder then the encoder
(train_autoencoder.py:54-57) with std WEIGHT_STD, then every BatchNorm2d of the encoder and of the decoder, in module
order, gets seeded non-trivial values from one generator (BN_SEED) -- gamma in [0.5, 1.5], beta in [-0.2, 0.2],
running_mean ~ N(0, 0.1), running_var in [0.5, 1.5] -- so that folding the BatchNorms is really exercised.
WEIGHT_STD = 0.04 puts the standard deviation of both outputs between 0.2 and 0.8 (recorded as out_std; with the
training script's 0.02 the untrained output is ~1e-3 and tanh, the bytes and the error would be tested near zero only).

The 21.6 M parameters are not stored: the fixture records the seeds and recipe constants, checksums of the state_dicts,
the N codes, strided samples of decoder(codes) and decoder(encoder(x)), the reference's bytes
(denorm(...).astype(np.uint8), train_autoencoder.py:42-43, 97-100) at the same positions, and the per-image and mean
squared errors of the reconstruction against its input.

Usage: python tests/golden/make_golden_autoencoder_eval.py
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
SEED, BN_SEED, DATA_SEED, CODE_SEED, N = 1, 5, 2, 3, 2
WEIGHT_STD = 0.04
SAMPLE_IDX = np.arange(0, N * 3 * 128 * 128, 997)


def sums(t):
    t = t.detach().double()
    return np.array([t.sum().item(), t.abs().sum().item(), (t * t).sum().item()])


def build_modules(Encoder, Decoder):
    """The seeded eval-mode (encoder, decoder) of the recipe above, on the CPU, from the given classes."""
    torch.manual_seed(SEED)
    encoder, decoder = Encoder(), Decoder()
    decoder.weight_init(mean=0.0, std=WEIGHT_STD)
    encoder.weight_init(mean=0.0, std=WEIGHT_STD)
    gen = torch.Generator().manual_seed(BN_SEED)
    with torch.no_grad():
        for module in (encoder, decoder):
            for m in module.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    c = m.num_features
                    m.weight.copy_(0.5 + torch.rand(c, generator=gen))
                    m.bias.copy_(-0.2 + 0.4 * torch.rand(c, generator=gen))
                    m.running_mean.copy_(0.1 * torch.randn(c, generator=gen))
                    m.running_var.copy_(0.5 + torch.rand(c, generator=gen))
    return encoder.eval(), decoder.eval()


def images():
    return torch.rand(N, 3, 128, 128, generator=torch.Generator().manual_seed(DATA_SEED)) * 2 - 1


def codes():
    return torch.randn(N, 128, 1, 1, generator=torch.Generator().manual_seed(CODE_SEED))


def denorm_bytes(t):
    """train_autoencoder.py:42-43 + .astype(np.uint8) (:97-100), on the whole tensor."""
    return (((t + 1.0) / 2.0) * 255.0).numpy().astype(np.uint8)


def main():
    sys.path.insert(0, REF)
    from models.image_autoencoder import Decoder, Encoder         # the reference's module
    torch.set_num_threads(1)
    encoder, decoder = build_modules(Encoder, Decoder)
    out = {"seed": np.array(SEED), "bn_seed": np.array(BN_SEED), "data_seed": np.array(DATA_SEED),
           "code_seed": np.array(CODE_SEED), "n": np.array(N), "weight_std": np.array(WEIGHT_STD), "sample_idx": SAMPLE_IDX}
    for pre, m in (("encoder.", encoder), ("decoder.", decoder)):
        for k, v in m.state_dict().items():
            if v.is_floating_point():
                out["state/" + pre + k] = sums(v)
    x, z = images(), codes()
    with torch.no_grad():
        dec = decoder(z)
        rec = decoder(encoder(x))
    out["codes"] = z.reshape(N, 128).numpy()
    out["decode"] = dec.reshape(-1)[SAMPLE_IDX].double().numpy()
    out["recon"] = rec.reshape(-1)[SAMPLE_IDX].double().numpy()
    out["decode_u8"] = denorm_bytes(dec).reshape(-1)[SAMPLE_IDX]
    out["recon_u8"] = denorm_bytes(rec).reshape(-1)[SAMPLE_IDX]
    out["out_std"] = np.array([dec.double().std().item(), rec.double().std().item()])
    err = ((rec.double() - x.double()) ** 2).reshape(N, -1).mean(dim=1)
    out["mse"] = err.numpy()
    out["mean_mse"] = np.array(err.mean().item())
    assert 0.2 <= out["out_std"].min() and out["out_std"].max() <= 0.8, out["out_std"]
    path = os.path.join(HERE, "autoencoder_eval_case.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "out_std", out["out_std"], "mse", out["mse"], "mean", out["mean_mse"])


if __name__ == "__main__":
    main()
