#!/usr/bin/env python3
"""Golden vector for the image autoencoder, from the REFERENCE's own `models.image_autoencoder.Encoder` / `Decoder`
driven exactly as train_autoencoder.py:37-90 drives them: torch.manual_seed(1), Encoder() then Decoder(), weight_init
of the decoder then the encoder (mean 0, std 0.02), one optim.Adam over the two parameter groups (lr 2e-4, betas
(0.5, 0.999)), nn.MSELoss of the reconstruction against the input, two iterations on a small batch.
Runs only in the build container (needs /root/reference); the .npz travels.

The 21.6 M parameters are not stored: the fixture records the seeds, checksums of the initial state_dicts, both losses,
reconstruction samples, per-tensor gradient checksums of both iterations, post-step parameter checksums and the running
statistics after the two steps.

Usage: python tests/golden/make_golden_autoencoder.py
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
SEED, DATA_SEED, N = 1, 2, 2
SAMPLE_IDX = np.arange(0, N * 3 * 128 * 128, 997)


def sums(t):
    t = t.detach().double()
    return np.array([t.sum().item(), t.abs().sum().item(), (t * t).sum().item()])


def images():
    gen = torch.Generator().manual_seed(DATA_SEED)
    return [torch.rand(N, 3, 128, 128, generator=gen) * 2 - 1 for _ in range(2)]


def main():
    sys.path.insert(0, REF)
    from models.image_autoencoder import Decoder, Encoder         # the reference's module
    torch.set_num_threads(1)
    torch.manual_seed(SEED)
    encoder, decoder = Encoder(), Decoder()
    decoder.weight_init(mean=0.0, std=0.02)
    encoder.weight_init(mean=0.0, std=0.02)
    out = {"seed": np.array(SEED), "data_seed": np.array(DATA_SEED), "n": np.array(N), "sample_idx": SAMPLE_IDX}
    for pre, m in (("encoder.", encoder), ("decoder.", decoder)):
        for k, v in m.state_dict().items():
            if v.is_floating_point():
                out["init/" + pre + k] = sums(v)
    mse = torch.nn.MSELoss()
    opt = torch.optim.Adam([{"params": decoder.parameters()}, {"params": encoder.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    losses = []
    for it, x in enumerate(images()):
        recon = decoder(encoder(x))
        loss = mse(recon, x)
        opt.zero_grad()
        loss.backward()
        losses.append(loss.item())
        out["recon%d" % it] = recon.detach().reshape(-1)[SAMPLE_IDX].double().numpy()
        for pre, m in (("encoder.", encoder), ("decoder.", decoder)):
            for k, p in m.named_parameters():
                if p.grad is not None:
                    out["grad%d/%s%s" % (it, pre, k)] = sums(p.grad)
        opt.step()
        for pre, m in (("encoder.", encoder), ("decoder.", decoder)):
            for k, v in m.state_dict().items():
                if v.is_floating_point():
                    out["post%d/%s%s" % (it, pre, k)] = sums(v)
    out["losses"] = np.array(losses)
    path = os.path.join(HERE, "autoencoder_case.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "losses", losses)


if __name__ == "__main__":
    main()
