#!/usr/bin/env python3
"""Golden vector for the evaluation of the forward (next-frame) model -- multi-step prediction error -- from the
REFERENCE's own `models.forward_encoder.ForwardAutoencoder` in `.eval()` on the CPU.  Runs only in the build container
(needs /root/reference); the .npz travels and holds data only.

Recipe (`build_module`, which tests/test_forward_model_eval.py and tests/test_gpu_forward_model_eval.py replay through the
oracle's restatement and the mirror's class): torch.manual_seed(SEED), ForwardAutoencoder(), weight_init of the decoder
then the encoder (train_forward_model.py:68-70) with std WEIGHT_STD, then every BatchNorm2d, in module order, gets seeded
non-trivial values from one generator (BN_SEED) -- gamma in [0.5, 1.5], beta in [-0.2, 0.2], running_mean ~ N(0, 0.1),
running_var in [0.5, 1.5] -- so that the eval-mode BatchNorm is really exercised.  WEIGHT_STD = 0.03 gives a residual that
matters (recorded as resid_std; with the training script's 0.02 the untrained residual is ~1e-3 and the model's error
could not be told from the persistence error).

The case: B = 2 trajectories of T = 4 byte frames [T,128,128,3] with bytes in 40 .. 215 (so that state + residual stays
inside [-1, 1], where the reference's own cast to bytes and the kernels' saturating one agree; asserted below on every
value, not only the sampled ones), actions ~ U[-1, 1), and a rollout from EVERY start frame for as long as a target frame
exists: start t is fed its own fp32 predictions for h = 1 .. T - 1 - t steps (at most 3) and scored against frame t + h.
Prediction order: trajectory, then start, then h (12 predictions).

The 33 M parameters are not stored: the fixture records the seeds and recipe constants, checksums of the state_dict, the
byte frames, the actions, strided samples ([:, ::16, ::16]) of every prediction, each prediction's MSE against its target
and the persistence MSE (start frame against the same target) in fp32 as the reference computes them (nn.MSELoss), and
the reference's bytes, denorm(...).astype(np.uint8) (train_forward_model.py:116-145), at the sampled positions.

Usage: python tests/golden/make_golden_fm_eval.py
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
SEED, BN_SEED, DATA_SEED = 11, 12, 13
B, T, H = 2, 4, 3
WEIGHT_STD = 0.03
BYTE_LO, BYTE_HI = 40, 216


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def sums(t):
    t = t.detach().double()
    return np.array([t.sum().item(), t.abs().sum().item(), (t * t).sum().item()])


def build_module(ForwardAutoencoder):
    """The seeded eval-mode module of the recipe above, on the CPU, from the given class."""
    torch.manual_seed(SEED)
    model = ForwardAutoencoder()
    model.decoder.weight_init(mean=0.0, std=WEIGHT_STD)
    model.encoder.weight_init(mean=0.0, std=WEIGHT_STD)
    gen = torch.Generator().manual_seed(BN_SEED)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                c = m.num_features
                m.weight.copy_(0.5 + torch.rand(c, generator=gen))
                m.bias.copy_(-0.2 + 0.4 * torch.rand(c, generator=gen))
                m.running_mean.copy_(0.1 * torch.randn(c, generator=gen))
                m.running_var.copy_(0.5 + torch.rand(c, generator=gen))
    return model.eval()


def inputs():
    """(byte frames uint8 [B,T,128,128,3], actions float32 [B,T,4])"""
    gen = torch.Generator().manual_seed(DATA_SEED)
    frames = torch.randint(BYTE_LO, BYTE_HI, (B, T, 128, 128, 3), generator=gen, dtype=torch.uint8)
    actions = torch.rand(B, T, 4, generator=gen) * 2.0 - 1.0
    return frames, actions


def norm_frames(frames_u8):
    """utils/hdf5_load.py:9-11 on byte frames [...,128,128,3] -> float32 [...,3,128,128]."""
    x = (frames_u8.to(torch.float32).div(255) - 0.5) * 2.0
    return x.movedim(-1, -3).contiguous()


def order():
    """[(trajectory, start, h)] of the stored predictions."""
    return [(b, t, h) for b in range(B) for t in range(T - 1) for h in range(1, min(H, T - 1 - t) + 1)]


def denorm_bytes(t):
    """train_forward_model.py:41-42 denorm + .astype(np.uint8) (:116-145), on the whole tensor."""
    return (((t + 1.0) / 2.0) * 255.0).numpy().astype(np.uint8)


def main():
    mpl = _stub("matplotlib")
    mpl.pyplot = _stub("matplotlib.pyplot")
    _stub("imageio")
    tv = _stub("torchvision")
    tv.datasets, tv.transforms = _stub("torchvision.datasets"), _stub("torchvision.transforms")
    sys.path.insert(0, REF)
    from models.forward_encoder import ForwardAutoencoder          # the reference's module
    torch.set_num_threads(1)
    model = build_module(ForwardAutoencoder)
    frames_u8, actions = inputs()
    frames = norm_frames(frames_u8)
    mse = torch.nn.MSELoss()
    out = {"seed": np.array(SEED), "bn_seed": np.array(BN_SEED), "data_seed": np.array(DATA_SEED),
           "weight_std": np.array(WEIGHT_STD), "shape": np.array([B, T, H]), "byte_range": np.array([BYTE_LO, BYTE_HI]),
           "frames_u8": frames_u8.numpy(), "actions": actions.numpy(), "order": np.array(order(), np.int32)}
    for k, v in model.state_dict().items():
        if v.is_floating_point():
            out["state/" + k] = sums(v)
    samples, bytes_, errs, base, resid_std = [], [], [], [], []
    lo, hi = 1.0, -1.0
    with torch.no_grad():
        for b in range(B):
            for t in range(T - 1):
                state = frames[b, t:t + 1]
                for h in range(1, min(H, T - 1 - t) + 1):
                    prev = state
                    state = model(prev, actions[b, t + h - 1:t + h])           # eval mode: state_cur + residual
                    target = frames[b, t + h:t + h + 1]
                    samples.append(state[0, :, ::16, ::16].numpy().copy())
                    bytes_.append(denorm_bytes(state)[0, :, ::16, ::16].copy())
                    errs.append(mse(state, target).item())
                    base.append(mse(frames[b, t:t + 1], target).item())
                    resid_std.append((state - prev).double().std().item())
                    lo, hi = min(lo, state.min().item()), max(hi, state.max().item())
    # inside [-1, 1] the reference's cast (wraps outside) and a saturating one agree: every value, not only the samples
    assert -1.0 <= lo and hi <= 1.0, (lo, hi)
    assert min(resid_std) >= 0.02, resid_std
    out["pred_sample"] = np.stack(samples).astype(np.float32)       # [12,3,8,8]
    out["pred_u8_sample"] = np.stack(bytes_)                        # [12,3,8,8] uint8
    out["pred_mse"] = np.array(errs, np.float32)
    out["persistence_mse"] = np.array(base, np.float32)
    out["resid_std"] = np.array(resid_std)
    out["value_range"] = np.array([lo, hi])
    path = os.path.join(HERE, "fm_eval_case.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; range", lo, hi, "resid_std", min(resid_std), max(resid_std))
    print("pred_mse", out["pred_mse"], "\npersistence_mse", out["persistence_mse"])


if __name__ == "__main__":
    main()
