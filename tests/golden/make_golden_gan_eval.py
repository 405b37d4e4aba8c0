#!/usr/bin/env python3
"""Golden vector for the evaluation of the action generator -- best-of-K action error, diversity, the discriminator's
pick -- from the REFERENCE's own `models.gan.Decoder`, `models.gan.Discriminator` and `diversity` on the CPU, in fp32 and
in fp64.  Runs only where a reference checkout is at hand; the .npz travels and holds data only.

Two cases: "a" n = 5 rows x K = 6 samples with noise_dim 2 (the training configuration) and "b" n = 5 x K = 3 with
noise_dim 5.  Per case: torch.manual_seed(seed), Decoder(noise_dim), Discriminator(); every parameter is multiplied by
GAIN (the default initialisation gives samples that hardly differ: a best-of-K could not be told from sample 0), fc1's
noise columns once more by NOISE_GAIN, and snapped to multiples of 2^-8 (exactly representable: the stored parameters
compress well and are the same numbers in every precision).  codes ~ N(0,1) [n,256], actions ~ U[-1,1) [n,4], noise ~
U[0,1) [n,K,nz] from a generator of their own.  The network input is cat(repeat_interleave(codes, K), noise) as
train_gan.py:42-47 builds it; D sees (action_hat, the same repeated codes) and (actions, codes).

Stored per case (prefix "a/", "b/"): the parameters in state_dict order (g/fcN.weight ...), the inputs, and for "32" (the
reference's fp32) and "64" (the same modules in double): action_hat [n,K,4], fake_logits [n,K], real_logits [n], sample_err
[n,K], mean_err [n], action_mse (the reference's mse(repeat_interleave(actions, K), action_hat),
control_evaluation.py:140-142), best_err, best_k, best_curve, spread (the mean over i != j of diversity.compute_pairwise),
ndiv [n] (the row's share of diversity.compute_pairwise_divergence), ndiv_total (that function itself), d_fake_prob,
d_real_prob, d_pick_k, d_pick_err.

Asserted here, so that best_k / d_pick_k can be compared on ALL rows: in every row the two smallest e_k differ by at least
100 x the action-error bound the GPU test uses (2 sqrt(e) 1e-4 + 1e-8), and the two largest logits by at least 100 x 1e-4.

Usage: python tests/golden/make_golden_gan_eval.py REFERENCE_CHECKOUT
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {"a": dict(n=5, k=6, nz=2, seed=21, data_seed=25), "b": dict(n=5, k=3, nz=5, seed=23, data_seed=27)}
GAIN, NOISE_GAIN, STEP = 2.0, 64.0, 2.0 ** -8
ACTION_BOUND = 1e-4


def err_bound(e):
    """What an error of 1e-4 in every component of a sample can move its mean squared error e by."""
    return 2.0 * np.sqrt(e) * ACTION_BOUND + 1e-8


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _stubs():
    tv = _stub("torchvision")
    tv.models, tv.datasets, tv.transforms = _stub("torchvision.models"), _stub("torchvision.datasets"), _stub("torchvision.transforms")
    mpl = _stub("matplotlib")
    mpl.pyplot = _stub("matplotlib.pyplot")
    _stub("imageio")
    _stub("spectral_normalization", SpectralNorm=object)      # imported by models/gan.py, never used by these classes


def build_modules(Decoder, Discriminator, nz, seed):
    """The seeded modules of the recipe above, on the CPU in fp32, from the given classes."""
    torch.manual_seed(seed)
    g, d = Decoder(noise_dim=nz), Discriminator()
    with torch.no_grad():
        for m in (g, d):
            for p in m.parameters():
                p.mul_(GAIN)
        g.fc1.weight[:, 256:].mul_(NOISE_GAIN)
        for m in (g, d):
            for p in m.parameters():
                p.copy_(torch.round(p / STEP) * STEP)
    return g.eval(), d.eval()


def inputs(n, k, nz, data_seed):
    gen = torch.Generator().manual_seed(data_seed)
    codes = torch.randn(n, 256, generator=gen)
    actions = torch.rand(n, 4, generator=gen) * 2.0 - 1.0
    noise = torch.rand(n, k, nz, generator=gen)
    return codes, actions, noise


def first_best(values, larger):
    best, bk, run = values[0], 0, []
    for i, v in enumerate(values):
        if v == v and (best != best or (v > best if larger else v < best)):
            best, bk = v, i
        run.append(best)
    return bk, run


def metrics(g, d, diversity, codes, actions, noise, dtype):
    n, k, nz = noise.shape
    g, d = g.to(dtype), d.to(dtype)
    codes, actions, noise = codes.to(dtype), actions.to(dtype), noise.to(dtype)
    mse = torch.nn.MSELoss()
    with torch.no_grad():
        rep = torch.repeat_interleave(codes, k, dim=0)
        hat = g(torch.cat([rep, noise.view(n * k, nz)], dim=1))
        fake = d(hat, rep).view(n, k)
        real = d(actions, codes).view(n)
        hat3 = hat.view(n, k, 4)
        sq = (hat3 - actions[:, None, :]) ** 2
        sample_err = sq.mean(2)
        dx = diversity.compute_pairwise(hat3)
        z_delta, x_delta = diversity.compute_pair_distance(noise), diversity.compute_pair_distance(hat3)
        out = {
            "action_hat": hat3, "fake_logits": fake, "real_logits": real, "sample_err": sample_err,
            "mean_err": sq.mean((1, 2)), "action_mse": mse(torch.repeat_interleave(actions, k, dim=0), hat),
            "spread": dx.sum((1, 2)) / (k * (k - 1)), "ndiv": torch.relu(z_delta * 0.8 - x_delta).sum((1, 2)),
            "ndiv_total": diversity.compute_pairwise_divergence(hat3, noise),
            "d_fake_prob": torch.sigmoid(fake).mean(1), "d_real_prob": torch.sigmoid(real),
        }
    out = {key: v.numpy() for key, v in out.items()}
    picks = [first_best(list(row), larger=False) for row in out["sample_err"]]
    out["best_k"] = np.array([p[0] for p in picks], np.int32)
    out["best_curve"] = np.array([p[1] for p in picks], out["sample_err"].dtype)
    out["best_err"] = out["sample_err"][np.arange(n), out["best_k"]]
    out["d_pick_k"] = np.array([first_best(list(row), larger=True)[0] for row in out["fake_logits"]], np.int32)
    out["d_pick_err"] = out["sample_err"][np.arange(n), out["d_pick_k"]]
    g.float(), d.float()
    return out


def main(ref):
    _stubs()
    sys.path.insert(0, ref)
    import diversity                                               # the reference's modules
    from models.gan import Decoder, Discriminator
    torch.set_num_threads(1)
    out = {"gain": np.array([GAIN, NOISE_GAIN, STEP]), "action_bound": np.array(ACTION_BOUND)}
    for name, c in CASES.items():
        g, d = build_modules(Decoder, Discriminator, c["nz"], c["seed"])
        codes, actions, noise = inputs(c["n"], c["k"], c["nz"], c["data_seed"])
        out[name + "/shape"] = np.array([c["n"], c["k"], c["nz"], c["seed"], c["data_seed"]])
        for net, m in (("g", g), ("d", d)):
            for key, v in m.state_dict().items():
                assert np.array_equal(np.round(v.numpy() / STEP) * STEP, v.numpy())
                out["%s/%s/%s" % (name, net, key)] = v.numpy().copy()
        out[name + "/codes"], out[name + "/actions"], out[name + "/noise"] = codes.numpy(), actions.numpy(), noise.numpy()
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            for key, v in metrics(g, d, diversity, codes, actions, noise, dtype).items():
                out["%s/%s/%s" % (name, key, tag)] = v
        e, lg = np.sort(out[name + "/sample_err/64"], axis=1), np.sort(out[name + "/fake_logits/64"], axis=1)
        gap_e, gap_l = e[:, 1] - e[:, 0], lg[:, -1] - lg[:, -2]
        assert (gap_e >= 100 * err_bound(e[:, 1])).all(), (name, gap_e, 100 * err_bound(e[:, 1]))
        assert (gap_l >= 100 * ACTION_BOUND).all(), (name, gap_l)
        assert np.array_equal(out[name + "/best_k/32"], out[name + "/best_k/64"])
        assert np.array_equal(out[name + "/d_pick_k/32"], out[name + "/d_pick_k/64"])
        print(name, "best_k", out[name + "/best_k/64"], "d_pick_k", out[name + "/d_pick_k/64"], "min gaps", gap_e.min(), gap_l.min(),
              "\n  spread", out[name + "/spread/64"], "\n  ndiv", out[name + "/ndiv/64"], "\n  best_err", out[name + "/best_err/64"])
    path = os.path.join(HERE, "gan_eval_case.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "../reference")
