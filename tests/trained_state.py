"""TEST INFRASTRUCTURE -- one recipe for a "trained-like" state of the conv networks (the forward model, the image
autoencoder's encoder / decoder), shared by every test that starts a training step from somewhere else than what
`weight_init` leaves.

Right after `weight_init` every convolution bias is 0, every BatchNorm weight 1 and bias 0, the running statistics 0 / 1
and the batch counter 0: a bias taken from the wrong column, a swapped gamma / beta channel, a momentum update that
forgets the old value or a running mean without the convolution's bias all give the right result from that state.
`trained_like` returns a state in which none of these is invisible.  No GPU is touched here."""
import contextlib
from collections import OrderedDict

import torch

BATCHES_TRACKED = 7          # what every BatchNorm's counter is set to (the never-applied conv4_bn / conv5_bn included)
MEAN2_OVER_VAR_MAX = 50.0    # the guard: beyond this E[x^2] - mean^2 over fp32 sums is a question of its own


def trained_like(state, seed):
    """A new state_dict with the keys of `state`, drawn from torch.Generator().manual_seed(1000 + seed) in state_dict order:

        conv / deconv weight   weight x (1 + 1.5 U[0,1)), one scalar per tensor (no two layers share a scale)
        conv / deconv bias     N(0, 0.1) -- every one, those in front of a BatchNorm included
        BatchNorm weight       0.5 + U[0,1)
        BatchNorm bias         -0.2 + 0.4 U[0,1)
        running_mean           N(0, 0.1)
        running_var            0.5 + U[0,1)
        num_batches_tracked    7

    conv4_bn / conv5_bn (constructed, never applied) are perturbed as well: a step must hand every value of theirs back."""
    gen = torch.Generator().manual_seed(1000 + seed)
    out = OrderedDict()
    for name, t in state.items():
        t = t.detach()
        if name.endswith("num_batches_tracked"):
            out[name] = torch.full_like(t, BATCHES_TRACKED)
            continue
        rand = lambda: torch.rand(t.shape, generator=gen)            # noqa: E731
        randn = lambda: torch.randn(t.shape, generator=gen)          # noqa: E731
        if name.endswith("running_mean"):
            new = 0.1 * randn()
        elif name.endswith("running_var"):
            new = 0.5 + rand()
        elif "_bn." in name:
            new = 0.5 + rand() if name.endswith(".weight") else -0.2 + 0.4 * rand()
        elif name.endswith(".bias"):
            new = 0.1 * randn()
        else:
            assert name.endswith(".weight") and t.dim() == 4, name
            new = t.float() * (1.0 + 1.5 * torch.rand(1, generator=gen))
        out[name] = new.to(t.dtype)
    return out


def state_checksum(state):
    """[sum, sum of magnitudes, count] over the floating tensors, in fp64 (the fixtures' `state_checksum`)."""
    w64 = torch.cat([v.detach().double().reshape(-1) for v in state.values() if v.dtype.is_floating_point])
    return [w64.sum().item(), w64.abs().sum().item(), float(w64.numel())]


@contextlib.contextmanager
def record_mean2_over_var(module_with_F):
    """While active, every training-mode F.batch_norm call made through `module_with_F.F` (oracle.forward_model_oracle)
    appends the largest per-channel mean^2 / var (biased) of its input to the yielded list, one entry per BatchNorm site."""
    real = module_with_F.F
    seen = []

    class Spy:
        def __getattr__(self, name):
            return getattr(real, name)

        @staticmethod
        def batch_norm(x, rm, rv, w, b, training, *a, **kw):
            if training:
                with torch.no_grad():
                    d = x.detach().double()
                    dims = [i for i in range(d.dim()) if i != 1]
                    seen.append(float((d.mean(dims) ** 2 / d.var(dims, unbiased=False)).max()))
            return real.batch_norm(x, rm, rv, w, b, training, *a, **kw)
    module_with_F.F = Spy()
    try:
        yield seen
    finally:
        module_with_F.F = real


def assert_guard(seen, sites):
    """The recipe keeps every BatchNorm input far from the regime where E[x^2] - mean^2 loses digits.  A failure here
    means the recipe (or the inputs) changed; it is not a finding about a kernel."""
    assert len(seen) == sites, (len(seen), sites)
    assert max(seen) <= MEAN2_OVER_VAR_MAX, "mean^2 / var up to %.1f: the recipe was altered" % max(seen)
