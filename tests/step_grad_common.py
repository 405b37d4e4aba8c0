"""What the gradient tests of the fused GAN step share: an adjudicator that holds the D and G
gradients a run of the step exposes to the fp64 oracle, per parameter tensor, with a bound measured on the fp32 oracle.
No GPU is touched here; tests/test_step_grad_adjudication_host.py proves it on the CPU, with the hand-written fp32
`StepMath` standing in for the run, and tests/test_gpu_step_gradients.py feeds it the kernels' numbers.

Why the references are *injected* with the run's own decisions.  The step is discontinuous in three places, and at each
of them two correct fp32 implementations part by far more than rounding:

* G's ReLUs: one pre-activation decided the other way moves a small layer's gradient by O(1);
* NDiv's hinge terms: `nd_grad` is ~1e3 x the BCE gradient per row and cancels within a row, and a few of its terms sit
  inside fp32 rounding in every batch -- the plain fp32 and fp64 steps differ by 0.6 (max norm) in the G gradient at
  FLAT = 448 / K = 6, and a bound measured that way lets a kernel lose a whole 64 x 64 job;
* D's leaky ReLUs: among the 1e6 .. 1e7 units of a pass one pre-activation within ~1e-7 of zero is the rule rather than
  the exception from a few thousand rows, and its decision moves fc1..fc3's gradients by the whole contribution of that
  unit in that row: ~1e-3 of the tensor's largest entry, up to 58 x the bound (measured on MI355X: B = 25 / K = 6, unit 244
  of D.h3, fake row 725, pre-activation +2.8e-8 in fp64; every D tensor but fc4's, which no decision enters, was off).

So the step is compared in pieces, each continuous once the run's decisions are taken over:

* D gradient: both oracles with the run's leaky-ReLU decisions (d.h_i > 0 of its saved D activations);
* G gradient = J_G(run's ReLU masks)^T . d_action(run): both oracles start G's backward from the run's dLoss/d action_hat
  (NDiv term included) and take the run's masks (g.h_i > 0) -- every weight-gradient job and the backward data path of
  G, with nothing of D or NDiv in the way;
* d_action = dBCE/d action_hat through the run's post-update D + the run's nd_grad, row by row, both oracles evaluated
  at the run's action_hat; rows that hold a D unit closer to zero than tau_D = 4 x max |pre32 - pre64| (per layer) are
  left out;
* `nd_grad` against the oracle's NDiv gradient at the run's action_hat; the FLAT rows that hold a hinge term closer to
  zero than tau = 4 x max |h32 - h64| are left out.

Both tau are measured per case on the two oracles; the share of rows left out is capped (MAX_LEFT_OUT), so that the
exception cannot swallow the check.

The rule, per tensor:  max |run - fp64| <= max(MARGIN x max |fp32 - fp64|, FLOOR x S), S = max |fp64 gradient| over
that layer's weight and bias together (fc5.bias under NDiv is a sum that cancels to ~1e-3 against terms of ~1e2).
MARGIN and FLOOR are tests/test_gpu_parity.py::_grad_close_adjudicated's numbers, applied per layer instead of net-wide.
"""
from collections import OrderedDict

import torch

from oracle import gan_oracle as O

MARGIN = 4.0            # x the fp32 oracle's own distance from fp64
FLOOR = 1e-5            # x the layer's largest fp64 gradient entry
MAX_LEFT_OUT = 0.03     # share of a case's rows a row-wise check may leave out (a condition, not a measurement)
G_ACTIVATIONS = ("g.h1", "g.h2", "g.h3", "g.h4")
D_ACTIVATIONS = ("d.h1", "d.h2", "d.h3")


def to_dtype(params, dt):
    return OrderedDict((n, v.detach().cpu().to(dt).clone()) for n, v in params.items())


def split_flat(flat, like):
    """Flat vector in state_dict order -> {name: tensor} shaped like `like`."""
    flat = flat.detach().cpu().reshape(-1)
    out, o = OrderedDict(), 0
    for n, v in like.items():
        out[n] = flat[o:o + v.numel()].reshape(v.shape)
        o += v.numel()
    assert o == flat.numel(), "flat vector of %d values for parameters of %d" % (flat.numel(), o)
    return out


def flatten(params):
    return torch.cat([p.reshape(-1) for p in params.values()])


def _as_dict(value, like):
    return value if isinstance(value, dict) else split_flat(value, like)


def inject(acts, masks):
    """Saved layer inputs [x, h1, h2, ..] with the decisions of h1.. replaced by `masks`: _mlp_backward reads a decision
    off the saved activation (h > 0), so a unit the run switched on is made positive and one it switched off non-positive.
    The values move by less than the pre-activation's rounding error: the two decisions differ only where it decides."""
    out = [acts[0]]
    for a, mk in zip(acts[1:], masks):
        out.append(torch.where(mk, a.clamp_min(1e-30), a.clamp_max(0.0)))
    return out


class Report:
    def __init__(self, what):
        self.what = what
        self.ratios = OrderedDict()     # tensor -> |run - fp64| / bound
        self.detail = OrderedDict()     # tensor -> (err_run, err_ref, S)
        self.failures = []              # tensors (and conditions) that broke their bound
        self.tau = 0.0                  # NDiv hinge terms
        self.left_out = 0.0             # share of FLAT rows the nd_grad check left out
        self.tau_d = 0.0                # D pre-activations (largest of the three layers)
        self.left_out_d = 0.0           # share of the M rows the d_action check left out
        self.losses64 = None            # (D_loss, G_loss, pair_div) of the fp64 oracle
        self.action_hat64 = None

    def add(self, name, err_run, err_ref, scale, finite=True):
        bound = max(MARGIN * err_ref, FLOOR * scale)
        ratio = 0.0 if err_run == 0.0 else (err_run / bound if bound > 0.0 else float("inf"))
        if not finite:
            ratio = float("inf")
        self.ratios[name] = ratio
        self.detail[name] = (err_run, err_ref, scale)
        if not ratio <= 1.0:
            self.failures.append(name)

    def cap(self, what, share):
        if share > MAX_LEFT_OUT:
            self.failures.append("%s rows left out (%.2f %% > %.0f %%)" % (what, 100 * share, 100 * MAX_LEFT_OUT))

    def worst(self, prefix=""):
        sel = {n: r for n, r in self.ratios.items() if n.startswith(prefix)}
        name = max(sel, key=sel.get)
        return name, sel[name]

    def line(self):
        parts = ["%s %.3f" % (n, r) for n, r in self.ratios.items()]
        return ("%s: |run - fp64| / bound per tensor: %s; NDiv tau %.2e, %.2f %% of the FLAT rows left out; "
                "D tau %.2e, %.2f %% of the rows left out" % (self.what, ", ".join(parts), self.tau, 100.0 * self.left_out,
                                                             self.tau_d, 100.0 * self.left_out_d))

    def assert_ok(self):
        def one(n):
            if n not in self.detail:
                return n
            return "%s (|run - fp64| %.3e, |fp32 - fp64| %.3e, layer scale %.3e)" % ((n,) + self.detail[n])
        assert not self.failures, "%s: beyond max(%g x |fp32 - fp64|, %g x S): %s" % (
            self.what, MARGIN, FLOOR, "; ".join(one(n) for n in self.failures))


def compare_net(report, prefix, run, ref32, ref64):
    """Per tensor of one network: `run`, `ref32`, `ref64` are {fcN.weight / fcN.bias: tensor}."""
    for i in range(1, len(ref64) // 2 + 1):
        names = ["fc%d.weight" % i, "fc%d.bias" % i]
        scale = max(ref64[n].abs().max().item() for n in names)
        for n in names:
            r = run[n].detach().cpu().double()
            report.add(prefix + n, (r - ref64[n]).abs().max().item(), (ref32[n].double() - ref64[n]).abs().max().item(),
                       scale, bool(torch.isfinite(r).all()))


# ------------------------------------------------------------------------------------------------ D gradient
def reference_d_grads(g0, d_at, codes, actions, noise, d_masks, inv_m=None):
    """{dtype: (D gradient, D loss, action_hat)} from generator `g0` and discriminator `d_at`, hand-written, with the
    run's leaky-ReLU decisions: d_masks = (real, fake), three masks each; real per distinct row [FLAT,.] (the fused
    step's de-duplicated real pass) or per row [M,.]."""
    out = {}
    k = noise.shape[1]
    real, fake = [[m.detach().cpu() for m in part] for part in d_masks]
    if real[0].shape[0] == codes.shape[0] and k > 1:
        real = [torch.repeat_interleave(m, k, dim=0) for m in real]
    for dt in (torch.float32, torch.float64):
        sm = O.StepMath(to_dtype(g0, dt), to_dtype(d_at, dt))
        sm.g_forward(codes.to(dt), actions.to(dt), noise.to(dt))
        m_rows = sm.action_hat.shape[0]
        im = 1.0 / m_rows if inv_m is None else inv_m
        lr_, acts_r = O.d_forward(sm.d, sm.actions_rep, sm.codes_rep, keep=True)
        lf_, acts_f = O.d_forward(sm.d, sm.action_hat, sm.codes_rep, keep=True)
        d_loss = (O.bce_with_logits_sum(lr_, 1.0) + O.bce_with_logits_sum(lf_, 0.0)) * im
        gr, _ = O._mlp_backward(sm.d, inject(acts_r, real), O.bce_with_logits_grad(lr_, 1.0, im), "lrelu", False)
        gf, _ = O._mlp_backward(sm.d, inject(acts_f, fake), O.bce_with_logits_grad(lf_, 0.0, im), "lrelu", False)
        out[dt] = (OrderedDict((n, gr[n] + gf[n]) for n in gr), d_loss.item(), sm.action_hat)
    return out


def adjudicate_d(report, d_grad_run, g0, d_at, codes, actions, noise, d_masks, inv_m=None):
    """The run's D gradient (flat or per tensor) at discriminator `d_at`.  Returns the references (D loss, action_hat)."""
    ref = reference_d_grads(g0, d_at, codes, actions, noise, d_masks, inv_m)
    g64 = ref[torch.float64][0]
    compare_net(report, "d.", _as_dict(d_grad_run, g64), ref[torch.float32][0], g64)
    return ref


# ------------------------------------------------------------------------------------------------ G gradient
def injected_g_grads(g0, codes, noise, d_action_run, masks_run):
    """{dtype: G gradient} = J_G(run's masks)^T . d_action(run): G's backward from the run's dLoss/d action_hat."""
    out = {}
    masks = [m.detach().cpu() for m in masks_run]
    for dt in (torch.float32, torch.float64):
        g = to_dtype(g0, dt)
        _, acts = O.g_forward(g, O.make_generator_input(codes.to(dt), noise.to(dt)), keep=True)
        out[dt], _ = O._mlp_backward(g, inject(acts, masks), d_action_run.detach().cpu().to(dt), "relu", False)
    return out


# ------------------------------------------------------------------------------------------------ d_action
def compare_d_action(report, d_action_run, nd_grad_run, action_hat_run, d_post, codes, k, inv_m):
    """The run's dLoss/d action_hat against dBCE/d action_hat through `d_post` + the run's nd_grad, both oracles
    evaluated at the run's action_hat: only D's own rounding can then decide a leaky ReLU differently, and the rows
    where it can are left out (and counted).  Returns the fp64 G loss."""
    res = {}
    for dt in (torch.float32, torch.float64):
        d = to_dtype(d_post, dt)
        x = action_hat_run.detach().cpu().to(dt)
        lg, acts = O.d_forward(d, x, torch.repeat_interleave(codes.to(dt), k, dim=0), keep=True)
        _, dx = O._mlp_backward(d, acts, O.bce_with_logits_grad(lg, 1.0, inv_m), "lrelu", True)
        pre = [torch.where(a > 0, a, a / O.LRELU_SLOPE) for a in acts[1:]]
        res[dt] = (dx[:, :O.ACTION_DIM] + nd_grad_run.detach().cpu().to(dt), pre, O.bce_with_logits_sum(lg, 1.0).item() * inv_m)
    (da32, pre32, _), (da64, pre64, g_loss) = res[torch.float32], res[torch.float64]
    keep = torch.ones(da64.shape[0], dtype=torch.bool)
    for p32, p64 in zip(pre32, pre64):
        tau = MARGIN * (p32.double() - p64).abs().max().item()
        report.tau_d = max(report.tau_d, tau)
        keep &= ~(p64.abs() < tau).any(dim=1)
    report.left_out_d = 1.0 - keep.double().mean().item()
    report.cap("d_action", report.left_out_d)
    run = d_action_run.detach().cpu().double()
    report.add("d_action", (run - da64)[keep].abs().max().item(), (da32.double() - da64)[keep].abs().max().item(),
               da64[keep].abs().max().item(), bool(torch.isfinite(run).all()))
    return g_loss


# ------------------------------------------------------------------------------------------------ nd_grad
def hinge_terms(x, z):
    """h_ij = 0.8 z~_ij - x~_ij of diversity.py:40 as ndiv_loss_and_grad forms it; x [FLAT,K,C], z [FLAT,K,nz]."""
    dx, dz = O.compute_pairwise(x), O.compute_pairwise(z)
    return O.HINGE_ALPHA * dz / dz.sum(dim=2, keepdim=True) - dx / dx.sum(dim=2, keepdim=True)


def compare_nd_grad(report, nd_grad_run, action_hat_run, noise, factor):
    """The run's factor * dNDiv/d action_hat against both oracles evaluated at the run's own action_hat: only NDiv's
    own rounding can then flip a hinge term, and the rows where it can are left out (and counted).  Returns the fp64
    NDiv loss at that action_hat."""
    flat, k = noise.shape[0], noise.shape[1]
    res = {}
    for dt in (torch.float32, torch.float64):
        x = action_hat_run.detach().cpu().to(dt).reshape(flat, k, -1)
        z = noise.detach().cpu().to(dt)
        loss, grad = O.ndiv_loss_and_grad(x, z)
        res[dt] = (hinge_terms(x, z), factor * grad, loss.item())
    (h32, nd32, _), (h64, nd64, pair_div) = res[torch.float32], res[torch.float64]
    tau = MARGIN * (h32.double() - h64).abs().max().item()
    off = ~torch.eye(k, dtype=torch.bool)[None]
    keep = ~((h64.abs() < tau) & off).flatten(1).any(dim=1)
    report.tau = tau
    report.left_out = 1.0 - keep.double().mean().item()
    report.cap("nd_grad", report.left_out)
    run = nd_grad_run.detach().cpu().double().reshape(flat, k, -1)
    report.add("nd_grad", (run - nd64)[keep].abs().max().item(), (nd32.double() - nd64)[keep].abs().max().item(),
               nd64[keep].abs().max().item(), bool(torch.isfinite(run).all()))
    return pair_div


# ------------------------------------------------------------------------------------------------ the whole step
def adjudicate(what, run, g0, d0, codes, actions, noise, factor, inv_m=None):
    """`run`: what one step exposes -- "d_grad", "g_grad" (flat or per tensor), "d_post" (post-update D, likewise),
    "action_hat" [M,4], "masks" (h_i > 0 of G's four saved activations, [M,width] each), "d_masks" (h_i > 0 of D's three
    saved activations of the D step as (real, fake), see reference_d_grads), "nd_grad" [M,4] (already scaled by `factor`),
    "d_action" [M,4] (dLoss/d action_hat that G's backward started from).  g0, d0: the pre-step parameters; codes
    [FLAT,256], actions [FLAT,4], noise [FLAT,K,nz] on the CPU; inv_m: 1 / the global row count (None: this batch's
    own).  Returns a Report; nothing is asserted here."""
    rep = Report(what)
    k = noise.shape[1]
    im = 1.0 / (noise.shape[0] * k) if inv_m is None else inv_m
    d_ref = adjudicate_d(rep, run["d_grad"], g0, d0, codes, actions, noise, run["d_masks"], im)
    ref = injected_g_grads(g0, codes, noise, run["d_action"], run["masks"])
    g64 = ref[torch.float64]
    compare_net(rep, "g.", _as_dict(run["g_grad"], g64), ref[torch.float32], g64)
    g_loss = compare_d_action(rep, run["d_action"], run["nd_grad"], run["action_hat"], _as_dict(run["d_post"], d0), codes, k, im)
    pair_div = compare_nd_grad(rep, run["nd_grad"], run["action_hat"], noise, factor)
    rep.losses64 = (d_ref[torch.float64][1], g_loss, pair_div)
    rep.action_hat64 = d_ref[torch.float64][2]
    return rep


def stand_in_run(g0, d0, codes, actions, noise, factor, inv_m=None, dtype=torch.float32):
    """The hand-written StepMath in `dtype` as "the run": everything adjudicate() wants, plus the StepMath itself
    (its saved activations and d_action are what the planted errors are made of)."""
    sm = O.StepMath(to_dtype(g0, dtype), to_dtype(d0, dtype), pairwise_div_factor=factor)
    sm.g_forward(codes.to(dtype), actions.to(dtype), noise.to(dtype))
    d_masks = tuple([a > 0 for a in O.d_forward(sm.d, x, sm.codes_rep, keep=True)[1][1:]]
                    for x in (sm.actions_rep, sm.action_hat))
    d_grad = sm.d_grads(inv_m)
    sm.apply_d(d_grad)
    g_grad = sm.g_grads(inv_m)
    flat, k = noise.shape[0], noise.shape[1]
    nd = factor * O.ndiv_loss_and_grad(sm.action_hat.reshape(flat, k, -1), sm.noise)[1].reshape(flat * k, -1)
    run = {"d_post": to_dtype(sm.d, dtype), "action_hat": sm.action_hat.clone(), "masks": [a > 0 for a in sm.g_acts[1:]],
           "d_masks": d_masks, "nd_grad": nd, "d_action": sm.out["d_action"].clone(),
           "d_grad": OrderedDict((n, v.clone()) for n, v in d_grad.items()),
           "g_grad": OrderedDict((n, v.clone()) for n, v in g_grad.items())}
    return run, sm
