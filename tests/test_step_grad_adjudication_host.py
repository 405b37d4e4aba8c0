"""CPU: the adjudicator of the GAN step's gradients (tests/step_grad_common.py) proved without a GPU.  The hand-written
fp32 StepMath is "the run": its action_hat, activations, post-update D, gradients and NDiv gradient are all at hand.
The adjudicator must accept it -- as it stands and summed in another order -- at pairwise_div_factor 0.1 and 0, and must
reject each planted error and name the tensor; and the contrast that is the reason for the mask injection is asserted.
Also here: the layout of the accessor the GPU tests read the run's decisions through (ndp_step_workspace_offset)."""
import ctypes
from collections import OrderedDict

import pytest
import torch

import step_grad_common as C
from oracle import gan_oracle as O

SHAPES = [(25, 6, 2), (64, 6, 2), (24, 32, 2), (40, 5, 5)]
G_NAMES = ["g.fc%d.%s" % (i, p) for i in range(1, 6) for p in ("weight", "bias")]
D_NAMES = ["d.fc%d.%s" % (i, p) for i in range(1, 5) for p in ("weight", "bias")]

_cases = {}


def _case(batch, k, nz, factor):
    """One stand-in run per shape and factor, shared by the tests below and left unchanged by them."""
    key = (batch, k, nz, factor)
    if key not in _cases:
        torch.set_num_threads(16)
        g0, d0 = O.init_params(0, nz)
        codes, actions, noise = O.synthetic_batch(7, batch, k, nz, steps=1)
        run, sm = C.stand_in_run(g0, d0, codes, actions, noise[0], factor)
        _cases[key] = (g0, d0, codes, actions, noise[0], run, sm)
    return _cases[key]


def _adjudicate(case, factor, **changed):
    g0, d0, codes, actions, noise, run, _ = case
    return C.adjudicate("stand-in", dict(run, **changed), g0, d0, codes, actions, noise, factor)


def _chunked_run(case, factor, chunk):
    """The same step, its weight gradients summed over row chunks (split-K, as the kernels do): a second correct fp32
    implementation whose rounding differs from the oracle's."""
    g0, d0, codes, actions, noise, run, sm = case
    m = sm.action_hat.shape[0]
    g_grad = OrderedDict((n, torch.zeros_like(v)) for n, v in run["g_grad"].items())
    for r0 in range(0, m, chunk):
        part, _ = O._mlp_backward(sm.g, [a[r0:r0 + chunk] for a in sm.g_acts], sm.out["d_action"][r0:r0 + chunk], "relu", False)
        for n in g_grad:
            g_grad[n] += part[n]
    return g_grad


@pytest.mark.parametrize("factor", [0.1, 0.0])
@pytest.mark.parametrize("batch,k,nz", SHAPES)
def test_a_correct_fp32_run_is_accepted(batch, k, nz, factor):
    case = _case(batch, k, nz, factor)
    rep = _adjudicate(case, factor)
    print(rep.line())
    rep.assert_ok()
    assert sorted(rep.ratios) == sorted(G_NAMES + D_NAMES + ["nd_grad", "d_action"])
    assert rep.left_out <= C.MAX_LEFT_OUT and rep.left_out_d <= C.MAX_LEFT_OUT
    rep = _adjudicate(case, factor, g_grad=_chunked_run(case, factor, 48))
    print(rep.line())
    rep.assert_ok()


@pytest.mark.parametrize("factor", [0.1, 0.0])
@pytest.mark.parametrize("batch,k,nz", SHAPES)
def test_planted_errors_are_rejected_by_name(batch, k, nz, factor):
    case = _case(batch, k, nz, factor)
    g0, d0, codes, actions, noise, run, sm = case
    # (a) one layer's weight gradient scaled by 63/64, in either network
    for net, key, name in (("g_grad", "fc3.weight", "g.fc3.weight"), ("g_grad", "fc1.weight", "g.fc1.weight"),
                           ("d_grad", "fc2.weight", "d.fc2.weight"), ("d_grad", "fc4.weight", "d.fc4.weight")):
        bad = OrderedDict(run[net])
        bad[key] = run[net][key] * (63.0 / 64.0)
        rep = _adjudicate(case, factor, **{net: bad})
        assert rep.failures == [name], (name, rep.failures)
        with pytest.raises(AssertionError, match=name.replace(".", r"\.")):
            rep.assert_ok()
    # (b) one 16-row tile missing from G.fc2.weight
    m = sm.action_hat.shape[0]
    r0 = (m // 32) * 16
    tile, _ = O._mlp_backward(sm.g, [a[r0:r0 + 16] for a in sm.g_acts], sm.out["d_action"][r0:r0 + 16], "relu", False)
    bad = OrderedDict(run["g_grad"])
    bad["fc2.weight"] = run["g_grad"]["fc2.weight"] - tile["fc2.weight"]
    rep = _adjudicate(case, factor, g_grad=bad)
    assert rep.failures == ["g.fc2.weight"], rep.failures
    # (e) the real pass of the D gradient weighted 1/K: the de-duplication's scale dropped
    lr_, acts_r = O.d_forward(d0, sm.actions_rep, sm.codes_rep, keep=True)
    gr, _ = O._mlp_backward(d0, acts_r, O.bce_with_logits_grad(lr_, 1.0, 1.0 / m), "lrelu", False)
    bad = OrderedDict((n, run["d_grad"][n] - gr[n] * (1.0 - 1.0 / k)) for n in gr)
    rep = _adjudicate(case, factor, d_grad=bad)
    assert sorted(rep.failures) == sorted(D_NAMES), rep.failures
    if factor == 0.0:
        return                                     # (c) and (d) change nothing without NDiv
    # (c) nd_grad of one FLAT row negated: the nd_grad check fails (and d_action, made with the right one, no longer is
    # dBCE + nd_grad; nothing else moves)
    kept = _adjudicate(case, factor)
    flat = noise.shape[0]
    h64 = C.hinge_terms(run["action_hat"].double().reshape(flat, k, -1), noise.double())
    off = ~torch.eye(k, dtype=torch.bool)[None]
    compared = (~((h64.abs() < kept.tau) & off).flatten(1).any(dim=1)).nonzero().reshape(-1)
    row = int(compared[len(compared) // 2])
    nd = run["nd_grad"].clone()
    nd[row * k:(row + 1) * k] *= -1.0
    rep = _adjudicate(case, factor, nd_grad=nd)
    assert rep.failures == ["d_action", "nd_grad"], rep.failures
    # (d) the G gradient computed without adding nd_grad (NDiv is translation invariant: nd_grad sums to zero over the K
    # samples of a row, so fc5.bias, the plain sum of d_action, is the one tensor that cannot see it)
    bad, _ = O._mlp_backward(sm.g, sm.g_acts, sm.out["d_action"] - run["nd_grad"], "relu", False)
    rep = _adjudicate(case, factor, g_grad=bad)
    assert sorted(rep.failures) == sorted(G_NAMES[:-1]), rep.failures
    # (f) nd_grad never added to dLoss/d action_hat, and G's backward run from that: the G gradient is consistent with
    # its d_action, which is the one that is wrong
    rep = _adjudicate(case, factor, g_grad=bad, d_action=sm.out["d_action"] - run["nd_grad"])
    assert rep.failures == ["d_action"], rep.failures
    # (g) one leaky-ReLU decision of D's fake pass taken the other way *without* the gradient following it: as large as
    # a decision the run really took differently would be if the references did not take it over
    lf_, acts_f = O.d_forward(d0, sm.action_hat, sm.codes_rep, keep=True)
    row, unit = divmod(int(acts_f[3].abs().argmin()), acts_f[3].shape[1])         # the one nearest to deciding otherwise
    real, fake = run["d_masks"]
    fake = [f.clone() for f in fake]
    fake[2][row, unit] = ~fake[2][row, unit]
    rep = _adjudicate(case, factor, d_masks=(real, fake))
    assert rep.failures and all(n.startswith("d.fc") and n[4] in "123" for n in rep.failures), rep.failures
    assert "d.fc3.bias" in rep.failures


def test_without_injection_the_reference_is_a_hundred_times_looser():
    """Why the injection exists (FLAT = 448, K = 6): the plain fp32 and fp64 steps, each taking its own ReLU and hinge
    decisions, differ by ~0.6 in the G gradient; with the run's decisions injected into both, by ~1e-5."""
    g0, d0, codes, actions, noise, run, sm = _case(64, 6, 2, 0.1)
    plain = O.StepMath(C.to_dtype(g0, torch.float64), C.to_dtype(run["d_post"], torch.float64), pairwise_div_factor=0.1)
    plain.g_forward(codes.double(), actions.double(), noise.double())
    loose = (C.flatten(plain.g_grads()) - C.flatten(run["g_grad"]).double()).abs().max().item()
    ref = C.injected_g_grads(g0, codes, noise, run["d_action"], run["masks"])
    tight = (C.flatten(ref[torch.float64]) - C.flatten(ref[torch.float32]).double()).abs().max().item()
    print("G gradient |fp32 - fp64| without injection %.3e, with %.3e" % (loose, tight))
    assert loose >= 100.0 * tight and tight > 0.0


def test_step_workspace_offsets():
    """ndp_step_workspace_offset: G's h1..h4 back to back with a stride of the padded M, behind them d_action, D's
    h1..h3 in both layouts (which share their region) and nd_grad, all inside ndp_step_workspace_floats, none
    overlapping another; bad configurations and indices give -1."""
    from ndivplanning_amd import _build, _capi
    _build.build()
    lib = _capi.load()
    widths = (128, 64, 128, 256, 4, 4, 64, 128, 256, 64, 128, 256)
    for flat, k, nz in ((35, 7, 2), (448, 6, 2), (168, 32, 2), (280, 5, 5), (1, 1, 1), (4704, 6, 2)):
        cfg = _capi.StepConfig(noise_dim=nz, num_sample=k, flat=flat)
        total = lib.ndp_step_workspace_floats(ctypes.byref(cfg))
        mpad = _capi.pad_rows(flat * k)
        rows = [mpad] * 6 + [_capi.pad_rows(flat) + mpad] * 3 + [2 * mpad] * 3
        offs = [lib.ndp_step_workspace_offset(ctypes.byref(cfg), t) for t in range(12)]
        assert offs[0] >= 0 and all(o % 4 == 0 for o in offs)
        order = [0, 1, 2, 3, 5, 6, 7, 8, 4]                                                  # as they lie in the workspace
        assert all(offs[b] > offs[a] for a, b in zip(order, order[1:]))                      # increasing
        assert [offs[t + 1] - offs[t] for t in range(3)] == [mpad * w for w in widths[:3]]   # row stride = padded M
        assert [offs[t + 1] - offs[t] for t in (6, 7)] == [rows[6] * w for w in widths[6:8]]
        assert [offs[t + 1] - offs[t] for t in (9, 10)] == [rows[9] * w for w in widths[9:11]]
        assert all(offs[a] + rows[a] * widths[a] <= offs[b] for a, b in zip(order, order[1:]))   # disjoint
        assert offs[8] + rows[8] * widths[8] <= offs[4] and offs[11] + rows[11] * widths[11] <= offs[4]
        assert offs[5] + mpad * 4 <= offs[9]                                                 # the repeat layout: same region
        assert all(o + r * w <= total for o, r, w in zip(offs, rows, widths))                # inside the workspace
        assert lib.ndp_step_workspace_offset(ctypes.byref(cfg), 12) == -1
        assert lib.ndp_step_workspace_offset(ctypes.byref(cfg), -1) == -1
    assert lib.ndp_step_workspace_offset(None, 0) == -1
    for bad in (dict(noise_dim=2, num_sample=0, flat=8), dict(noise_dim=2, num_sample=257, flat=8),
                dict(noise_dim=2, num_sample=6, flat=0), dict(noise_dim=0, num_sample=6, flat=8),
                dict(noise_dim=17, num_sample=6, flat=8), dict(noise_dim=2, num_sample=6, flat=1 << 40)):
        cfg = _capi.StepConfig(**bad)
        assert lib.ndp_step_workspace_offset(ctypes.byref(cfg), 0) == -1, bad
