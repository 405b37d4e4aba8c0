"""GPU: the D and G gradients of the fused, graph-replayed GAN step at every launch plan the host code chooses, held per
parameter tensor to the fp64 oracle with the run's own discontinuous decisions injected into the references
(tests/step_grad_common.py, proved on the CPU by tests/test_step_grad_adjudication_host.py).

Each case: init_params(0, nz), one synthetic batch, GanTrainer(use_graph=True) -- graph replay without a collective is
the shipped path -- one step(), then what the step leaves behind is read: d_grad / g_grad (k_reduce_adam stores the summed
gradient in fused mode too), the post-update D, action_hat, and through GanTrainer.activation G's and D's saved
activations (their signs are the run's ReLU / leaky-ReLU decisions), nd_grad and d_action (dLoss/d action_hat).
Rule per tensor: max |run - fp64| <= max(4 x max |fp32 - fp64|, 1e-5 x S), S = the layer's largest fp64 gradient entry.
 * D gradient: both oracles with the run's leaky-ReLU decisions;
 * G gradient: J_G(run's masks)^T . d_action(run) in both oracles;
 * d_action against dBCE/d action_hat through the run's post-update D + the run's nd_grad, at the run's action_hat, rows
   with a D pre-activation inside tau_D = 4 x max |pre32 - pre64| left out;
 * nd_grad against NDiv at the run's action_hat, FLAT rows with a hinge term inside tau = 4 x max |h32 - h64| left out;
 * at most 3 % of the rows left out by either.
Every case runs at pairwise_div_factor 0.1 and 0 (the same kernels; without NDiv's 1e3 x scale d_action, the BCE path
through the updated D, is held to 1e-5 of its own size), and the three losses and action_hat are held to the fp64 oracle
at the suite's 1e-4 bounds, so that no case passes on the gradients of a wrong forward.

The tests prove parity; which plan runs at each shape -- the plan beside it below -- is asserted on the CPU by
tests/test_step_plan_host.py, together with these shapes reaching every kernel variant and every branch of the plan.

measured on MI355X (30 cases, 8 s; worst |run - fp64| / bound over the cases, 1 = the bound):
  D gradient   0.70 (fc3.bias at B 128 / K 32, k_wgrad_wide), otherwise <= 0.40; repeat D step 0.35 (fc2.bias)
  G gradient   0.88 (fc5.bias at B 40 / K 6 / nz 1, factor 0.1; fc5.* lead at factor 0.1 in every case, 0.25 .. 0.88);
               at factor 0 <= 0.02 in every case
  d_action     <= 0.054 at factor 0 (the 1e-5 x S floor decides), <= 0.004 at factor 0.1
  nd_grad      <= 0.019
  tau (hinge)  8.1e-8 (K 32) .. 5.6e-7; FLAT rows left out: 0.89 % at B 128 / K 32, 0.07 % at B 200 / K 3, none elsewhere
  tau_D        3.0e-6 .. 4.6e-6; rows left out: 0 .. 0.45 %
Before D's decisions were taken over, one leaky-ReLU unit decided differently put D's fc1..fc3 tensors at 2.8 .. 69 x the
bound at B 25 / K 6, B 128 / K 32 and B 672 / K 6 and at 112 .. 699 x in the repeat D step, and the G gradient through
the references' own dBCE at 1.1 .. 56 x at factor 0 (B 64 and B 392 / K 6); fc4 of D, which no decision enters, was
at <= 0.43 throughout.  No kernel or host fix was needed.
"""
import pytest
import torch

import step_grad_common as C
from oracle import gan_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (B, K, nz): FLAT = 7 B rows, M = FLAT K; rows are padded to 32.  "G" / "D": chunk counts heavy/light of k_wgrad over
# pad(M) resp. pad(FLAT) + pad(M) rows; "A" / "B": workgroups of k_phase_a / k_phase_b and their template.
SHAPES = [
    # M 245 (ragged: not a multiple of 16), 256 / 320 rows: G uniform 4, D uniform 5 (fewer than 64 rows per chunk
    # otherwise); A 20, B 16 workgroups, 96-register rings; seg_per_tile 4
    (5, 7, 2),
    # M 1,050, 1,056 / 1,248 rows: G below 1,536 rows, uniform 16; D 8/8; one real tile per helper workgroup (66 tiles)
    (25, 6, 2),
    # config 2 -- M 2,688, 2,688 / 3,136 rows: G 24/12, D 8/8; paired real tiles (168 tiles); A 196 workgroups, 96 rings
    (64, 6, 2),
    # M 2,184, 2,208 / 2,592 rows: the same with a ragged last tile (138 tiles)
    (52, 6, 2),
    # M 3,024, 3,040 / 3,552 rows: stacked passes (190 + 32 = 222 workgroups, still <= 256)
    (72, 6, 2),
    # M 4,116, 4,128 / 4,832 rows: first size with > 256 tiles (A 302, B 258): small rings, NR = 4; G 24/12, D 32/8
    (98, 6, 2),
    # M 4,200, 4,224 / 5,632 rows: small rings with NR = 0 (K < 6); seg_per_tile 7; D 32/8
    (200, 3, 2),
    # M 5,376, 5,376 / 5,568 rows: small rings with NR = 1 (K % 16 == 0); seg_per_tile 2; D 32/8
    (24, 32, 2),
    # M 16,464, 16,480 / 19,232 rows: both networks on the uniform plan from 16,384 rows (32 chunks); NR = 4
    (392, 6, 2),
    # config-5 shard -- M 28,672, 28,672 / 29,568 rows: k_wgrad_wide for D.fc3 and G.fc4 (64 chunks each); NR = 1
    (128, 32, 2),
    # M 28,224, 28,224 / 32,928 rows: k_wgrad_wide at K = 6 (NR = 4), 64 chunks each as well
    (672, 6, 2),
    # M 1,400, 1,408 / 1,696 rows: noise_dim 5 -- NDiv as a launch of its own in phase B, fc1 width 261 (scalar weight
    # path); G uniform 16, D 8/8; seg_per_tile 5
    (40, 5, 5),
    # M 1,680, 1,696 / 1,984 rows: noise_dim 1; G 24/12, D 8/8
    (40, 6, 1),
]
FACTORS = [0.1, 0.0]
# synthetic_batch seed per shape (7 unless listed).  (24, 32, 2): with seed 7 the run left out 5 of the 168 FLAT rows of
# the nd_grad check (2.98 %), one row from the cap; seed 13 has a third as many hinge terms within 2 tau of zero.
SEEDS = {(24, 32, 2): 13}

_inputs = {}


def _case_inputs(batch, k, nz):
    """Parameters and batch of a shape: made once, shared by the cases of that shape (both factors, the data-parallel
    scaling and the repeat D step read them and leave them unchanged).  The references depend on the run's decisions."""
    key = (batch, k, nz)
    if key not in _inputs:
        torch.set_num_threads(16)
        g0, d0 = O.init_params(0, nz)
        codes, actions, noise = O.synthetic_batch(SEEDS.get(key, 7), batch, k, nz, steps=1)
        _inputs[key] = (g0, d0, codes, actions, noise[0])
    return _inputs[key]


def _load_modules(g, d, nz):
    from ndivplanning_amd.models.gan import Decoder, Discriminator
    dec, dis = Decoder(nz), Discriminator()
    dec.load_state_dict(g)
    dis.load_state_dict(d)
    return dec.to(DEV), dis.to(DEV)


def _d_masks(tr, repeat=False):
    pairs = [tr.activation(n, repeat=repeat) for n in C.D_ACTIVATIONS]
    return [(r > 0).cpu() for r, _ in pairs], [(f > 0).cpu() for _, f in pairs]


def _exposed(tr):
    """What a finished step leaves behind, on the CPU."""
    torch.cuda.synchronize()
    m = tr.m
    return {"d_post": tr.d_flat.detach().cpu().clone(), "action_hat": tr.action_hat[:m].cpu(),
            "masks": [(tr.activation(n) > 0).cpu() for n in C.G_ACTIVATIONS], "d_masks": _d_masks(tr),
            "nd_grad": tr.activation("nd_grad").cpu(), "d_action": tr.activation("d_action").cpu(),
            "d_grad": tr.d_grad.cpu(), "g_grad": tr.g_grad.cpu()}


def _run_and_adjudicate(what, batch, k, nz, factor, inv_scale=1):
    from ndivplanning_amd.trainer import GanTrainer
    g0, d0, codes, actions, noise = _case_inputs(batch, k, nz)
    flat = codes.shape[0]
    inv_m = 1.0 / (inv_scale * flat * k)
    dec, dis = _load_modules(g0, d0, nz)
    tr = GanTrainer(dec, dis, flat=flat, num_sample=k, pairwise_div_factor=factor, flat_global=inv_scale * flat,
                    use_graph=True)
    tr.step(codes.to(DEV), actions.to(DEV), noise.to(DEV))
    run = _exposed(tr)
    rep = C.adjudicate(what, run, g0, d0, codes, actions, noise, factor, inv_m)
    print(rep.line())
    rep.assert_ok()
    assert rep.left_out <= C.MAX_LEFT_OUT and rep.left_out_d <= C.MAX_LEFT_OUT
    d_loss, g_loss, pd = tr.losses()
    ref_d, ref_g, ref_pd = rep.losses64
    assert abs(d_loss - ref_d) <= 1e-4 and abs(g_loss - ref_g) <= 1e-4, (what, d_loss, ref_d, g_loss, ref_g)
    assert abs(pd - ref_pd) <= 1e-4 * max(1.0, abs(ref_pd)), (what, pd, ref_pd)
    err = (run["action_hat"].double() - rep.action_hat64).abs().max().item()
    assert err <= 1e-4, "%s: action_hat max |diff| %.3e" % (what, err)
    return rep


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("batch,k,nz", SHAPES)
def test_step_gradients_at_every_launch_plan(batch, k, nz, factor):
    _run_and_adjudicate("B %d K %d nz %d factor %g" % (batch, k, nz, factor), batch, k, nz, factor)


@pytest.mark.parametrize("factor", FACTORS)
def test_step_gradients_with_data_parallel_scaling(factor):
    """Config 2's shard of a global batch twice its size: BCE terms are means over the global row count
    (inv_m = 1 / (2 M)), NDiv is a sum and is not scaled."""
    _run_and_adjudicate("B 64 K 6 flat_global 2 x flat factor %g" % factor, 64, 6, 2, factor, inv_scale=2)


@pytest.mark.parametrize("factor", FACTORS)
def test_repeat_d_step_gradient(factor):
    """discrim_steps = 2 at config 2: the second D step runs the two-pass k_d over 2 x 2,688 rows without segment sums,
    which selects D's 32/8 plan.  Non-fused and eager through _segments(): after the first D update d_flat is read,
    the second d_grads segment runs, and its gradient is adjudicated against both oracles at that d_flat (with the
    leaky-ReLU decisions that segment left behind: M real and M fake rows)."""
    from ndivplanning_amd.trainer import GanTrainer
    batch, k, nz = 64, 6, 2
    g0, d0, codes, actions, noise = _case_inputs(batch, k, nz)
    dec, dis = _load_modules(g0, d0, nz)
    tr = GanTrainer(dec, dis, flat=codes.shape[0], num_sample=k, pairwise_div_factor=factor, discrim_steps=2,
                    use_graph=False, reduce_fn=lambda grad: None)
    tr.codes.copy_(codes)
    tr.actions.copy_(actions)
    tr.noise.copy_(noise)
    segs = [fn for fn, _ in tr._segments(False)]        # d_grads, D Adam, d_grads (repeat), D Adam, g_grads, G Adam
    assert len(segs) == 6
    rep = C.Report("repeat D step, factor %g" % factor)
    with torch.cuda.device(tr.device):
        segs[0]()
        torch.cuda.synchronize()
        first, first_masks = tr.d_grad.cpu(), _d_masks(tr)
        segs[1]()
        torch.cuda.synchronize()
        d_mid = C.split_flat(tr.d_flat.detach().cpu().clone(), d0)
        segs[2]()
        torch.cuda.synchronize()
        second, second_masks = tr.d_grad.cpu(), _d_masks(tr, repeat=True)
    assert not torch.equal(first, second)
    C.adjudicate_d(rep, second, g0, d_mid, codes, actions, noise, second_masks)
    print(rep.line())
    rep.assert_ok()
    # the first D step of the same run, for the record of this mode (non-fused, eager)
    rep1 = C.Report("first D step, non-fused, factor %g" % factor)
    C.adjudicate_d(rep1, first, g0, d0, codes, actions, noise, first_masks)
    print(rep1.line())
    rep1.assert_ok()
