"""GPU: the training kernels from a mid-training state (tests/trained_state.py), and Adam from resumed moments.

Every other training-mode test starts where `weight_init` leaves the networks: all biases 0, BatchNorm weight 1 / bias 0,
running statistics 0 / 1, batch counter 0, Adam moments 0.  There a bias epilogue adds zeros, gamma and beta cannot be
mis-indexed visibly, the momentum update has no old value to forget, torch's running_mean carries no pre-BatchNorm bias
and Adam's first update is lr x sign(g).  Here none of that holds.

Comparison rule (tests/test_gpu_forward_model.py, tests/test_gpu_forward_rollout.py): the ReLU decisions of the run under
test are injected into the fp32 and the fp64 CPU oracle, and the kernels' error against the fp64 oracle may be at most
max(floor, 2 x the fp32 oracle's error against it).  Floors: loss 1e-5 x max(1, loss), residual 2e-5 absolute, gradients
2e-5 of the tensor's norm (those tests' own), running statistics 1e-6 x the tensor's largest magnitude.

The autoencoder step and the rollout / input-gradient passes from the same state are cases of the existing tests
(tests/test_gpu_autoencoder.py, tests/test_gpu_forward_rollout.py: `trained`)."""
import functools

import numpy as np
import pytest
import torch

import trained_state as TS
from oracle import forward_model_oracle as FO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR, BETAS, EPS = 2e-4, (0.5, 0.999), 1e-8

# Biases of the layers a BatchNorm follows: zero gradient but for rounding (tests/test_gpu_forward_model.py)
NOISE_BIASES = tuple("%s.bias" % n for n in ("encoder.conv1", "encoder.conv2", "encoder.conv3", "decoder.deconv1",
                                             "decoder.deconv2", "decoder.deconv3", "decoder.deconv4", "decoder.deconv5",
                                             "decoder.deconv6", "decoder.conv_refine_1"))
UNUSED_BN = ("encoder.conv4_bn", "encoder.conv5_bn")
BN_LEAVES = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def _inputs(data_seed, n):
    gen = torch.Generator().manual_seed(data_seed)
    frames = torch.rand(n, 3, 3, 128, 128, generator=gen) * 2.0 - 1.0
    actions = torch.rand(n, 3, 4, generator=gen) * 2.0 - 1.0
    return frames, actions


def _trained_fm_trainer(seed, n, **kw):
    from ndivplanning_amd.forward_trainer import ForwardModelTrainer
    from ndivplanning_amd.models import forward_encoder as FE
    state = TS.trained_like(FO.init_forward_model_state(seed), seed)
    model = FE.ForwardAutoencoder()
    model.load_state_dict(state)
    model = model.to(DEV).train()
    return ForwardModelTrainer(model, batch=n, lr=LR, **kw), state


def _to64(state):
    return {k: (v.detach().double() if v.is_floating_point() else v.clone()) for k, v in state.items()}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _maxabs(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


# ------------------------------------------------------------------------------------------ (a) forward-model step
@pytest.mark.parametrize("n", [1, 3, 16, 65])   # 16: deconv5's four parity classes in one workgroup; 65: 128-row tiles, k_fm_rows_cls
def test_forward_model_step_from_a_trained_state(n):
    """One training iteration (n = 3: a second, teacher-forced one) from trained_like(): loss, residual, every gradient --
    the four biases no BatchNorm follows and every BatchNorm weight / bias among them --, every running_mean / running_var
    element after the pass (the means carry the N(0, 0.1) convolution biases: a kernel that leaves the bias out of its
    statistics fails here and nowhere else) and the batch counters."""
    torch.set_num_threads(16)
    tr, state = _trained_fm_trainer(40 + n, n, keep_residual=True)
    loaded = {k: v.detach().clone() for k, v in state.items()}
    state64 = _to64(state)
    oracle = FO.ForwardModelTrainer(state, lr=LR)
    frames, actions = _inputs(50 + n, n)
    worst = {"grad": (-1.0, 0.0, 0.0, ""), "running": (-1.0, 0.0, 0.0, "")}       # (share of the bound, kernels, fp32 oracle, what)
    tracked = TS.BATCHES_TRACKED
    for it in range(2 if n == 3 else 1):
        cur, fut, act = frames[:, it].contiguous(), frames[:, it + 1].contiguous(), actions[:, it].contiguous()
        if it == 1:                                            # teacher forcing: the oracle's parameters and statistics
            with torch.no_grad():
                tr.model.load_state_dict({k: v.detach() for k, v in state.items()})
            tr.load_from_module()
            state64 = _to64(state)
        tr.grads(cur.to(DEV), fut.to(DEV), act.to(DEV))
        tracked += 1
        masks = {site: (tr.activation(site, n) > 0).cpu() for site in FO.RELU_SITES}
        want = oracle.step(cur, fut, act, relu_masks=masks)
        with TS.record_mean2_over_var(FO) as seen:
            exact = FO.ForwardModelTrainer(state64, lr=LR).step(cur.double(), fut.double(), act.double(), relu_masks=masks)
        TS.assert_guard(seen, 10)
        # ---- loss and residual
        l64 = exact["loss"].item()
        err, ref = abs(tr.loss.item() - l64), abs(want["loss"].item() - l64)
        print("n=%d it=%d loss: kernels %.3e, fp32 oracle %.3e (loss %.4f)" % (n, it, err, ref, l64))
        assert err <= max(1e-5 * max(1.0, l64), 2.0 * ref), (n, it, err, ref)
        err, ref = _maxabs(tr.resid, exact["resid"]), _maxabs(want["resid"], exact["resid"])
        print("n=%d it=%d resid: kernels %.3e, fp32 oracle %.3e" % (n, it, err, ref))
        assert err <= max(2e-5, 2.0 * ref), (n, it, err, ref)
        # ---- gradients
        grads = tr.named_gradients()
        checked = 0
        for name, ref32 in want["grads"].items():
            if ref32 is None:                                  # conv4_bn / conv5_bn: constructed, never applied
                assert name not in grads and name.startswith(UNUSED_BN)
                continue
            mine = grads[name].cpu()
            if name in NOISE_BIASES:
                wscale = float(want["grads"][name[:-4] + "weight"].abs().max())
                assert float(mine.abs().max()) <= 1e-4 * wscale, (name, n, it)
                continue
            err, ref = _rel(mine, exact["grads"][name]), _rel(ref32, exact["grads"][name])
            worst["grad"] = max(worst["grad"], (err / max(2e-5, 2.0 * ref), err, ref, "%s it=%d" % (name, it)))
            assert err <= max(2e-5, 2.0 * ref), (name, n, it, err, ref)
            checked += 1
        assert checked == 14 + 4 + 2 * 10                      # 14 weights, 4 live biases, 10 BatchNorms' weight and bias
        tr.apply()
        # ---- running statistics and counters
        sd = {k: v.detach().cpu() for k, v in tr.sync_to_module().state_dict().items()}
        stats = [k for k in sd if "running_" in k and not k.startswith(UNUSED_BN)]
        assert len(stats) == 20
        for k in stats:
            err, ref = _maxabs(sd[k], state64[k]), _maxabs(state[k], state64[k])
            floor = 1e-6 * float(state64[k].abs().max())
            worst["running"] = max(worst["running"], (err / max(floor, 2.0 * ref), err, ref, "%s it=%d" % (k, it)))
            assert err <= max(floor, 2.0 * ref), (k, n, it, err, ref, floor)
            assert _maxabs(sd[k], loaded[k]) > 1e-4, k         # (it moved)
        for k in sd:
            if k.endswith("num_batches_tracked") and not k.startswith(UNUSED_BN):
                assert int(sd[k]) == tracked == int(state64[k]), (k, int(sd[k]), tracked)
        for bn in UNUSED_BN:                                   # bit-identical to what was loaded, the 7 included
            for leaf in BN_LEAVES:
                assert torch.equal(sd[bn + "." + leaf], loaded[bn + "." + leaf]), (bn, leaf)
            assert int(sd[bn + ".num_batches_tracked"]) == TS.BATCHES_TRACKED
    for what in ("grad", "running"):
        print("n=%d worst %s: %.2f of its bound, kernels %.3e, fp32 oracle %.3e (%s)" % ((n, what) + worst[what]))
    # a grads() without apply() is a training-mode forward as well: torch's BatchNorm counts it
    steps = tr.steps
    tr.grads(cur.to(DEV), fut.to(DEV), act.to(DEV))
    sd = tr.sync_to_module().state_dict()
    assert tr.steps == steps == (2 if n == 3 else 1)
    assert int(sd["decoder.deconv3_bn.num_batches_tracked"]) == tracked + 1
    assert int(sd["encoder.conv4_bn.num_batches_tracked"]) == TS.BATCHES_TRACKED


# ------------------------------------------------------------------------------------------ (e) Adam from resumed moments
def _adam_inputs(count, seed, live=None):
    """(grad, exp_avg, exp_avg_sq) as fp32: per element s = 10^U[-10,-1]; g = +-s 10^U[-1,1]; m = +-s 10^U[-1,1];
    v = (s 10^U[-0.5,0.5])^2; every 97th g zero, every 291st m and v zero.  Elements with sqrt(v) comparable to eps,
    elements where nothing moves (291 = 3 x 97), every step <~ 30 lr.  `live`: the positions that are no layout padding --
    padded entries are zero in every vector (include/ndp.h)."""
    gen = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(count, generator=gen, dtype=torch.float64)        # noqa: E731
    sign = lambda: (torch.randint(0, 2, (count,), generator=gen) * 2 - 1).double()                   # noqa: E731
    s = 10.0 ** u(-10.0, -1.0)
    g = sign() * s * 10.0 ** u(-1.0, 1.0)
    m = sign() * s * 10.0 ** u(-1.0, 1.0)
    v = (s * 10.0 ** u(-0.5, 0.5)) ** 2
    idx = torch.arange(count)
    g[idx % 97 == 0] = 0.0
    m[idx % 291 == 0] = 0.0
    v[idx % 291 == 0] = 0.0
    out = [t.float() for t in (g, m, v)]
    if live is not None:
        for t in out:
            t[~live] = 0.0
    return out


def _torch_adam(p, g, m, v, t0, dtype):
    """torch.optim.Adam on the CPU with that state loaded: (param, exp_avg, exp_avg_sq) after one step, as numpy fp64."""
    p = p.to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=LR, betas=BETAS, eps=EPS)
    opt.state[p] = {"step": torch.tensor(float(t0)), "exp_avg": m.to(dtype).clone(), "exp_avg_sq": v.to(dtype).clone()}
    p.grad = g.to(dtype).clone()
    opt.step()
    st = opt.state[p]
    assert int(st["step"]) == t0 + 1
    return [t.detach().double().numpy() for t in (p, st["exp_avg"], st["exp_avg_sq"])]


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _check_adam(what, t0, p_old, g, got, live_count):
    """got: (params, exp_avg, exp_avg_sq) of the kernel, CPU fp32; elementwise against torch's Adam in fp32 and fp64.
    The 2e-5 terms: adam_update forms 1.f - b2 in fp32 from 0.999f where torch rounds the double 1 - 0.999 -- the
    (1 - b2) g^2 increment of v differs by at most 1.31e-5 of itself, a step by at most 0.7e-5 of itself."""
    g_, m_, v_ = g
    r32, r64 = _torch_adam(p_old, g_, m_, v_, t0, torch.float32), _torch_adam(p_old, g_, m_, v_, t0, torch.float64)
    g64, old64 = g_.double().numpy(), p_old.double().numpy()
    extra = (lambda: 2e-5 * np.abs(r64[0] - old64) + _ulp32(r64[0]),                      # one bound at a time: 33 M doubles each
             lambda: 4.0 * _ulp32(r64[1]),
             lambda: 2e-5 * (1.0 - BETAS[1]) * g64 * g64 + 4.0 * _ulp32(r64[2]))
    moved = int((r64[0] != old64).sum())
    assert 0.95 * live_count <= moved < live_count, (moved, live_count)   # (every 291st element has nothing to move)
    assert float(np.abs(r64[0] - old64).max()) <= 50 * LR                 # (10 s / (0.316 s) and the bias corrections)
    for name, mine, e32, e64, more in zip(("params", "exp_avg", "exp_avg_sq"), got, r32, r64, extra):
        a = mine.double().numpy()
        bound = 2.0 * np.abs(e32 - e64) + more()
        err = np.abs(a - e64)
        i = int(np.argmax(err / bound))
        print("%s t0=%d %s: worst element %.2f of its bound (kernel error %.3e, fp32 torch error %.3e, value %.3e)"
              % (what, t0, name, err[i] / bound[i], err[i], abs(e32[i] - e64[i]), e64[i]))
        assert np.isfinite(a).all() and bool((err <= bound).all()), (what, t0, name, i, err[i], bound[i])


def _live_mask(pack, modules):
    """Which positions of the flat vector hold a parameter (the rest is layout padding): pack modules of all ones."""
    with torch.no_grad():
        for mod in modules:
            for p in mod.parameters():
                p.fill_(1.0)
    return (pack(*[mod.to(DEV) for mod in modules], DEV)[0] != 0).cpu()


@functools.lru_cache(maxsize=None)
def _fm_adam_case():
    from ndivplanning_amd.models import forward_encoder as FE
    live = _live_mask(FE.pack_module, [FE.ForwardAutoencoder()])
    return live, _adam_inputs(live.numel(), 71, live)


@functools.lru_cache(maxsize=None)
def _ae_adam_case():
    from ndivplanning_amd.models import image_autoencoder as IA
    live = _live_mask(IA.pack_autoencoder, [IA.Encoder(), IA.Decoder()])
    return live, _adam_inputs(live.numel(), 72, live)


def _resume_and_apply(tr, t0, inputs):
    g, m, v = inputs
    assert tr.params.numel() == g.numel()
    tr.step_word.zero_()
    tr.step_word[0] = t0
    tr.grad.copy_(g)
    tr.exp_avg.copy_(m)
    tr.exp_avg_sq.copy_(v)
    p_old = tr.params.cpu()
    tr.apply()
    torch.cuda.synchronize()
    assert int(tr.step_word[0]) == t0 + 1
    return p_old, (tr.params.cpu(), tr.exp_avg.cpu(), tr.exp_avg_sq.cpu())


def _assert_head_is_a_full_repack(tr, pack_fn, head):
    """After the optimizer launch the second weight order in the workspace head is bit for bit what a repack from the new
    parameters gives (the check of test_the_optimizer_launch_leaves_the_second_weight_order_a_full_repack_would, on
    updates that are not +-lr)."""
    from ndivplanning_amd import _capi
    before = tr.workspace[:head].view(torch.int32).clone()
    assert int((before != 0).sum()) > head // 2
    _capi.check(getattr(tr.lib, pack_fn)(_capi.ptr(tr.params), _capi.ptr(tr.workspace), _capi.stream_ptr(DEV)), pack_fn)
    torch.cuda.synchronize()
    assert torch.equal(before, tr.workspace[:head].view(torch.int32))


@pytest.mark.parametrize("t0", [2, 1000])        # (an exponent t + 1 in the first bias correction is inside the bounds at 1000)
def test_fm_apply_adam_from_resumed_moments(t0):
    """ndp_fm_apply_adam (k_fm_adam_pack: 33 M elements, the tiled and the plain segments) against torch.optim.Adam."""
    torch.set_num_threads(16)
    live, inputs = _fm_adam_case()
    tr, _ = _trained_fm_trainer(61, 1)
    assert tr.params.numel() > 33_000_000
    p_old, got = _resume_and_apply(tr, t0, inputs)
    assert tr.steps == 1
    _check_adam("ndp_fm_apply_adam", t0, p_old, inputs, got, int(live.sum()))
    head = tr.lib.ndp_fm_workspace_offset(1, 0)
    assert head > 30_000_000
    _assert_head_is_a_full_repack(tr, "ndp_fm_pack_params", head)


@pytest.mark.parametrize("t0", [2, 1000])
def test_ae_apply_adam_from_resumed_moments(t0):
    """ndp_ae_apply_adam (k_fm_adam_pack with the autoencoder's segments) against torch.optim.Adam."""
    from ndivplanning_amd.autoencoder_trainer import AutoencoderTrainer
    from ndivplanning_amd.models import image_autoencoder as IA
    torch.set_num_threads(16)
    live, inputs = _ae_adam_case()
    torch.manual_seed(3)
    enc, dec = IA.Encoder(), IA.Decoder()
    dec.weight_init(0.0, 0.02)
    enc.weight_init(0.0, 0.02)
    enc.load_state_dict(TS.trained_like(enc.state_dict(), 62))
    dec.load_state_dict(TS.trained_like(dec.state_dict(), 63))
    tr = AutoencoderTrainer(enc.to(DEV).train(), dec.to(DEV).train(), batch=1)
    p_old, got = _resume_and_apply(tr, t0, inputs)
    _check_adam("ndp_ae_apply_adam", t0, p_old, inputs, got, int(live.sum()))
    # the second-order region, from the layout: conv1 as [rows][27 -> 32 columns], conv2 .. deconv5 at their full size
    sizes = [IA.ae_layout(tr.lib, 0, l)[1][:3] for l in range(len(IA.AE_LAYERS) - 1)]
    p2 = sizes[0][0] * 32 + sum(r * t * c for r, t, c in sizes[1:])
    assert 18_000_000 < p2 < tr.lib.ndp_ae_workspace_offset(1, 0)
    _assert_head_is_a_full_repack(tr, "ndp_ae_pack_params", p2)


@pytest.mark.parametrize("t0", [2, 1000])
def test_adam_step_from_resumed_moments(t0):
    """ndp_adam_step (k_adam, the GAN path's stand-alone update) at n = 58,305 against torch.optim.Adam."""
    from ndivplanning_amd import _capi
    lib, p = _capi.load(), _capi.ptr
    n = 58305
    inputs = _adam_inputs(n, 73)
    p_old = torch.randn(n, generator=torch.Generator().manual_seed(74))
    dev = [t.to(DEV) for t in (p_old, *inputs)]
    word = torch.zeros(4, dtype=torch.int32, device=DEV)            # the Adam state word: int32[4] (include/ndp.h)
    word[0] = t0
    _capi.check(lib.ndp_adam_step(p(dev[0]), p(dev[1]), p(dev[2]), p(dev[3]), n, p(word), LR, BETAS[0], BETAS[1], EPS,
                                  _capi.stream_ptr()), "ndp_adam_step")
    torch.cuda.synchronize()
    assert int(word[0]) == t0 + 1
    assert torch.equal(dev[1].cpu(), inputs[0])                      # the gradient is read only
    _check_adam("ndp_adam_step", t0, p_old, inputs, (dev[0].cpu(), dev[2].cpu(), dev[3].cpu()), n)
