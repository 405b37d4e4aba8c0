"""Input gradients of Decoder, Discriminator and the eval-mode ForwardAutoencoder (ndivplanning_amd.input_grad):
ndp_g_input_grad, ndp_d_input_grad, ndp_fm_input_grads against the oracles' autograd.

Comparison rule (tests/test_gpu_forward_model.py): with _rel(a, b) = |a - b| / |b| in fp64, the kernels' error against
the fp64 oracle may be at most max(2e-5, 2 x the fp32 CPU oracle's error against the same fp64 result)."""
import pytest
import torch

from conftest import load_golden
from oracle import forward_model_oracle as FO
from oracle import gan_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 2), (17, 2), (33, 5), (100, 1), (64, 16), (300, 2)]       # one partial tile, tile boundaries, nz 1..16


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _check(mine, ref32, ref64, what):
    mine = mine.detach().cpu()
    assert torch.isfinite(mine).all(), what
    err_mine, err_ref = _rel(mine, ref64), _rel(ref32.detach(), ref64)
    print("%s: kernels %.3e, fp32 oracle %.3e" % (what, err_mine, err_ref))
    assert err_mine <= max(2e-5, 2.0 * err_ref), (what, err_mine, err_ref)


def _switch():
    from ndivplanning_amd.input_grad import input_gradients
    return input_gradients()


def _modules(nz):
    from ndivplanning_amd.models.gan import Decoder, Discriminator
    g, _ = O.init_params(1, nz)
    _, d = O.init_params(2, 2)
    dec, dis = Decoder(nz), Discriminator()
    dec.load_state_dict(g)
    dis.load_state_dict(d)
    return g, d, dec.to(DEV), dis.to(DEV)


def _ambiguous_rows(params, acts):
    """Rows in which some hidden pre-activation of the fp64 oracle is within 1e-6 of zero: two correct fp32
    implementations may decide that (Leaky)ReLU differently, which moves the row's input gradient by per cent."""
    bad = torch.zeros(acts[0].shape[0], dtype=torch.bool)
    for i in range(1, len(acts)):
        pre = acts[i - 1] @ params["fc%d.weight" % i].t() + params["fc%d.bias" % i]
        bad |= (pre.abs() < 1e-6).any(dim=1)
    return bad


def _g_oracle(g, z, up, dtype):
    p = {k: v.to(dtype) for k, v in g.items()}
    zz = z.to(dtype).clone().requires_grad_(True)
    out, acts = O.g_forward(p, zz, keep=True)
    (out * up.to(dtype)).sum().backward()
    return zz.grad, p, [a.detach() for a in acts]


def _d_oracle(d, action, code, up, dtype):
    p = {k: v.to(dtype) for k, v in d.items()}
    a, c = action.to(dtype).clone().requires_grad_(True), code.to(dtype).clone().requires_grad_(True)
    out, acts = O.d_forward(p, a, c, keep=True)
    (out * up.to(dtype)).sum().backward()
    return torch.cat([a.grad, c.grad], dim=1), p, [x.detach() for x in acts]


def _keep_rows(bad, m):
    assert int(bad.sum()) <= 0.02 * m, "%d of %d rows have a rounding-level pre-activation" % (int(bad.sum()), m)
    return ~bad


@pytest.mark.parametrize("m,nz", SHAPES)
def test_decoder_input_gradient(m, nz):
    g, _, dec, _ = _modules(nz)
    gen = torch.Generator().manual_seed(m)
    z = torch.cat([torch.randn(m, 256, generator=gen), torch.rand(m, nz, generator=gen)], dim=1)
    up = torch.randn(m, 4, generator=gen)
    exact, p64, acts64 = _g_oracle(g, z, up, torch.float64)
    ref32, _, _ = _g_oracle(g, z, up, torch.float32)
    keep = _keep_rows(_ambiguous_rows(p64, acts64), m)
    zd = z.to(DEV).requires_grad_(True)
    with _switch():
        out = dec(zd)
    (out * up.to(DEV)).sum().backward()
    assert zd.grad.shape == (m, 256 + nz)
    _check(zd.grad.cpu()[keep], ref32[keep], exact[keep], "d z (%d, %d)" % (m, nz))
    _check(zd.grad.cpu()[keep][:, 256:], ref32[keep][:, 256:], exact[keep][:, 256:], "d noise (%d, %d)" % (m, nz))
    # the parameter gradients under the switch are those of the same call outside it, bit for bit
    inside = [p.grad.clone() for p in dec.parameters()]
    dec.zero_grad(set_to_none=True)
    (dec(z.to(DEV)) * up.to(DEV)).sum().backward()
    for a, p in zip(inside, dec.parameters()):
        assert torch.equal(a, p.grad)
    # all parameters frozen: the input gradient alone (the same kernels on the same data)
    dec.zero_grad(set_to_none=True)
    for p in dec.parameters():
        p.requires_grad_(False)
    zf = z.to(DEV).requires_grad_(True)
    with _switch():
        out = dec(zf)
    (out * up.to(DEV)).sum().backward()
    assert torch.equal(zf.grad, zd.grad) and all(p.grad is None for p in dec.parameters())


@pytest.mark.parametrize("m", sorted({m for m, _ in SHAPES}))
def test_discriminator_input_gradients(m):
    _, d, _, dis = _modules(2)
    gen = torch.Generator().manual_seed(m)
    action = torch.rand(m, 4, generator=gen) * 2 - 1
    code = torch.randn(m, 256, generator=gen)
    up = torch.randn(m, 1, generator=gen) / m
    exact, p64, acts64 = _d_oracle(d, action, code, up, torch.float64)
    ref32, _, _ = _d_oracle(d, action, code, up, torch.float32)
    keep = _keep_rows(_ambiguous_rows(p64, acts64), m)
    ad, cd = action.to(DEV).requires_grad_(True), code.to(DEV).requires_grad_(True)
    with _switch():
        out = dis(ad, cd)
    (out * up.to(DEV)).sum().backward()
    mine = torch.cat([ad.grad, cd.grad], dim=1).cpu()
    _check(mine[keep], ref32[keep], exact[keep], "d (action, code) m = %d" % m)
    _check(cd.grad.cpu()[keep], ref32[keep][:, 4:], exact[keep][:, 4:], "d code m = %d" % m)
    inside = [p.grad.clone() for p in dis.parameters()]
    dis.zero_grad(set_to_none=True)
    a2 = action.to(DEV).requires_grad_(True)
    (dis(a2, code.to(DEV)) * up.to(DEV)).sum().backward()
    for a, p in zip(inside, dis.parameters()):
        assert torch.equal(a, p.grad)
    assert torch.equal(a2.grad, ad.grad)
    dis.zero_grad(set_to_none=True)
    for p in dis.parameters():
        p.requires_grad_(False)
    cf = code.to(DEV).requires_grad_(True)
    with _switch():
        out = dis(action.to(DEV), cf)
    (out * up.to(DEV)).sum().backward()
    assert torch.equal(cf.grad, cd.grad) and all(p.grad is None for p in dis.parameters())


def test_code_gradient_flows_through_generator_and_discriminator():
    m, nz = 33, 2
    g, d, dec, dis = _modules(nz)
    # 2 % of 33 rows is no row at all, so this draw is one in which the fp64 oracle has no pre-activation near zero: the
    # smallest |h| is 1.2e-5 (the draw seeded with m itself has 7.9e-7 in row 13 of G's fc4), and all 33 rows are compared
    gen = torch.Generator().manual_seed(1000 + m)
    code = torch.randn(m, 256, generator=gen)
    noise = torch.rand(m, nz, generator=gen)
    up = torch.randn(m, 1, generator=gen) / m

    def oracle(dtype):
        pg, pd = ({k: v.to(dtype) for k, v in q.items()} for q in (g, d))
        c = code.to(dtype).clone().requires_grad_(True)
        a, acts_g = O.g_forward(pg, torch.cat([c, noise.to(dtype)], dim=1), keep=True)
        out, acts_d = O.d_forward(pd, a, c, keep=True)
        (out * up.to(dtype)).sum().backward()
        bad = _ambiguous_rows(pg, [x.detach() for x in acts_g]) | _ambiguous_rows(pd, [x.detach() for x in acts_d])
        return c.grad, bad
    exact, bad = oracle(torch.float64)
    ref32, _ = oracle(torch.float32)
    keep = _keep_rows(bad, m)
    cd = code.to(DEV).requires_grad_(True)
    with _switch():
        out = dis(dec(torch.cat([cd, noise.to(DEV)], dim=1)), cd)
    (out * up.to(DEV)).sum().backward()
    _check(cd.grad.cpu()[keep], ref32[keep], exact[keep], "d code through D(G(.), .)")
    # through D alone the gradient is a different one -- by 1.8e-3 of its norm in the fp64 oracle, a hundred times what
    # the comparison above allows: both paths contribute
    c2 = code.to(DEV).requires_grad_(True)
    with _switch():
        out = dis(dec(torch.cat([code.to(DEV), noise.to(DEV)], dim=1)).detach(), c2)
    (out * up.to(DEV)).sum().backward()
    assert _rel(c2.grad.cpu(), exact) > 5e-4


# ------------------------------------------------------------------------------------------ forward model
def _fm_state(seed):
    """init_forward_model_state with every BatchNorm overwritten: a gradient that ignored the running statistics or the
    weights would be wrong by tens of per cent."""
    state = FO.init_forward_model_state(seed)
    gen = torch.Generator().manual_seed(1000 + seed)
    for k in list(state):
        if k.endswith(".running_mean"):
            c = state[k].numel()
            base = k[:-len(".running_mean")]
            state[k] = torch.randn(c, generator=gen) * 0.05
            state[base + ".running_var"] = torch.rand(c, generator=gen) * 1.5 + 0.5
            state[base + ".weight"] = torch.rand(c, generator=gen) + 0.5
            state[base + ".bias"] = torch.randn(c, generator=gen) * 0.1
    return state


def _fm_model(state):
    from ndivplanning_amd.models import forward_encoder as FE
    model = FE.ForwardAutoencoder()
    model.load_state_dict(state)
    return model.to(DEV).eval()


def _fm_inputs(seed, n):
    gen = torch.Generator().manual_seed(seed)
    cur = torch.rand(n, 3, 128, 128, generator=gen) * 2.0 - 1.0
    act = torch.rand(n, 4, generator=gen) * 2.0 - 1.0
    up = torch.randn(n, 3, 128, 128, generator=gen)
    return cur, act, up


def _fm_oracle(state, cur, act, up, masks, dtype):
    s = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in state.items()}
    c, a = cur.to(dtype).clone().requires_grad_(True), act.to(dtype).clone().requires_grad_(True)
    out = FO.forward(s, c, a, training=False, relu_masks=masks)
    out.backward(up.to(dtype))
    return out.detach(), c.grad, a.grad


@pytest.mark.parametrize("n", [1, 3, 16, 32, 65])   # where the data-gradient launches change variant (65: deconv1's through the 128-row tiles)
def test_forward_model_input_gradients(n):
    from ndivplanning_amd.models import forward_encoder as FE
    torch.set_num_threads(8)
    state = _fm_state(11 + n)
    model = _fm_model(state)
    cur, act, up = _fm_inputs(20 + n, n)
    cd, ad = cur.to(DEV).requires_grad_(True), act.to(DEV).requires_grad_(True)
    with _switch():
        out = model(cd, ad)
    assert out.requires_grad
    masks = {k: v.cpu() for k, v in FE.saved_relu_masks(out).items()}
    assert sorted(masks) == sorted(FO.RELU_SITES)
    out.backward(up.to(DEV))
    out64, dc64, da64 = _fm_oracle(state, cur, act, up, masks, torch.float64)
    _, dc32, da32 = _fm_oracle(state, cur, act, up, masks, torch.float32)
    assert float((out.detach().cpu().double() - out64).abs().max()) <= 2e-5
    _check(ad.grad, da32, da64, "d actions n = %d" % n)
    _check(cd.grad, dc32, dc64, "d state_cur n = %d" % n)
    # the identity (out = state_cur + residual) dominates d state_cur by ~10^3: the part that went through the network
    up64 = up.double()
    _check(cd.grad.cpu().double() - up64, dc32.double() - up64, dc64 - up64, "d state_cur - upstream n = %d" % n)
    assert 0.0 < float((dc64 - up64).norm()) < 0.1 * float(dc64.norm())


def test_forward_model_input_gradient_variants():
    """Actions only, byte frames, run-to-run bits, one backward per forward."""
    from ndivplanning_amd import _capi
    n = 3
    model = _fm_model(_fm_state(5))
    cur, act, up = _fm_inputs(6, n)
    upd = up.to(DEV)

    def run(frames, state_grad):
        c = frames.to(DEV)
        if state_grad:
            c.requires_grad_(True)
        a = act.to(DEV).requires_grad_(True)
        with _switch():
            out = model(c, a)
        out.backward(upd, retain_graph=True)
        return out, c, a
    out1, c1, a1 = run(cur, True)
    _, c2, a2 = run(cur, True)
    assert torch.equal(a1.grad, a2.grad) and torch.equal(c1.grad, c2.grad)             # bit-reproducible
    _, c3, a3 = run(cur, False)
    assert torch.equal(a3.grad, a1.grad) and c3.grad is None                           # the chain stops at the decoder
    with pytest.raises(_capi.NdpError):
        out1.backward(upd)                                                             # its activations are consumed
    lut = torch.from_numpy(load_golden("frames_case")["lut"])
    gen = torch.Generator().manual_seed(7)
    frames8 = torch.randint(0, 256, (n, 128, 128, 3), generator=gen, dtype=torch.uint8)
    floats = lut[frames8.long()].permute(0, 3, 1, 2).contiguous()
    out8, _, a8 = run(frames8, False)
    outf, _, af = run(floats, False)
    assert torch.equal(out8, outf) and torch.equal(a8.grad, af.grad) and float(a8.grad.abs().max()) > 0


def test_goal_loss_and_grad_and_refine_actions():
    from ndivplanning_amd import evaluation
    from ndivplanning_amd.models import forward_encoder as FE
    torch.set_num_threads(8)
    b, th = 3, 2
    state = _fm_state(8)
    model = _fm_model(state)
    gen = torch.Generator().manual_seed(9)
    cur = torch.rand(b, 3, 128, 128, generator=gen) * 2.0 - 1.0
    goal = torch.rand(b, 3, 128, 128, generator=gen) * 2.0 - 1.0
    actions = torch.rand(b, th, 4, generator=gen) * 2.0 - 1.0
    # each call's own ReLU decisions, for the oracles: the same rollout, step by step, inside the switch
    masks = []
    x = cur.to(DEV)
    with _switch():
        for t in range(th):
            x = model(x, actions[:, t].to(DEV).requires_grad_(True))
            masks.append({k: v.cpu() for k, v in FE.saved_relu_masks(x).items()})
    del x
    loss, grad = evaluation.goal_loss_and_grad(model, cur.to(DEV), goal.to(DEV), actions.to(DEV))
    assert loss.shape == (b,) and grad.shape == (b, th, 4)

    def oracle(dtype):
        s = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in state.items()}
        a = actions.to(dtype).clone().requires_grad_(True)
        y = cur.to(dtype)
        for t in range(th):
            y = FO.forward(s, y, a[:, t], training=False, relu_masks=masks[t])
        ls = ((y - goal.to(dtype)) ** 2).flatten(1).mean(dim=1)
        ls.sum().backward()
        return ls.detach(), a.grad
    loss64, grad64 = oracle(torch.float64)
    loss32, grad32 = oracle(torch.float32)
    _check(loss, loss32, loss64, "rollout loss")
    _check(grad, grad32, grad64, "d loss / d actions of the rollout")
    lr = 0.5
    refined, losses = evaluation.refine_actions(model, cur.to(DEV), goal.to(DEV), actions.to(DEV), 1,
                                                lambda p: torch.optim.SGD(p, lr=lr, foreach=False))
    assert torch.equal(losses[0], loss)
    assert torch.equal(refined, torch.add(actions.to(DEV), grad, alpha=-lr))


def test_nothing_changes_outside_the_switch():
    from ndivplanning_amd.input_grad import input_gradients
    _, _, dec, dis = _modules(2)
    with pytest.raises(NotImplementedError):
        dec(torch.zeros(4, 258, device=DEV).requires_grad_(True))
    code = torch.zeros(4, 256, device=DEV).requires_grad_(True)
    out = dis(torch.zeros(4, 4, device=DEV), code)
    with pytest.raises(NotImplementedError):
        out.sum().backward()
    model = _fm_model(FO.init_forward_model_state(2))
    cur, act, _ = _fm_inputs(3, 2)
    with pytest.raises(NotImplementedError):
        model(cur.to(DEV), act.to(DEV).requires_grad_(True))
    with pytest.raises(NotImplementedError):
        model(cur.to(DEV).requires_grad_(True), act.to(DEV))
    pred = model(cur.to(DEV), act.to(DEV))
    assert not pred.requires_grad
    with input_gradients():
        assert not model(cur.to(DEV), act.to(DEV)).requires_grad            # nothing asks for a gradient: the plain path
        model.train()
        with pytest.raises(NotImplementedError):                            # training mode: batch statistics depend on the input
            model(cur.to(DEV), act.to(DEV).requires_grad_(True))
        with input_gradients(False):
            model.eval()
            with pytest.raises(NotImplementedError):
                model(cur.to(DEV), act.to(DEV).requires_grad_(True))
