"""GPU parity of the forward (next-frame) model kernels (csrc/ndp_forward_model.inc) with
the oracle's restatement of models/forward_encoder.py + train_forward_model.py:98-112 and with the golden vector the
REFERENCE's own ForwardAutoencoder / MSELoss / Adam produced (tests/golden/forward_model_case.npz)."""
import io
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import forward_model_oracle as FO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR = 2e-4

# Biases of the layers a BatchNorm follows: the batch mean is subtracted right after them, so their gradient is zero
# but for rounding (1e-9 of the weight gradient's scale here, 1e-17 in an fp64 reference) and Adam turns that noise
# into steps of up to lr whose sign no two implementations share.  They have no effect on the function.
NOISE_BIASES = tuple("%s.bias" % n for n in ("encoder.conv1", "encoder.conv2", "encoder.conv3", "decoder.deconv1",
                                             "decoder.deconv2", "decoder.deconv3", "decoder.deconv4", "decoder.deconv5",
                                             "decoder.deconv6", "decoder.conv_refine_1"))


def _inputs(data_seed, n):
    gen = torch.Generator().manual_seed(data_seed)
    frames = torch.rand(n, 3, 3, 128, 128, generator=gen) * 2.0 - 1.0
    actions = torch.rand(n, 3, 4, generator=gen) * 2.0 - 1.0
    return frames, actions


def _sums(t):
    t = t.detach().double().cpu()
    return np.array([t.sum().item(), t.abs().sum().item(), (t * t).sum().item()])


def _hip_trainer(seed, n, **kw):
    from ndivplanning_amd.forward_trainer import ForwardModelTrainer
    from ndivplanning_amd.models import forward_encoder as FE
    state = FO.init_forward_model_state(seed)
    model = FE.ForwardAutoencoder()
    model.load_state_dict(state)
    model = model.to(DEV).train()
    return ForwardModelTrainer(model, batch=n, lr=LR, **kw), state


def test_two_training_iterations_match_the_reference_golden():
    """Against what the REFERENCE's own module, loss and optimizer produced (checksums: the fixture holds no 33 M weights).
    The bounds on gradients and parameters are those of a run whose ReLU decisions may differ from the reference's in a
    few elements: this case has a conv3_bn output 5.8e-8 from zero (scale 4) in fp64, a coin toss for any fp32 summation
    order, and deciding it the other way moves conv1_bn's bias gradient by 1e-3 of its scale.  A wrong formula would be off
    by O(1); the tight elementwise comparison is test_training_iterations_against_the_oracle_elementwise."""
    g = load_golden("forward_model_case")
    seed, data_seed, n = (int(v) for v in g["meta"])
    tr, _ = _hip_trainer(seed, n, keep_residual=True)
    frames, actions = _inputs(data_seed, n)
    names = [str(s) for s in g["names"]]
    for it in range(2):
        cur, fut, act = (t.contiguous().to(DEV) for t in (frames[:, it], frames[:, it + 1], actions[:, it]))
        tr.grads(cur, fut, act)
        # iteration 2 starts from parameters that Adam moved by +-lr with the sign of gradients that may have differed
        first = it == 0
        assert abs(tr.loss.item() - float(g["s%d.loss" % it])) <= (2e-6 if first else 2e-4)
        resid = tr.resid.cpu()
        np.testing.assert_allclose(resid[:, :, ::16, ::16].numpy(), g["s%d.resid_sample" % it], atol=2e-5 if first else 3e-3)
        np.testing.assert_allclose(_sums(resid)[1:], g["s%d.resid_sums" % it][1:], rtol=1e-4 if first else 1e-2)
        grads = tr.named_gradients()
        tr.apply()
        params = tr.named_parameters()
        for i, name in enumerate(names):
            want = g["s%d.grad_sums" % it][i]
            if name not in grads:                         # conv4_bn / conv5_bn: constructed, never applied
                assert not want.any(), name
                continue
            if name in NOISE_BIASES:
                wscale = g["s%d.grad_sums" % it][names.index(name[:-4] + "weight")][1]
                assert _sums(grads[name])[1] <= 1e-5 * wscale, name
                continue
            assert abs(_sums(grads[name])[1] - want[1]) <= (2e-2 if first else 5e-2) * max(want[1], 1e-12), (name, it)
            wantp = g["s%d.param_sums" % it][i]
            # (iteration 2: plus a few elements whose second Adam step went the other way, 2 lr each)
            slack = 1e-7 if first else 2 * LR * (2 + 0.01 * params[name].numel())
            assert abs(_sums(params[name])[1] - wantp[1]) <= (2e-3 if first else 1e-2) * max(wantp[1], 1e-12) + slack, (name, it)
    model = tr.sync_to_module()
    sd = model.state_dict()
    keys = [k for k in sd if "running_" in k]
    for k, want in zip(keys, g["running_sums"]):
        got = _sums(sd[k])
        if k.endswith("running_var"):
            np.testing.assert_allclose(got, want, rtol=1e-4, err_msg=k)
        else:
            # batch means of zero-mean maps are ~1e-3 of the maps' scale: their rounding error is relative to THAT scale
            # (the signed sum cancels further and is not compared)
            np.testing.assert_allclose(got[1:], want[1:], rtol=5e-3, atol=1e-9, err_msg=k)
    assert int(sd["decoder.deconv3_bn.num_batches_tracked"]) == 2


def test_second_iteration_is_as_tight_as_the_first_where_no_relu_is_a_coin_toss():
    """tests/golden/forward_model_case_sharp.npz: the reference's own module / MSELoss / Adam on a case chosen so that the
    first iteration decides every ReLU unambiguously (tests/golden/search_forward_model_seed.py: at every ReLU site the
    smallest |pre-activation| is >= 15 x the site's rms fp32 rounding error).  Then nothing amplifies rounding: the
    first-iteration gradients agree to rounding, Adam moves every parameter the same way (but the biases in front of a
    BatchNorm, whose gradient IS rounding noise and which have no effect on the function), and the second iteration's
    loss and residual are held to the first iteration's bounds -- unconditionally, against numbers only the reference
    produced.  (Its gradient CHECKSUMS keep a looser bound: the second iteration has its own near-zero pre-activations.)"""
    g = load_golden("forward_model_case_sharp")
    seed, data_seed, n = (int(v) for v in g["meta"])
    tr, _ = _hip_trainer(seed, n, keep_residual=True)
    frames, actions = _inputs(data_seed, n)
    names = [str(s) for s in g["names"]]
    seen = []
    for it in range(2):
        cur, fut, act = (t.contiguous().to(DEV) for t in (frames[:, it], frames[:, it + 1], actions[:, it]))
        tr.grads(cur, fut, act)
        resid = tr.resid.cpu()
        dl = abs(tr.loss.item() - float(g["s%d.loss" % it]))
        dr = float(np.abs(resid[:, :, ::16, ::16].numpy() - g["s%d.resid_sample" % it]).max())
        ds = float(np.abs(_sums(resid)[1:] / g["s%d.resid_sums" % it][1:] - 1).max())
        grads = tr.named_gradients()
        tr.apply()
        params = tr.named_parameters()
        worst_g = worst_p = 0.0
        for i, name in enumerate(names):
            want = g["s%d.grad_sums" % it][i]
            if name not in grads or name in NOISE_BIASES:
                continue
            worst_g = max(worst_g, abs(_sums(grads[name])[1] - want[1]) / max(want[1], 1e-12))
            wantp = g["s%d.param_sums" % it][i]
            worst_p = max(worst_p, abs(_sums(params[name])[1] - wantp[1]) / max(wantp[1], 1e-12))
        seen.append((dl, dr, ds, worst_g, worst_p))
    report = "per iteration (|d loss|, max |d resid sample|, rel resid sums, rel grad abs-sums, rel param abs-sums): %s" % (seen,)
    print(report)
    for it, (dl, dr, ds, wg, wp) in enumerate(seen):
        assert dl <= 2e-6 and dr <= 2e-5 and ds <= 1e-4, (it, report)                  # the SAME bounds for both iterations
        # measured: gradient abs-sums 4e-6 / 8e-4, parameter abs-sums 2e-6 / 6e-4 of their size (iteration 2: its own
        # near-zero pre-activations; BatchNorm biases are still ~lr in size, one element's step weighs per cent there)
        assert wg <= (1e-4 if it == 0 else 5e-3), (it, report)
        assert wp <= (1e-5 if it == 0 else 3e-3), (it, report)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


@pytest.mark.parametrize("n", [1, 3, 8, 16, 32, 65])  # (from 16: deconv5 runs its four parity classes in one workgroup; 32: the bench size, unsplit data gradients; 65: the 4x4 <-> 1x1 layers through the 128-row GEMM tiles)
def test_training_iterations_against_the_oracle_elementwise(n):
    """Every gradient of two iterations against the oracle, adjudicated by the oracle's own arithmetic in fp64: the error of
    the kernels against fp64 may be at most twice the fp32 oracle's (or 2e-5).  Two things keep the comparison tight:
      * the ReLU decisions of the run under test are injected into both oracles (FO.forward, relu_masks): among 10^6
        pre-activations some are within rounding of zero, and ONE element decided the other way moves a small map's
        gradients by 1e-3 -- measured: seed 14, n = 3, an element of up5 -- while the activations themselves agree to 1e-6;
      * iteration 2 starts from the fp32 oracle's parameters (Adam turns rounding-level gradients into steps of lr whose
        sign implementations do not share, so the parameters after a step are compared by their distribution instead)."""
    torch.set_num_threads(8)
    tr, state = _hip_trainer(11 + n, n, keep_residual=True)
    state64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in state.items()}
    oracle = FO.ForwardModelTrainer(state, lr=LR)
    frames, actions = _inputs(20 + n, n)
    for it in range(2):
        cur, fut, act = frames[:, it].contiguous(), frames[:, it + 1].contiguous(), actions[:, it].contiguous()
        if it == 1:                                            # teacher forcing: the oracle's parameters and statistics
            with torch.no_grad():
                tr.model.load_state_dict({k: v.detach() for k, v in state.items()})
            tr.load_from_module()
            state64 = {k: (v.detach().double() if v.is_floating_point() else v.clone()) for k, v in state.items()}
        tr.grads(cur.to(DEV), fut.to(DEV), act.to(DEV))
        masks = {site: (tr.activation(site, n) > 0).cpu() for site in FO.RELU_SITES}
        want = oracle.step(cur, fut, act, relu_masks=masks)
        exact = FO.ForwardModelTrainer(state64, lr=LR).step(cur.double(), fut.double(), act.double(), relu_masks=masks)
        assert abs(tr.loss.item() - exact["loss"].item()) <= 1e-5 * max(1.0, exact["loss"].item())
        assert float((tr.resid.cpu().double() - exact["resid"]).abs().max()) <= 2e-5
        grads = tr.named_gradients()
        for name, ref in want["grads"].items():
            if ref is None:
                assert name not in grads
                continue
            mine = grads[name].cpu()
            if name in NOISE_BIASES:
                wscale = float(want["grads"][name[:-4] + "weight"].abs().max())
                assert float(mine.abs().max()) <= 1e-4 * wscale, name
                continue
            err_mine, err_ref = _rel(mine, exact["grads"][name]), _rel(ref, exact["grads"][name])
            assert err_mine <= max(2e-5, 2.0 * err_ref), (name, n, it, err_mine, err_ref)
        tr.apply()
        params = tr.named_parameters()
        for name in want["grads"]:
            if name in NOISE_BIASES or name not in params:
                continue
            diff = (params[name].cpu() - state[name].detach()).abs()
            assert float(diff.max()) <= 2.2 * LR, name              # one Adam step moves an element by at most ~lr
            assert float(diff.mean()) <= 0.03 * LR, (name, float(diff.mean()))
    assert float(tr.loss_sum.item()) > 0.0


def test_relu_decisions_differ_from_the_oracle_only_at_rounding_level_preactivations():
    """What the mask injection above leaves unchecked: the decisions themselves.  Against the fp64 oracle they may differ only
    where the pre-activation is within rounding of zero, and only in a handful of the ~10^7 elements."""
    n = 2
    tr, state = _hip_trainer(31, n)
    frames, actions = _inputs(32, n)
    cur, fut, act = frames[:, 0].contiguous(), frames[:, 1].contiguous(), actions[:, 0].contiguous()
    tr.grads(cur.to(DEV), fut.to(DEV), act.to(DEV))
    state64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in state.items()}
    recorded = {}                                              # the fp64 oracle's pre-activations, site by site
    import torch.nn.functional as F
    real_relu = F.relu
    sites = iter(FO.RELU_SITES)

    def spy(x, *a, **kw):
        recorded[next(sites)] = x.detach().clone()
        return real_relu(x, *a, **kw)
    FO.F.relu = spy
    try:
        with torch.no_grad():
            FO.forward(state64, cur.double(), act.double(), training=True)
    finally:
        FO.F.relu = real_relu
    assert sorted(recorded) == sorted(FO.RELU_SITES)
    total = flips = 0
    for site, pre in recorded.items():
        mine = tr.activation(site, n).cpu().double()
        differ = (mine > 0) != (pre > 0)
        total += pre.numel()
        flips += int(differ.sum())
        assert float(pre[differ].abs().max() if differ.any() else 0.0) <= 3e-5, site   # only rounding-level pre-activations
        assert float((mine - pre.clamp_min(0)).abs().max()) <= 3e-5, site
    assert flips <= 20 and total > 3_000_000, (flips, total)


def test_eval_and_no_grad_forward_of_the_module_match_the_oracle():
    from ndivplanning_amd.models import forward_encoder as FE
    n = 2
    tr, state = _hip_trainer(3, n)
    oracle = FO.ForwardModelTrainer(state, lr=LR)
    frames, actions = _inputs(4, n)
    cur, fut, act = frames[:, 0].contiguous(), frames[:, 1].contiguous(), actions[:, 0].contiguous()
    oracle.step(cur, fut, act)
    tr.step(cur.to(DEV), fut.to(DEV), act.to(DEV))
    model = tr.sync_to_module()
    # eval mode, grad mode on, parameters requiring grad: how control_evaluation.py / mpc_eval.py call it
    model.eval()
    pred = model(frames[:, 2].to(DEV), actions[:, 2].to(DEV))
    with torch.no_grad():
        want = FO.forward(state, frames[:, 2], actions[:, 2], training=False)
    assert pred.shape == (n, 3, 128, 128) and not pred.requires_grad
    assert float((pred.cpu() - want).abs().max()) <= 2e-4
    # training mode under no_grad: the residual, and the running statistics move
    model.train()
    before = model.decoder.deconv2_bn.running_mean.clone()
    with torch.no_grad():
        resid = model(frames[:, 2].to(DEV), actions[:, 2].to(DEV))
        want = FO.forward(state, frames[:, 2], actions[:, 2], training=True)
    assert float((resid.cpu() - want).abs().max()) <= 2e-4
    assert not torch.equal(before, model.decoder.deconv2_bn.running_mean)
    np.testing.assert_allclose(model.decoder.deconv2_bn.running_mean.cpu().numpy(),
                               state["decoder.deconv2_bn.running_mean"].numpy(), rtol=1e-3, atol=1e-6)
    assert int(model.decoder.deconv2_bn.num_batches_tracked) == int(state["decoder.deconv2_bn.num_batches_tracked"])
    # a CPU tensor has no path
    from ndivplanning_amd import _capi
    with pytest.raises(_capi.NdpError), torch.no_grad():
        model(frames[:, 2], actions[:, 2].to(DEV))
    # the reference saves the whole module (train_forward_model.py:157-163)
    buf = io.BytesIO()
    torch.save(model, buf)
    buf.seek(0)
    again = torch.load(buf, weights_only=False)                  # our own file
    assert isinstance(again, FE.ForwardAutoencoder)
    assert torch.equal(again.encoder.conv3.weight.cpu(), model.encoder.conv3.weight.cpu())


def test_a_step_is_bit_reproducible_and_smaller_batches_reuse_the_trainer():
    tr1, _ = _hip_trainer(9, 4)
    tr2, _ = _hip_trainer(9, 4)
    frames, actions = _inputs(10, 4)
    for tr in (tr1, tr2):
        for it in range(2):
            tr.step(frames[:, it].contiguous().to(DEV), frames[:, it + 1].contiguous().to(DEV), actions[:, it].contiguous().to(DEV))
    assert torch.equal(tr1.params, tr2.params) and torch.equal(tr1.grad, tr2.grad) and torch.equal(tr1.stats, tr2.stats)
    # a ragged final batch (the reference's loader has no drop_last): 3 images through the 4-image trainer
    loss = tr1.step(frames[:3, 0].contiguous().to(DEV), frames[:3, 1].contiguous().to(DEV), actions[:3, 0].contiguous().to(DEV))
    assert torch.isfinite(loss).all() and torch.isfinite(tr1.params).all()
    from ndivplanning_amd import _capi
    with pytest.raises(_capi.NdpError):
        tr1.grads(torch.zeros(5, 3, 128, 128, device=DEV), torch.zeros(5, 3, 128, 128, device=DEV), torch.zeros(5, 4, device=DEV))


def test_train_script_epoch_matches_an_oracle_replay(tmp_path):
    """ndivplanning_amd/train_forward_model.py::train (mirror of the reference's script) on synthetic trajectories against
    a CPU replay with the oracle: same seeding order (seed -> model construction -> weight_init -> loader shuffle)."""
    import models.forward_encoder as shim
    from ndivplanning_amd.train_forward_model import train
    from ndivplanning_amd.train_gan import make_dataset
    from ndivplanning_amd.utils.file import AttrDict
    torch.set_num_threads(8)

    def config():
        return AttrDict({"random_seed": 0, "train_data_path": "synthetic:3:images", "gpu_id": 0, "trajectory_length": 3,
                         "forward_save_path": str(tmp_path / "fm"),
                         "training": {"forward": {"num_epochs": 1, "learning_rate": LR, "report_feq": 10, "batch_size": 2,
                                                  "epochs_per_stage": 1, "step_lr_gamma": 0.1}}})
    # the reference initialises the weights ON the device (train_forward_model.py:67-70: .to(gpu_id), then weight_init):
    # they come from the device's generator, so the replay takes the initial state from the run itself
    from ndivplanning_amd import train_forward_model as script
    initial = {}
    real_trainer = script.ForwardModelTrainer

    def spy(model, **kw):
        initial.update({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
        return real_trainer(model, **kw)
    script.ForwardModelTrainer = spy
    try:
        hist = train(config())
    finally:
        script.ForwardModelTrainer = real_trainer
    cfg = config()
    torch.manual_seed(cfg.random_seed)
    np.random.seed(cfg.random_seed)
    from ndivplanning_amd.models import forward_encoder as FE
    FE.ForwardAutoencoder()                                     # consumes the CPU stream as the run's construction did
    state = initial
    ds = make_dataset(cfg)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=True)
    oracle = FO.ForwardModelTrainer(state, lr=LR)
    total, count = 0.0, 0
    for images, _, actions, _ in loader:
        for i in range(ds.seq_length - 1):
            total += oracle.step(images[:, i].contiguous(), images[:, i + 1].contiguous(), actions[:, i].contiguous())["loss"].item()
            count += 1
    assert count == 4 and len(hist) == 1                      # batches of 2 and 1 trajectories x 2 frame pairs
    assert abs(hist[0] - total / count) <= 2e-5
    saved = torch.load(str(tmp_path / "fm" / "forward_autoencoder_0.pt"), weights_only=False)   # our own file
    assert isinstance(saved, shim.ForwardAutoencoder) and type(saved).__module__ == "models.forward_encoder"
    for name in ("decoder.deconv2.weight", "encoder.conv5.weight", "decoder.deconv4_bn.weight"):
        diff = (saved.state_dict()[name].cpu() - state[name].detach()).abs()
        assert float(diff.mean()) <= 0.05 * LR, (name, float(diff.mean()))
    np.testing.assert_allclose(saved.state_dict()["decoder.deconv5_bn.running_var"].cpu().numpy(),
                               state["decoder.deconv5_bn.running_var"].numpy(), rtol=1e-3)


def _fm_rank_main(rank, world, port, cfg_dict, out_dir):
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", NDP_DIST_BACKEND="gloo", NDP_BENCH_ONE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from ndivplanning_amd import train_forward_model as script
    from ndivplanning_amd.utils.file import AttrDict
    initial = {}
    real_trainer = script.ForwardModelTrainer

    def spy(model, **kw):
        initial.update({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
        return real_trainer(model, **kw)
    script.ForwardModelTrainer = spy
    hist = script.train(AttrDict(cfg_dict))
    tr = script.train.last_trainer
    torch.save({"params": tr.params.cpu(), "stats": tr.stats.cpu(), "hist": hist, "initial": initial,
                "named": {k: v.cpu() for k, v in tr.named_parameters().items()}}, os.path.join(out_dir, "fm_rank%d.pt" % rank))
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_average_their_gradients(tmp_path):
    """train_forward_model.train under two processes (both on cuda:0, gloo): each rank takes half of every global batch,
    the flat gradient is averaged between backward and Adam, BatchNorm statistics stay per rank (torch DDP's recipe).
    Replicas must stay bit-identical; the result must be what the oracle gives when it is driven the same way."""
    import socket
    import torch.multiprocessing as mp
    from ndivplanning_amd.train_gan import make_dataset
    from ndivplanning_amd.utils.file import AttrDict
    torch.set_num_threads(8)
    cfg = {"random_seed": 0, "train_data_path": "synthetic:4:images", "gpu_id": 0, "trajectory_length": 3,
           "forward_save_path": str(tmp_path / "fm"),
           "training": {"forward": {"num_epochs": 1, "learning_rate": LR, "report_feq": 10, "batch_size": 4,
                                    "epochs_per_stage": 1, "step_lr_gamma": 0.1, "sync_batchnorm": False}}}
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_fm_rank_main, args=(2, port, cfg, str(tmp_path)), nprocs=2, join=True)
    res = [torch.load(str(tmp_path / ("fm_rank%d.pt" % r))) for r in range(2)]
    assert torch.equal(res[0]["params"], res[1]["params"])                 # replicas in lockstep
    assert not torch.equal(res[0]["stats"], res[1]["stats"])               # BatchNorm statistics are each rank's own
    assert res[0]["hist"] == res[1]["hist"] and len(res[0]["hist"]) == 1
    assert all(torch.equal(res[0]["initial"][k], res[1]["initial"][k]) for k in res[0]["initial"])
    assert os.path.isfile(str(tmp_path / "fm" / "forward_autoencoder_0.pt"))
    # ---- the same thing with the oracle: shared parameters, one set of BatchNorm buffers per rank
    acfg = AttrDict(cfg)
    torch.manual_seed(0)
    np.random.seed(0)
    from ndivplanning_amd.models import forward_encoder as FE
    FE.ForwardAutoencoder()                                                # the CPU stream position of the run
    ds = make_dataset(acfg)
    loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=True)
    state = {k: v.clone() for k, v in res[0]["initial"].items()}
    names = FO.trainable(state)
    used = [n for n in names if not n.startswith(("encoder.conv4_bn", "encoder.conv5_bn"))]
    for n in used:
        state[n].requires_grad_(True)
    opt = torch.optim.Adam([state[n] for n in used], lr=LR, betas=(0.5, 0.999))
    views = [state, dict(state)]
    for k in state:
        if "running_" in k or "num_batches" in k:
            views[1][k] = state[k].clone()
    losses = []
    for images, _, actions, _ in loader:
        for i in range(ds.seq_length - 1):
            grads, step_loss = None, 0.0
            for r in range(2):
                cur, fut, act = images[2 * r:2 * r + 2, i], images[2 * r:2 * r + 2, i + 1], actions[2 * r:2 * r + 2, i]
                loss = torch.nn.functional.mse_loss(FO.forward(views[r], cur, act, training=True), fut - cur)
                g = torch.autograd.grad(loss, [state[n] for n in used])
                grads = list(g) if grads is None else [a + b for a, b in zip(grads, g)]
                step_loss += loss.item() / 2
            for n, g in zip(used, grads):
                state[n].grad = g / 2
            opt.step()
            losses.append(step_loss)
    assert abs(res[0]["hist"][0] - sum(losses) / len(losses)) <= 5e-5
    for name in ("decoder.deconv2.weight", "encoder.conv5.weight", "decoder.conv_refine_1.weight"):
        diff = (res[0]["named"][name] - state[name].detach()).abs()
        assert float(diff.mean()) <= 0.05 * LR, (name, float(diff.mean()))
    # ---- that run averaged the gradient bucket by bucket on a communication stream (the default); ONE collective between
    # backward and Adam (`grad_exchange: single`) must give the same bits: two ranks, one addition per element
    cfg["training"]["forward"]["grad_exchange"] = "single"
    single_dir = tmp_path / "single"
    single_dir.mkdir()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_fm_rank_main, args=(2, port, cfg, str(single_dir)), nprocs=2, join=True)
    single = torch.load(str(single_dir / "fm_rank0.pt"))
    assert torch.equal(single["params"], res[0]["params"]) and single["hist"] == res[0]["hist"]


def test_two_ranks_with_cross_rank_batchnorm_train_the_single_process_step(tmp_path):
    """`batch_size` is the global batch.  Two ranks with 2 images each, BatchNorm statistics summed over the ranks (the
    fixed-point accumulators all-reduced as int64: exact, order-free) and gradients averaged, against ONE process on the
    same 4 images per step: the same losses, the same running statistics on every rank, the same parameters -- up to the
    fp32 summation order inside a tile and Adam's +-lr on the biases whose gradient is rounding noise."""
    import socket
    import torch.multiprocessing as mp
    from ndivplanning_amd import train_forward_model as script
    from ndivplanning_amd.utils.file import AttrDict
    cfg = {"random_seed": 0, "train_data_path": "synthetic:4:images", "gpu_id": 0, "trajectory_length": 3,
           "forward_save_path": str(tmp_path / "fm"),
           "training": {"forward": {"num_epochs": 1, "learning_rate": LR, "report_feq": 10, "batch_size": 4,
                                    "epochs_per_stage": 1, "step_lr_gamma": 0.1}}}       # sync_batchnorm: the default
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_fm_rank_main, args=(2, port, cfg, str(tmp_path)), nprocs=2, join=True)
    res = [torch.load(str(tmp_path / ("fm_rank%d.pt" % r))) for r in range(2)]
    assert torch.equal(res[0]["params"], res[1]["params"])                 # replicas in lockstep
    assert torch.equal(res[0]["stats"], res[1]["stats"])                   # ... running statistics included: they are global
    # the same epoch in this process, alone, on the whole batch
    single_cfg = AttrDict(cfg)
    single_cfg["forward_save_path"] = str(tmp_path / "single")
    hist = script.train(single_cfg)
    tr = script.train.last_trainer
    assert abs(hist[0] - res[0]["hist"][0]) <= 2e-6 * max(1.0, abs(hist[0]))
    # (a tile's fp32 column sum groups its rows differently when the tile holds one rank's images or both ranks': 1e-7 of
    # sum x^2, which var = E[x^2] - mean^2 amplifies where a channel's mean dominates its spread: measured 3e-5)
    stats = tr.stats.cpu()
    assert float((stats - res[0]["stats"]).abs().max()) <= 1e-4 * float(stats.abs().max())
    mine = {k: v.cpu() for k, v in tr.named_parameters().items()}
    worst, off, total = 0.0, 0, 0
    for name, want in mine.items():
        if name in NOISE_BIASES:
            continue
        diff = (res[0]["named"][name] - want).abs()
        worst = max(worst, float(diff.max()))
        off += int((diff > 2e-5).sum())
        total += diff.numel()
    # two Adam steps of lr 2e-4: the gradients agree to ~1e-5 of their tensor's norm (next test), but Adam's first steps
    # are lr * sign(g) whatever |g| is, and in a network this sparse ~1 % of the 33 M elements have a gradient inside that
    # noise and may step the other way, 2 lr = 4e-4 apart (measured: 1.1 %)
    assert worst <= 2.5 * 2 * LR and off <= 0.05 * total, (worst, off, total)


def _syncbn_rank(rank, world, port, out_dir):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      NDP_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from ndivplanning_amd import dp
    dp.init_process_group(DEV)
    tr, _ = _hip_trainer(3, 2, sync_batchnorm_world=world)
    frames, actions = _inputs(7, 4)
    sl = slice(2 * rank, 2 * rank + 2)
    tr.grads(frames[sl, 0].contiguous().to(DEV), frames[sl, 1].contiguous().to(DEV), actions[sl, 0].contiguous().to(DEV))
    g = tr.grad.clone()
    dp.mean_all_reduce(world)(g)
    torch.save({"grad": g.cpu(), "loss": tr.loss.item(), "stats": tr.stats.cpu(), "calls": tr.stat_sync.calls},
               os.path.join(out_dir, "syncbn%d.pt" % rank))
    tr.close()
    dist.destroy_process_group()


def test_cross_rank_batchnorm_gives_the_global_batch_gradient(tmp_path):
    """ndp_fm_train_grads_dp / dp.StatAllReduce at the gradient level: two ranks with 2 images each -- every BatchNorm's
    fixed-point accumulator all-reduced as int64 between the kernel that fills it and the kernel that reads it (10 forward
    + 10 backward callbacks per rank), d beta / d gamma from each rank's own sums, dx from the global ones -- then the mean
    of the two flat gradients, against ONE process on the 4 images: same loss, same running statistics, every gradient
    tensor within 1e-4 of its norm (measured 2e-7 ... 3e-5; the biases in front of a BatchNorm are rounding noise)."""
    import socket
    import torch.multiprocessing as mp
    from ndivplanning_amd.models import forward_encoder as FE
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_syncbn_rank, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    res = [torch.load(str(tmp_path / ("syncbn%d.pt" % r))) for r in range(2)]
    assert res[0]["calls"] == res[1]["calls"] == 20
    tr, _ = _hip_trainer(3, 4)
    frames, actions = _inputs(7, 4)
    tr.grads(frames[:, 0].contiguous().to(DEV), frames[:, 1].contiguous().to(DEV), actions[:, 0].contiguous().to(DEV))
    assert abs(tr.loss.item() - (res[0]["loss"] + res[1]["loss"]) / 2) <= 1e-6
    assert abs(res[0]["loss"] - res[1]["loss"]) > 1e-4                    # (the ranks did see different images)
    assert torch.equal(res[0]["stats"], res[1]["stats"])
    assert float((tr.stats.cpu() - res[0]["stats"]).abs().max()) <= 1e-5
    want = FE.unpack_vector(tr.grad, tr.model)
    got = FE.unpack_vector(res[0]["grad"].to(DEV), tr.model)
    for name in want:
        if name in NOISE_BIASES:
            continue
        assert _rel(got[name], want[name]) <= 1e-4, (name, _rel(got[name], want[name]))


def test_gradient_buckets_cover_the_flat_vector_in_completion_order():
    """ndp_fm_grad_buckets: 7 disjoint ranges that tile the flat gradient; the last layers (whose weight gradients the
    backward pass finishes first) come first, deconv2 -- half of all parameters -- has a bucket of its own."""
    from ndivplanning_amd import _capi
    lib = _capi.load()
    buckets = _capi.fm_grad_buckets()
    total = lib.ndp_fm_param_floats()
    assert len(buckets) == 7 and sum(c for _, c in buckets) == total
    covered = sorted(buckets)
    assert covered[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(covered, covered[1:])) and covered[-1][0] + covered[-1][1] == total
    import ctypes
    off, dims = ctypes.c_int64(), (ctypes.c_int64 * 6)()
    _capi.check(lib.ndp_fm_layout(0, 7, ctypes.byref(off), dims), "ndp_fm_layout")      # decoder.deconv2
    assert buckets[2][0] == off.value and buckets[2][1] == 2048 * 16 * 512 + 512
    assert buckets[0][0] > buckets[1][0] > buckets[2][0] > buckets[3][0] > buckets[4][0] > buckets[5][0] == 0
    # a backward pass records the events; waiting for them on a second stream orders that stream behind the pass
    tr, _ = _hip_trainer(0, 2)
    frames, actions = _inputs(1, 2)
    cur, fut, act = (t.contiguous().to(DEV) for t in (frames[:, 0], frames[:, 1], actions[:, 0]))
    tr.grads(cur, fut, act)
    side = torch.cuda.Stream(DEV)
    sums = []
    with torch.cuda.stream(side):
        for b, (o, c) in enumerate(buckets):
            _capi.check(lib.ndp_fm_bucket_wait(b, _capi.stream_ptr(DEV)), "ndp_fm_bucket_wait")
            sums.append(tr.grad[o:o + c].double().abs().sum())
    torch.cuda.synchronize(DEV)
    want = [tr.grad[o:o + c].double().abs().sum().item() for o, c in buckets]
    assert [s_.item() for s_ in sums] == want and all(w > 0 for w in want)


def test_train_grads_dp_without_a_function_is_train_grads_bit_for_bit():
    """ndp_fm_train_grads_dp(stat_sync=NULL, world=1) against ndp_fm_train_grads (float frames) and ndp_fm_train_grads_u8
    (byte frames, frames_u8=1): the same launches, so the same bits in grad, loss, running statistics and residual.  A world
    size outside 1..4096 is NDP_E_ARG and launches nothing."""
    from ndivplanning_amd import _capi
    lib, p = _capi.load(), _capi.ptr
    tr, _ = _hip_trainer(5, 2, keep_residual=True)
    frames, actions = _inputs(11, 2)
    act = actions[:, 0].contiguous().to(DEV)
    f32 = [frames[:, i].contiguous().to(DEV) for i in (0, 1)]
    u8 = [((f.permute(0, 2, 3, 1) + 1.0) * 127.5).round().clamp(0, 255).to(torch.uint8).contiguous() for f in f32]
    stats0 = tr.stats.clone()

    def run(name, cur, fut, *dp):
        tr.stats.copy_(stats0)
        for t in (tr.grad, tr.loss, tr.resid):
            t.zero_()
        flag = [int(cur.dtype == torch.uint8)] if dp else []
        with torch.cuda.device(DEV):
            rc = getattr(lib, name)(p(tr.params), p(tr.stats), p(cur), p(fut), *flag, p(act), 2, p(tr.grad), p(tr.loss), None,
                                    p(tr.resid), p(tr.workspace), _capi.stream_ptr(DEV), *dp)
        torch.cuda.synchronize(DEV)
        return rc, [t.clone() for t in (tr.grad, tr.loss, tr.stats, tr.resid)]
    for name, (cur, fut) in (("ndp_fm_train_grads", f32), ("ndp_fm_train_grads_u8", u8)):
        rc, want = run(name, cur, fut)
        assert rc == 0 and float(want[0].abs().sum()) > 0 and not torch.equal(want[2], stats0)
        rc, got = run("ndp_fm_train_grads_dp", cur, fut, None, None, 1)
        assert rc == 0
        for g, w, what in zip(got, want, ("grad", "loss", "running_stats", "resid_out")):
            assert torch.equal(g, w), (name, what)
    for world in (0, 4097):
        rc, got = run("ndp_fm_train_grads_dp", f32[0], f32[1], None, None, world)
        assert rc == 1 and b"ndp_fm_train_grads_dp" in lib.ndp_last_error()              # NDP_E_ARG
        assert not got[0].any() and not got[1].any() and not got[3].any() and torch.equal(got[2], stats0)


def _isolation_child(rank, port):
    import gc
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1",
                      NDP_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from ndivplanning_amd import _capi, dp
    from ndivplanning_amd.models import forward_encoder as FE
    lib = _capi.load()
    with torch.cuda.device(DEV):
        assert lib.ndp_fm_bucket_wait(0, _capi.stream_ptr(DEV)) == 1                     # NDP_E_ARG: no pass yet
    assert b"ndp_fm_bucket_wait" in lib.ndp_last_error()
    dp.init_process_group(DEV, force=True)
    frames, actions = _inputs(7, 2)
    cur, fut, act = (t.contiguous().to(DEV) for t in (frames[:, 0], frames[:, 1], actions[:, 0]))
    B, state = _hip_trainer(3, 2)
    B.grads(cur, fut, act)
    g0, loss0 = B.grad.clone(), B.loss.clone()
    A, _ = _hip_trainer(3, 2, sync_batchnorm_world=2)
    A.grads(cur, fut, act)
    stat = A.stat_sync
    assert stat.calls == 20
    B.grads(cur, fut, act)                                     # another trainer in the process: never through A's function
    assert torch.equal(B.grad, g0) and torch.equal(B.loss, loss0) and stat.calls == 20
    model = FE.ForwardAutoencoder()                            # the module's autograd path (ndp_fm_forward / ndp_fm_backward)
    model.load_state_dict(state)
    model = model.to(DEV).train()
    torch.nn.functional.mse_loss(model(cur, act), fut - cur).backward()
    assert model.encoder.conv1.weight.grad is not None and stat.calls == 20
    A.close()
    with pytest.raises(_capi.NdpError):
        A.grads(cur, fut, act)
    del A, stat
    gc.collect()
    B.grads(cur, fut, act)                                     # nothing dangles behind a trainer that is gone
    assert torch.equal(B.grad, g0)
    torch.cuda.synchronize(DEV)
    dist.destroy_process_group()


def test_cross_rank_statistics_stay_with_the_trainer_that_asked_for_them():
    """The statistics function travels with ndp_fm_train_grads_dp calls of ONE trainer: a plain trainer and the module's
    autograd path in the same process never call it, a closed trainer refuses, and after the trainer is collected the
    library holds no pointer to it.  ndp_fm_bucket_wait before any backward pass has nothing to wait for.  One child
    process with a one-rank gloo group."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_isolation_child, args=(port,), nprocs=1, join=True)


def test_the_reference_loop_unchanged_module_forward_loss_backward_torch_adam():
    """train_forward_model.py:102-110 as written -- `resid = model(cur, a); loss = mse(resid, fut - cur);
    optimizer.zero_grad(); loss.backward(); optimizer.step()` -- with the mirror module and torch's own Adam: the residual's
    grad_fn runs the HIP backward pass (ndp_fm_backward), gradients arrive in the parameters' .grad in the module's layouts."""
    from ndivplanning_amd.models import forward_encoder as FE
    torch.set_num_threads(8)
    n = 2
    state = FO.init_forward_model_state(41)
    model = FE.ForwardAutoencoder()
    model.load_state_dict(state)
    model = model.to(DEV).train()
    mse = torch.nn.MSELoss()
    opt = torch.optim.Adam([{"params": model.decoder.parameters()}, {"params": model.encoder.parameters()}], lr=LR,
                           betas=(0.5, 0.999))
    oracle = FO.ForwardModelTrainer(state, lr=LR)
    frames, actions = _inputs(42, n)
    for it in range(2):
        cur, fut, act = (t.contiguous().to(DEV) for t in (frames[:, it], frames[:, it + 1], actions[:, it]))
        resid = model(cur, act)
        assert resid.requires_grad and resid.grad_fn is not None
        loss = mse(resid, fut - cur)
        opt.zero_grad()
        loss.backward()
        want = oracle.step(frames[:, it].contiguous(), frames[:, it + 1].contiguous(), actions[:, it].contiguous())
        assert abs(loss.item() - want["loss"].item()) <= (1e-5 if it == 0 else 2e-4)
        if it == 0:
            for name, p in model.named_parameters():
                ref = want["grads"][name]
                if ref is None:
                    assert p.grad is None, name               # conv4_bn / conv5_bn: never applied
                elif name not in NOISE_BIASES:
                    assert _rel(p.grad.cpu(), ref) <= 2e-2, (name, _rel(p.grad.cpu(), ref))   # flip-tolerant, see above
        opt.step()
    assert int(model.decoder.deconv4_bn.num_batches_tracked) == 2
    with pytest.raises(NotImplementedError):
        model(frames[:, 0].to(DEV).requires_grad_(True), actions[:, 0].to(DEV))
    # a second forward invalidates the first one's activations: its backward must refuse, not compute garbage
    r1 = model(frames[:, 0].to(DEV), actions[:, 0].to(DEV))
    model(frames[:, 1].to(DEV), actions[:, 1].to(DEV))
    from ndivplanning_amd import _capi
    with pytest.raises(_capi.NdpError):
        r1.sum().backward()


def test_cli_entry_in_a_fresh_interpreter_pickles_the_reference_class_path(tmp_path):
    """`python train_forward_model.py --config-file ...` (the reference's command line) in a new interpreter: the saved
    whole-module checkpoint must record `models.forward_encoder.ForwardAutoencoder` (what control_evaluation.py:177-180
    unpickles), not the package-internal path, and load back into the mirror on the kernels' path."""
    import subprocess
    import sys
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    save = tmp_path / "fm"
    save.mkdir()
    cfg = {"random_seed": 0, "train_data_path": "synthetic:2:images", "gpu_id": 0, "trajectory_length": 2,
           "forward_save_path": str(save),
           "training": {"forward": {"num_epochs": 1, "learning_rate": LR, "report_feq": 10, "batch_size": 2,
                                    "epochs_per_stage": 1, "step_lr_gamma": 0.1}}}
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    res = subprocess.run([sys.executable, os.path.join(root, "train_forward_model.py"), "--config-file", str(tmp_path / "cfg.yaml"),
                          "--forward-save-path", str(save)], cwd=root, env=dict(os.environ, PYTHONPATH=root),
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:]
    path = save / "forward_autoencoder_0.pt"
    blob = open(path, "rb").read()
    assert b"models.forward_encoder" in blob and b"ndivplanning_amd.models" not in blob
    import models.forward_encoder as shim
    model = torch.load(str(path), weights_only=False).to(DEV).eval()               # our own file
    assert isinstance(model, shim.ForwardAutoencoder)
    frames, actions = _inputs(50, 1)
    pred = model(frames[:, 0].to(DEV), actions[:, 0].to(DEV))
    assert pred.shape == (1, 3, 128, 128) and bool(torch.isfinite(pred).all())


def test_weight_init_after_a_forward_is_seen_by_the_next_forward():
    """The reference's `__main__` pattern (forward_encoder.py:117-131): construct, run, then re-initialise.  The module keeps
    packed copies of its parameters between forwards; weight_init (and any in-place write through torch, or
    invalidate_cache() after a write through `.data`) must make the next forward read the new weights."""
    from ndivplanning_amd.models import forward_encoder as FE
    torch.manual_seed(3)
    model = FE.ForwardAutoencoder().to(DEV).eval()
    gen = torch.Generator().manual_seed(9)
    x = (torch.rand(2, 3, 128, 128, generator=gen) * 2 - 1).to(DEV)
    a = (torch.rand(2, 4, generator=gen) * 2 - 1).to(DEV)
    with torch.no_grad():
        y0 = model(x, a).clone()
        assert torch.equal(model(x, a), y0)                               # cached packed parameters, same result
        model.encoder.weight_init(0.0, 0.02)
        model.decoder.weight_init(0.0, 0.02)
        y1 = model(x, a).clone()
        want = FO.forward({k: v.cpu() for k, v in model.state_dict().items()}, x.cpu(), a.cpu(), training=False)
        assert (y1 - y0).abs().max().item() > 1e-3                        # the new weights were used ...
        assert (y1.cpu() - want).abs().max().item() <= 5e-5               # ... and give the oracle's output for them
        model.decoder.conv_refine_2.bias.data.add_(0.25)                  # a write through .data bumps no version counter
        model.invalidate_cache()
        y2 = model(x, a)
        want2 = FO.forward({k: v.cpu() for k, v in model.state_dict().items()}, x.cpu(), a.cpu(), training=False)
        assert (y2 - y1).abs().max().item() > 1e-2 and (y2.cpu() - want2).abs().max().item() <= 5e-5


def test_byte_frames_train_exactly_as_the_floats_the_reference_would_upload():
    """ndp_fm_train_grads_u8 / ndp_fm_forward_u8: frames [n,128,128,3] as bytes, normalised where they are read (the input
    gather and the loss target) with utils/hdf5_load.py:9-11's formula.  Two training iterations from byte frames and from
    the float tensors built from the same bytes give bit-identical losses, gradients and parameters."""
    lut = torch.from_numpy(load_golden("frames_case")["lut"])
    gen = torch.Generator().manual_seed(21)
    frames = torch.randint(0, 256, (3, 3, 128, 128, 3), generator=gen, dtype=torch.uint8)      # [n, t, H, W, C]
    actions = torch.rand(3, 3, 4, generator=gen) * 2 - 1
    floats = lut[frames.long()].permute(0, 1, 4, 2, 3).contiguous()                            # [n, t, 3, H, W]
    tr8, _ = _hip_trainer(5, 3, keep_residual=True)
    trf, _ = _hip_trainer(5, 3, keep_residual=True)
    for it in range(2):
        act = actions[:, it].contiguous().to(DEV)
        tr8.step(frames[:, it].contiguous().to(DEV), frames[:, it + 1].contiguous().to(DEV), act)
        grad8 = tr8.grad.clone()
        trf.step(floats[:, it].contiguous().to(DEV), floats[:, it + 1].contiguous().to(DEV), act)
        assert torch.equal(tr8.loss, trf.loss) and torch.equal(tr8.resid, trf.resid)
        assert torch.equal(grad8, trf.grad) and torch.equal(tr8.params, trf.params)
    assert float(tr8.loss) > 0
    with pytest.raises(Exception):
        tr8.step(frames[:, 0].contiguous().to(DEV), floats[:, 1].contiguous().to(DEV), actions[:, 0].contiguous().to(DEV))
    # the module's eval-mode forward (state_cur + residual) from bytes
    model = tr8.sync_to_module().eval()
    with torch.no_grad():
        y8 = model(frames[:, 0].contiguous().to(DEV), actions[:, 0].contiguous().to(DEV))
        yf = model(floats[:, 0].contiguous().to(DEV), actions[:, 0].contiguous().to(DEV))
    assert y8.shape == (3, 3, 128, 128) and torch.equal(y8, yf)


def test_the_optimizer_launch_leaves_the_second_weight_order_a_full_repack_would():
    """ndp_fm_apply_adam writes the new weights in both orders in one launch (k_fm_adam_pack: 32 x 32 tiles transposed
    through LDS, conv1's compact [64][32] copy and the refinement layers' [ci][tap][co] copies written element by element).
    ndp_fm_pack_params rebuilds the second order from the parameters alone: after two training steps it must change
    nothing -- the fixed head of the workspace (second weight order + statistics scratch) stays bit-identical."""
    from ndivplanning_amd import _capi
    n = 3
    tr, _ = _hip_trainer(5, n)
    frames, actions = _inputs(9, n)
    cur, fut, act = (t.contiguous().to(DEV) for t in (frames[:, 0], frames[:, 1], actions[:, 0]))
    for _ in range(2):
        tr.step(cur, fut, act)
    torch.cuda.synchronize()
    head = tr.lib.ndp_fm_workspace_offset(n, 0)
    assert head > 30_000_000                                       # the second order of 33 M weights lives there
    before = tr.workspace[:head].view(torch.int32).clone()         # bits: the scratch words behind the weights may hold anything
    _capi.check(tr.lib.ndp_fm_pack_params(_capi.ptr(tr.params), _capi.ptr(tr.workspace), _capi.stream_ptr(DEV)),
                "ndp_fm_pack_params")
    torch.cuda.synchronize()
    assert torch.equal(before, tr.workspace[:head].view(torch.int32))
    # and the copy is in use: a forward pass right after the repack gives the same loss as one before it
    tr.grads(cur, fut, act)
    loss_a = tr.loss.item()
    tr.grads(cur, fut, act)
    assert tr.loss.item() == loss_a


# {label: launches} of one training step of each network and one eval-mode decode at n = 2, every launch on the caller's
# stream: the kernel-timer names are what bench.py and the profiles filter on (prefixes such as "k_fm_gemm[deconv"), so
# they are pinned here byte for byte, with how often each is launched.
FM_STEP_LAUNCHES = {
    "k_fm_adam_pack": 1, "k_fm_bias_finish": 3, "k_fm_bn_apply": 10, "k_fm_bn_bwd_apply": 10, "k_fm_dgrad[conv2]": 1,
    "k_fm_dgrad[conv3]": 1, "k_fm_dgrad[conv4]": 1, "k_fm_dgrad[conv5]": 1, "k_fm_dgrad[conv6]": 1,
    "k_fm_dgrad[deconv1]": 1, "k_fm_dgrad[deconv2]": 1, "k_fm_dgrad[deconv3]": 1, "k_fm_dgrad[deconv4]": 1,
    "k_fm_dgrad[deconv5]": 1, "k_fm_dgrad[deconv6]": 1, "k_fm_dgrad[refine1]": 1, "k_fm_gemm[conv1]": 1,
    "k_fm_gemm[conv2]": 1, "k_fm_gemm[conv3]": 1, "k_fm_gemm[conv4]": 1, "k_fm_gemm[conv5]": 1, "k_fm_gemm[conv6]": 1,
    "k_fm_gemm[deconv1]": 1, "k_fm_gemm[deconv2]": 1, "k_fm_gemm[deconv3]": 1, "k_fm_gemm[deconv4]": 1,
    "k_fm_gemm[deconv5]": 1, "k_fm_gemm[deconv6]": 1, "k_fm_gemm[refine1]": 1, "k_fm_image_cols": 1,
    "k_fm_r2_dgrad": 1, "k_fm_r2_fwd": 1, "k_fm_r2_wgrad": 1, "k_fm_slab_sum": 2, "k_fm_splitk_reduce": 19,
    "k_fm_wgrad[conv1]": 1, "k_fm_wgrad[conv2]": 1, "k_fm_wgrad[conv3]": 1, "k_fm_wgrad[conv4]": 1,
    "k_fm_wgrad[conv5]": 1, "k_fm_wgrad[conv6]": 1, "k_fm_wgrad[deconv1]": 1, "k_fm_wgrad[deconv2]": 1,
    "k_fm_wgrad[deconv3]": 1, "k_fm_wgrad[deconv4]": 1, "k_fm_wgrad[deconv5]": 1, "k_fm_wgrad[deconv6]": 1,
    "k_fm_wgrad[refine1]": 1,
}
AE_STEP_LAUNCHES = {
    "k_ae_out_dgrad": 1, "k_ae_out_fwd_loss": 1, "k_ae_out_wgrad": 1, "k_fm_adam_pack": 1, "k_fm_bias_finish": 3,
    "k_fm_bn_apply": 8, "k_fm_bn_bwd_apply": 8, "k_fm_dgrad[ae.conv2]": 1, "k_fm_dgrad[ae.conv3]": 1,
    "k_fm_dgrad[ae.conv4]": 1, "k_fm_dgrad[ae.conv5]": 1, "k_fm_dgrad[ae.conv6]": 1, "k_fm_dgrad[ae.deconv1]": 1,
    "k_fm_dgrad[ae.deconv2]": 1, "k_fm_dgrad[ae.deconv3]": 1, "k_fm_dgrad[ae.deconv4]": 1,
    "k_fm_dgrad[ae.deconv5]": 1, "k_fm_gemm[ae.conv1]": 1, "k_fm_gemm[ae.conv2]": 1, "k_fm_gemm[ae.conv3]": 1,
    "k_fm_gemm[ae.conv4]": 1, "k_fm_gemm[ae.conv5]": 1, "k_fm_gemm[ae.conv6]": 1, "k_fm_gemm[ae.deconv1]": 1,
    "k_fm_gemm[ae.deconv2]": 1, "k_fm_gemm[ae.deconv3]": 1, "k_fm_gemm[ae.deconv4]": 1, "k_fm_gemm[ae.deconv5]": 1,
    "k_fm_image_cols": 1, "k_fm_slab_sum": 1, "k_fm_splitk_reduce": 18, "k_fm_wgrad[ae.conv1]": 1,
    "k_fm_wgrad[ae.conv2]": 1, "k_fm_wgrad[ae.conv3]": 1, "k_fm_wgrad[ae.conv4]": 1, "k_fm_wgrad[ae.conv5]": 1,
    "k_fm_wgrad[ae.conv6]": 1, "k_fm_wgrad[ae.deconv1]": 1, "k_fm_wgrad[ae.deconv2]": 1, "k_fm_wgrad[ae.deconv3]": 1,
    "k_fm_wgrad[ae.deconv4]": 1, "k_fm_wgrad[ae.deconv5]": 1,
}
AE_DECODE_LAUNCHES = {
    "k_ae_out_fwd": 1, "k_fm_gemm[aed.deconv1]": 1, "k_fm_gemm[aed.deconv2]": 1, "k_fm_gemm[aed.deconv3]": 1,
    "k_fm_gemm[aed.deconv4]": 1, "k_fm_gemm[aed.deconv5]": 1, "k_fm_splitk_reduce": 4,
}


def test_the_kernel_timer_labels_and_launch_counts_of_a_step_stay_as_they_are():
    from ndivplanning_amd import _capi
    from ndivplanning_amd import autoencoder_eval as AE
    from ndivplanning_amd.autoencoder_trainer import AutoencoderTrainer
    from ndivplanning_amd.models import image_autoencoder as IA
    n = 2
    tr, _ = _hip_trainer(5, n)
    frames, actions = _inputs(9, n)
    cur, fut, act = (t.contiguous().to(DEV) for t in (frames[:, 0], frames[:, 1], actions[:, 0]))
    torch.manual_seed(3)
    enc, dec = IA.Encoder().to(DEV).train(), IA.Decoder().to(DEV).train()
    ae = AutoencoderTrainer(enc, dec, batch=n)
    codes = torch.randn(n, 128, device=DEV)
    AE.decode(dec.eval(), codes)                                       # (the folded parameters are packed on first use)
    dec.train()
    torch.cuda.synchronize()

    def launches(fn):
        fn()
        torch.cuda.synchronize()
        got = _capi.timing_collect()
        assert len(got) < 64                                           # (timing_collect reports at most 64 names)
        return {k: v[1] for k, v in got.items()}

    side = tr.lib.ndp_fm_side_stream(0)
    _capi.timing_enable(True)
    try:
        fm_step = launches(lambda: tr.step(cur, fut, act))
        ae_step = launches(lambda: ae.step(cur))
        dec.eval()
        decode = launches(lambda: AE.decode(dec, codes))
    finally:
        _capi.timing_enable(False)
        tr.lib.ndp_fm_side_stream(side)
    for name, got in (("FM_STEP_LAUNCHES", fm_step), ("AE_STEP_LAUNCHES", ae_step), ("AE_DECODE_LAUNCHES", decode)):
        print("%s = %r" % (name, dict(sorted(got.items()))))
    assert fm_step == FM_STEP_LAUNCHES
    assert ae_step == AE_STEP_LAUNCHES
    assert decode == AE_DECODE_LAUNCHES
