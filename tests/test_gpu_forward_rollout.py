"""GPU tests of multi-step rollout training of the forward model: ndp_fm_backward_inputs, the
rollout link kernels and the gradient sum through ForwardModelTrainer.grads_rollout / step_rollout and
train_forward_model.train, against the definition restated on the oracle (tests/rollout_common.py).

Comparison rule (tests/test_gpu_forward_model.py, tests/test_gpu_input_grad.py): with _rel(a, b) = |a - b| / |b| in fp64,
the kernels' error against the fp64 oracle may be at most max(2e-5, 2 x the fp32 CPU oracle's error against the same fp64
result).  The ReLU decisions of the run under test are injected into both oracles, per pass; the biases in front of a
BatchNorm (NOISE_BIASES: zero gradient but for rounding) are held to 1e-4 of their weight gradient's scale."""
import numpy as np
import pytest
import torch

import rollout_common as C
import trained_state as TS
from oracle import forward_model_oracle as FO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR = 2e-4


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _check(mine, ref32, ref64, what):
    assert torch.isfinite(torch.as_tensor(mine)).all(), what
    err_mine, err_ref = _rel(mine, ref64), _rel(ref32, ref64)
    print("%s: kernels %.3e, fp32 oracle %.3e" % (what, err_mine, err_ref))
    assert err_mine <= max(2e-5, 2.0 * err_ref), (what, err_mine, err_ref)


def _trainer(seed, n, trained=False, **kw):
    """trained: from a mid-training state (tests/trained_state.py): non-zero biases, BatchNorm weight / bias / running
    statistics off 1 / 0 / 0 / 1, batch counters at 7."""
    from ndivplanning_amd.forward_trainer import ForwardModelTrainer
    from ndivplanning_amd.models import forward_encoder as FE
    state = FO.init_forward_model_state(seed)
    if trained:
        state = TS.trained_like(state, seed)
    model = FE.ForwardAutoencoder()
    model.load_state_dict(state)
    model = model.to(DEV).train()
    return ForwardModelTrainer(model, batch=n, lr=LR, **kw), state


def _to64(state):
    return {k: (v.detach().double() if v.is_floating_point() else v.clone()) for k, v in state.items()}


def _byte_window(seed, n, H):
    """Byte frames [n,H+1,128,128,3], the floats the loader would upload [n,H+1,3,128,128], actions [n,H,4]."""
    gen = torch.Generator().manual_seed(seed)
    frames8 = torch.randint(0, 256, (n, H + 1, 128, 128, 3), generator=gen, dtype=torch.uint8)
    actions = torch.rand(n, H, 4, generator=gen) * 2.0 - 1.0
    floats = torch.from_numpy(C.norm_table())[frames8.long()].permute(0, 1, 4, 2, 3).contiguous()
    return frames8, floats, actions


def _masks(tr, n, H):
    return [{site: (tr.activation(site, n, step=k) > 0).cpu() for site in FO.RELU_SITES} for k in range(H)]


def _check_grads(tr, want, exact, what):
    grads = tr.named_gradients()
    for name, ref in want["grads"].items():
        if ref is None:
            assert name not in grads
            continue
        mine = grads[name].cpu()
        if name in C.NOISE_BIASES:
            wscale = float(want["grads"][name[:-4] + "weight"].abs().max())
            assert float(mine.abs().max()) <= 1e-4 * wscale, (what, name)
            continue
        _check(mine, ref, exact["grads"][name], "%s %s" % (what, name))


def _check_window(tr, state, floats, actions, n, H, what, guard=False):
    """The trainer's last grads_rollout on (floats, actions) against the fp32 and fp64 oracles started from `state`;
    returns the fp64 oracle's state (its running statistics moved H times).  guard (a trained-like state): the window
    stays off the cancellation regime of E[x^2] - mean^2 at every BatchNorm site of every pass."""
    masks = _masks(tr, n, H)
    state32 = {k: v.detach().clone() for k, v in state.items()}
    state64 = _to64(state)
    want = C.rollout_grads(state32, floats, actions, masks)
    with TS.record_mean2_over_var(FO) as seen:
        exact = C.rollout_grads(state64, floats.double(), actions.double(), masks)
    if guard:
        TS.assert_guard(seen, 10 * H)
    _check(tr.loss.cpu()[0], want["loss"], exact["loss"], what + " L")
    _check(tr.rollout_losses.cpu(), torch.stack(want["losses"]), torch.stack(exact["losses"]), what + " rollout_losses")
    assert abs(float(tr.rollout_losses.double().mean()) - float(tr.loss)) <= 1e-6 * float(tr.loss)
    _check_grads(tr, want, exact, what)
    return state64


@pytest.mark.parametrize("n,trained", [pytest.param(1, False, id="1"), pytest.param(3, False, id="3"),
                                       pytest.param(3, True, id="trained-3")])
def test_backward_inputs_gives_backwards_gradient_and_the_input_gradients(n, trained):
    """ndp_fm_backward_inputs: `grad` bit-identical to ndp_fm_backward's on a second identical forward pass; d_state_cur (the
    data gradient of conv1 alone: no identity term) and d_actions against the oracle's autograd of the training-mode pass;
    either output alone."""
    from ndivplanning_amd import _capi
    torch.set_num_threads(8)
    tr, state = _trainer(50 + n, n, trained)
    lib, p = tr.lib, _capi.ptr
    gen = torch.Generator().manual_seed(60 + n)
    cur = torch.rand(n, 3, 128, 128, generator=gen) * 2.0 - 1.0
    act = torch.rand(n, 4, generator=gen) * 2.0 - 1.0
    d_resid = torch.randn(n, 3, 128, 128, generator=gen) * 1e-4
    cur_d, act_d, dres_d = cur.to(DEV), act.to(DEV), d_resid.to(DEV)
    resid = torch.empty_like(cur_d)

    def forward():
        _capi.check(lib.ndp_fm_forward(p(tr.params), p(tr.stats), p(cur_d), p(act_d), n, 1, p(resid), p(tr.workspace),
                                       _capi.stream_ptr(DEV)), "ndp_fm_forward")

    def backward_inputs(d_cur, d_act):
        grad = torch.full_like(tr.params, float("nan"))
        _capi.check(lib.ndp_fm_backward_inputs(p(tr.params), p(dres_d), n, p(grad), p(d_cur), p(d_act), p(tr.workspace),
                                               _capi.stream_ptr(DEV)), "ndp_fm_backward_inputs")
        return grad
    forward()
    masks = {site: (tr.activation(site, n) > 0).cpu() for site in FO.RELU_SITES}
    grad_a = torch.full_like(tr.params, float("nan"))
    _capi.check(lib.ndp_fm_backward(p(tr.params), p(dres_d), n, p(grad_a), p(tr.workspace), _capi.stream_ptr(DEV)), "ndp_fm_backward")
    forward()
    d_cur, d_act = torch.full_like(cur_d, float("nan")), torch.full_like(act_d, float("nan"))
    grad_b = backward_inputs(d_cur, d_act)
    assert torch.isfinite(grad_a).all() and torch.equal(grad_a, grad_b)
    refs = []
    for dtype in (torch.float32, torch.float64):
        st = {k: (v.detach().to(dtype) if v.is_floating_point() else v.clone()) for k, v in state.items()}
        x, a = cur.to(dtype).requires_grad_(True), act.to(dtype).requires_grad_(True)
        r = FO.forward(st, x, a, training=True, relu_masks=masks)
        refs.append(torch.autograd.grad(r, [x, a], grad_outputs=d_resid.to(dtype)))
    _check(d_cur.cpu(), refs[0][0], refs[1][0], "d_state_cur n=%d" % n)
    _check(d_act.cpu(), refs[0][1], refs[1][1], "d_actions n=%d" % n)
    # each output alone
    forward()
    only_act = torch.full_like(act_d, float("nan"))
    assert torch.equal(backward_inputs(None, only_act), grad_a) and torch.equal(only_act, d_act)
    forward()
    only_cur = torch.full_like(cur_d, float("nan"))
    assert torch.equal(backward_inputs(only_cur, None), grad_a) and torch.equal(only_cur, d_cur)


@pytest.mark.parametrize("n,H,trained", [pytest.param(2, 2, False, id="2-2"), pytest.param(3, 3, False, id="3-3"),
                                         pytest.param(2, 2, True, id="trained-2-2")])
def test_rollout_gradients_losses_and_statistics_match_the_oracle(n, H, trained):
    """grads_rollout from float and from byte frames (the same bits): L, rollout_losses, every parameter gradient and the
    running statistics after the window against the oracle.  n = 3 is odd and below every tile; H = 3 has a middle pass
    with both an upstream and a downstream gradient."""
    torch.set_num_threads(8)
    frames8, floats, actions = _byte_window(70 + n, n, H + 1)       # a longer trajectory tensor: the window is a slice of it
    tr, state = _trainer(80 + n, n, trained, rollout_steps=H)
    tr8, _ = _trainer(80 + n, n, trained, rollout_steps=H)
    fl_d, f8_d, act_d = floats.to(DEV), frames8.to(DEV), actions.to(DEV)
    stats0 = tr8.stats.clone()
    # (slices along the time axis, as train() passes them: only the image stride differs)
    tr.grads_rollout(fl_d[:, 1:H + 2], act_d[:, 1:H + 1])
    tr8.grads_rollout(f8_d[:, 1:H + 2], act_d[:, 1:H + 1])
    assert torch.equal(tr.grad, tr8.grad) and torch.equal(tr.loss, tr8.loss) and torch.equal(tr.rollout_losses, tr8.rollout_losses)
    assert torch.equal(tr.stats, tr8.stats) and torch.equal(tr.loss_sum, tr.loss)
    state64 = _check_window(tr, state, floats[:, 1:H + 2], actions[:, 1:H + 1], n, H, "n=%d, H=%d" % (n, H), guard=trained)
    sd = tr.sync_to_module().state_dict()
    for k, v in sd.items():                                          # the statistics moved H times, in order
        if "running_" in k:
            np.testing.assert_allclose(v.cpu().numpy(), state64[k].numpy(), rtol=1e-3, atol=1e-6, err_msg=k)
        elif k.endswith("num_batches_tracked"):                      # a window of H passes counts H, as torch's BatchNorm does
            unused = k.startswith(("encoder.conv4_bn", "encoder.conv5_bn"))
            assert int(v) == int(state64[k]) == (7 if trained else 0) + (0 if unused else H), k
    assert tr.steps == 0                                             # (Adam steps: none yet)
    # the contiguous window gives the same bits as the slice
    tr8.stats.copy_(stats0)
    tr8.grads_rollout(fl_d[:, 1:H + 2].contiguous(), act_d[:, 1:H + 1].contiguous())
    assert torch.equal(tr.grad, tr8.grad) and torch.equal(tr.stats, tr8.stats)


def test_a_second_window_after_adam_runs_every_pass_on_the_new_weights():
    """step_rollout, then a second window teacher-forced from the trainer's own parameters and statistics after the step:
    the gradients must again meet the rule.  Each pass' workspace keeps a second weight order of its own and Adam rebuilds
    it in the first workspace only: without the repack of the others, passes k >= 1 run on the weights of the step before."""
    torch.set_num_threads(8)
    n, H = 2, 2
    frames8, floats, actions = _byte_window(75, n, H + 1)
    tr, _ = _trainer(85, n, rollout_steps=H)
    fl_d, act_d = floats.to(DEV), actions.to(DEV)
    tr.step_rollout(fl_d[:, 0:H + 1], act_d[:, 0:H])
    before = tr.params.clone()
    sd = {k: v.detach().cpu().clone() for k, v in tr.sync_to_module().state_dict().items()}
    tr.grads_rollout(fl_d[:, 1:H + 2], act_d[:, 1:H + 1])
    assert torch.equal(before, tr.params)
    _check_window(tr, sd, floats[:, 1:H + 2], actions[:, 1:H + 1], n, H, "window 2 (n=%d, H=%d)" % (n, H))


def test_one_rollout_step_is_todays_step_to_the_bit():
    n = 2
    frames8, floats, actions = _byte_window(90, n, 2)
    a, _ = _trainer(91, n, rollout_steps=1)
    b, _ = _trainer(91, n)
    fl_d, act_d = floats.to(DEV), actions.to(DEV)
    for it in range(2):
        a.step_rollout(fl_d[:, it:it + 2], act_d[:, it:it + 1])
        b.step(fl_d[:, it].contiguous(), fl_d[:, it + 1].contiguous(), act_d[:, it].contiguous())
    for name in ("params", "exp_avg", "exp_avg_sq", "stats", "grad", "loss", "loss_sum"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.rollout_losses is None and len(a._workspaces) == 1 and a.steps == 2


def test_rollout_steps_are_bit_reproducible_and_smaller_batches_reuse_the_trainer():
    from ndivplanning_amd import _capi
    n, H = 3, 2
    frames8, floats, actions = _byte_window(92, n, H + 1)
    fl_d, act_d = floats.to(DEV), actions.to(DEV)
    trainers = [_trainer(93, n, rollout_steps=H)[0] for _ in range(2)]
    for tr in trainers:
        for it in range(2):
            tr.step_rollout(fl_d[:, it:it + H + 1], act_d[:, it:it + H])
    a, b = trainers
    for name in ("params", "exp_avg", "exp_avg_sq", "stats", "grad", "loss", "loss_sum", "rollout_losses"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert float(a.loss_sum) > float(a.loss) > 0
    # no host synchronisation in a step: torch raises on any of its own synchronising calls in this mode
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a.step_rollout(fl_d[:, 0:H + 1], act_d[:, 0:H])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    # a ragged final batch: 2 trajectories through the 3-trajectory trainer
    loss = a.step_rollout(fl_d[:2, 0:H + 1].contiguous(), act_d[:2, 0:H].contiguous())
    assert torch.isfinite(loss).all() and torch.isfinite(a.params).all() and torch.isfinite(a.rollout_losses).all()
    with pytest.raises(_capi.NdpError):
        a.grads_rollout(torch.zeros(4, H + 1, 3, 128, 128, device=DEV), torch.zeros(4, H, 4, device=DEV))
    with pytest.raises(_capi.NdpError):
        a.grads_rollout(fl_d[:, 0:H], act_d[:, 0:H])                 # one frame short
    with pytest.raises(ValueError):
        _trainer(93, n, rollout_steps=0)


def _run_train(tmp_path, tag, **forward):
    from ndivplanning_amd import train_forward_model as script
    from ndivplanning_amd.utils.file import AttrDict
    f = {"num_epochs": 1, "learning_rate": LR, "report_feq": 10, "batch_size": 2, "epochs_per_stage": 1, "step_lr_gamma": 0.1}
    f.update(forward)
    cfg = AttrDict({"random_seed": 0, "train_data_path": "synthetic:4:images", "gpu_id": 0, "trajectory_length": 4,
                    "forward_save_path": str(tmp_path / tag), "training": {"forward": f}})
    initial = {}
    real_trainer = script.ForwardModelTrainer

    def spy(model, **kw):
        initial.update({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
        return real_trainer(model, **kw)
    script.ForwardModelTrainer = spy
    try:
        hist = script.train(cfg)
    finally:
        script.ForwardModelTrainer = real_trainer
    return cfg, hist, script.train.last_trainer, initial


def test_train_with_rollout_steps_is_a_replay_of_step_rollout_and_one_step_is_the_key_being_absent(tmp_path):
    from ndivplanning_amd.forward_trainer import ForwardModelTrainer
    from ndivplanning_amd.models import forward_encoder as FE
    from ndivplanning_amd.train_gan import make_dataset
    H = 2
    cfg, hist, last, initial = _run_train(tmp_path, "h2", rollout_steps=H)
    assert len(hist) == 1 and last.rollout_steps == H and last.steps == 2 * (4 - H)     # 2 batches x 2 windows
    model = FE.ForwardAutoencoder()
    model.load_state_dict(initial)
    replay = ForwardModelTrainer(model.to(DEV).train(), batch=2, lr=LR, betas=(0.5, 0.999), rollout_steps=H)
    torch.manual_seed(cfg.random_seed)
    np.random.seed(cfg.random_seed)
    FE.ForwardAutoencoder()                                          # consumes the CPU stream as the run's construction did
    ds = make_dataset(cfg)
    windows = 0
    for images, _, actions, _ in torch.utils.data.DataLoader(ds, batch_size=2, shuffle=True):
        images, actions = images.to(DEV).float(), actions.to(DEV).float()
        for i in range(ds.seq_length - H):
            replay.step_rollout(images[:, i:i + H + 1], actions[:, i:i + H])
            windows += 1
    assert windows == 4 and hist[0] == float(replay.loss_sum.item()) / windows
    assert torch.equal(replay.params, last.params) and torch.equal(replay.stats, last.stats)
    # rollout_steps: 1 is the key being absent
    _, hist_1, last_1, _ = _run_train(tmp_path, "h1", rollout_steps=1)
    _, hist_0, last_0, _ = _run_train(tmp_path, "h0")
    assert hist_1 == hist_0 and last_1.steps == last_0.steps == 2 * 3
    assert torch.equal(last_1.params, last_0.params) and torch.equal(last_1.stats, last_0.stats)
    assert hist_1 != hist
