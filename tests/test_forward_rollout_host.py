"""Multi-step rollout training of the forward model, the parts that need no GPU: the definition
restated on the oracle (tests/rollout_common.py) against the oracle's own one-pair trainer, the gradient recursion the
device implements against end-to-end autograd in fp64, and the configuration errors of train()."""
import pytest
import torch

import rollout_common as C
from oracle import forward_model_oracle as FO


def _window(seed, n, H, dtype=torch.float32):
    gen = torch.Generator().manual_seed(seed)
    frames = torch.rand(n, H + 1, 3, 128, 128, generator=gen) * 2.0 - 1.0
    actions = torch.rand(n, H, 4, generator=gen) * 2.0 - 1.0
    return frames.to(dtype), actions.to(dtype)


def test_one_step_is_the_oracle_trainers_loss_and_gradients_to_the_bit():
    torch.set_num_threads(8)
    frames, actions = _window(3, 2, 1)
    mine = C.rollout_grads(FO.init_forward_model_state(7), frames, actions)
    want = FO.ForwardModelTrainer(FO.init_forward_model_state(7)).step(frames[:, 0].contiguous(), frames[:, 1].contiguous(),
                                                                      actions[:, 0].contiguous())
    assert torch.equal(mine["loss"], want["loss"]) and torch.equal(mine["losses"][0], want["loss"])
    assert list(mine["grads"]) == list(want["grads"])
    for name, ref in want["grads"].items():
        if ref is None:
            assert mine["grads"][name] is None, name
        else:
            assert torch.equal(mine["grads"][name], ref), name


def test_the_device_recursion_is_end_to_end_autograd_reassociated():
    """fp64, n = 2, H = 3: G_H = local_H; G_k = (local_k + G_{k+1}) + dcur_k; grad = ((grad_0 + grad_1) + grad_2), one
    autograd call per pass, against one autograd call through the whole window.  Only the order of additions differs."""
    torch.set_num_threads(8)
    frames, actions = _window(4, 2, 3, torch.float64)

    def state64():
        return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in FO.init_forward_model_state(8).items()}
    whole = C.rollout_grads(state64(), frames, actions)
    parts = C.recursion_grads(state64(), frames, actions)
    assert len(whole["losses"]) == 3 and float(whole["loss"]) > 0
    checked = 0
    for name, ref in whole["grads"].items():
        if ref is None:
            assert parts[name] is None, name
            continue
        if name in C.NOISE_BIASES:                                  # zero but for rounding, in both
            wscale = float(whole["grads"][name[:-4] + "weight"].abs().max())
            assert float(ref.abs().max()) <= 1e-12 * wscale and float(parts[name].abs().max()) <= 1e-12 * wscale, name
            continue
        scale = float(ref.norm())
        assert scale > 0, name
        assert float((parts[name] - ref).norm()) <= 1e-12 * scale, (name, float((parts[name] - ref).norm()) / scale)
        checked += 1
    assert checked == 38
    # the middle pass has both an upstream and a downstream gradient: later steps do reach the early passes' parameters
    single = C.rollout_grads(state64(), frames[:, :2], actions[:, :1])
    name = "encoder.conv1.weight"
    assert float((whole["grads"][name] * 3 - single["grads"][name]).norm()) > 1e-3 * float(single["grads"][name].norm())


def _config(tmp_path, **forward):
    from ndivplanning_amd.utils.file import AttrDict
    f = {"num_epochs": 1, "learning_rate": 2e-4, "report_feq": 10, "batch_size": 2, "epochs_per_stage": 1, "step_lr_gamma": 0.1}
    f.update(forward)
    return AttrDict({"random_seed": 0, "train_data_path": "synthetic:4:images", "gpu_id": 0, "trajectory_length": 4,
                     "forward_save_path": str(tmp_path / "fm"), "training": {"forward": f}})


def test_train_refuses_bad_rollout_settings_before_it_needs_a_gpu(tmp_path, monkeypatch):
    from ndivplanning_amd import train_forward_model as script

    def no_gpu(*a, **kw):
        raise AssertionError("train() touched the GPU before it checked rollout_steps")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu)
    monkeypatch.setattr(torch.cuda, "set_device", no_gpu)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="rollout_steps"):
            script.train(_config(tmp_path, rollout_steps=bad))
    with pytest.raises(ValueError, match="trajectory_length"):
        script.train(_config(tmp_path, rollout_steps=4))               # windows of 5 frames from trajectories of 4
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(ValueError, match="ranks"):
        script.train(_config(tmp_path, rollout_steps=2, batch_size=2))
