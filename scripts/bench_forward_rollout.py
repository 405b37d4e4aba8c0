#!/usr/bin/env python3
"""Time multi-step rollout training of the forward model on an MI355X: ms per
`ForwardModelTrainer.step_rollout` at batch 8 and 32 with H = 1, 2, 3, next to H x today's `step()` on the same trainer
(medians after a warm-up, the two alternating in one process), and the share of a rollout step taken by the launches that
are new with it -- the link kernels (begin, advance + its final pass, chain), the gradient sum and the repack of the
second weight order in the extra workspaces -- timed on their own in the same process.  Every timed `step_rollout`
follows an Adam step, as in training, and so includes its H - 1 repacks.  (The one further new launch,
conv1's data gradient inside ndp_fm_backward_inputs, runs beside the last weight gradient and is part of the remainder.)

With --learn: on `synthetic:64:frames_u8`, `forward_model_eval.evaluate`'s horizon_mse at horizons 1..3 on held-out
trajectories after the same number of optimiser steps with H = 1 and with H = 3, from the same initial weights.

Needs a GPU; prints one JSON line.

    python scripts/bench_forward_rollout.py [--repeats 15] [--learn] [--learn-steps 300] [--learn-batch 8]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def new_model(dev, seed=0):
    from ndivplanning_amd.models.forward_encoder import ForwardAutoencoder
    torch.manual_seed(seed)
    model = ForwardAutoencoder()
    model.decoder.weight_init(mean=0.0, std=0.02)
    model.encoder.weight_init(mean=0.0, std=0.02)
    return model.to(dev).train()


def links_only(tr, frames, actions):
    """The launches of grads_rollout + apply that are new with H > 1, on the trainer's own buffers, without the passes."""
    from ndivplanning_amd import _capi
    H, n = tr.rollout_steps, int(frames.shape[0])
    p, lib, st = _capi.ptr, tr.lib, _capi.stream_ptr(tr.device)
    stride, image = int(frames.stride(0)), 3 * 128 * 128 * frames.element_size()
    u8 = int(frames.dtype == torch.uint8)
    frame = lambda k: _capi.c_void_p(frames.data_ptr() + k * image)      # noqa: E731
    lib.ndp_fm_rollout_begin(frame(0), u8, stride, n, p(tr._states[0]), st)
    for k in range(H):
        lib.ndp_fm_rollout_advance(p(tr._states[k]), p(tr._resid), frame(k + 1), u8, stride, n, k, H, p(tr._states[k + 1]),
                                   p(tr._locals[k]), p(tr.rollout_losses), p(tr.loss), None, p(tr._workspaces[k]), st)
    for k in range(H - 1, 0, -1):
        lib.ndp_fm_rollout_chain(p(tr._locals[k - 1]), p(tr._locals[k]), p(tr._dcur), n, p(tr._locals[k - 1]), st)
    lib.ndp_fm_grad_sum(p(tr._step_grads), tr._grad_stride, H, tr.params.numel(), p(tr.grad), st)
    tr._pack_extra_workspaces()
    tr._extra_stale = True                 # as after apply(): the step_rollout timed next repacks, as every training step does


def time_steps(dev, batch, H, repeats):
    from ndivplanning_amd.forward_trainer import ForwardModelTrainer
    tr = ForwardModelTrainer(new_model(dev), batch=batch, rollout_steps=H)
    gen = torch.Generator().manual_seed(batch * 10 + H)
    frames = torch.randint(0, 256, (batch, H + 1, 128, 128, 3), generator=gen, dtype=torch.uint8).to(dev)
    actions = (torch.rand(batch, H, 4, generator=gen) * 2.0 - 1.0).to(dev)
    pairs = [(frames[:, k].contiguous(), frames[:, k + 1].contiguous(), actions[:, k].contiguous()) for k in range(H)]

    def rollout():
        tr.step_rollout(frames, actions)

    def singles():
        for cur, fut, act in pairs:
            tr.step(cur, fut, act)

    def links():
        links_only(tr, frames, actions)
    variants = {"step_rollout": rollout, "H_x_step": singles}
    if H > 1:
        variants["new_launches"] = links
    for _ in range(3):                                               # warm-up of every variant
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(repeats):                                         # alternating
        for name, fn in variants.items():
            times[name].append(timed(fn))
    out = {"batch": batch, "H": H}
    for name, t in times.items():
        out[name + "_ms_median"] = statistics.median(t)
        out[name + "_ms_min_max"] = [min(t), max(t)]
    if H > 1:
        out["new_launches_share"] = out["new_launches_ms_median"] / out["step_rollout_ms_median"]
        out["grad_sum_bytes"] = (H + 1) * 4 * tr.params.numel()
    out["rollout_over_H_x_step"] = out["step_rollout_ms_median"] / out["H_x_step_ms_median"]
    return out


def learn(dev, steps, batch):
    from ndivplanning_amd import forward_model_eval as FME
    from ndivplanning_amd.forward_trainer import ForwardModelTrainer
    from ndivplanning_amd.utils.trajectory_loader import SyntheticPushDataset
    seq = 8
    train_set = SyntheticPushDataset(64, seq_length=seq, mode="frames_u8", seed=0)
    val_set = SyntheticPushDataset(16, seq_length=seq, mode="frames_u8", seed=1)
    items = [train_set[i] for i in range(len(train_set))]
    out = {"steps": steps, "batch": batch, "train": "synthetic:64:frames_u8", "val_trajectories": len(val_set), "seq_length": seq}
    for H in (1, 3):
        tr = ForwardModelTrainer(new_model(dev, seed=0), batch=batch, rollout_steps=H)
        order = torch.Generator().manual_seed(5)
        done = 0
        while done < steps:
            perm = torch.randperm(len(items), generator=order).tolist()
            for b in range(0, len(perm) - batch + 1, batch):
                frames = torch.stack([items[i][0] for i in perm[b:b + batch]]).to(dev)
                actions = torch.stack([items[i][2] for i in perm[b:b + batch]]).to(dev).float()
                for i in range(seq - H):
                    if done < steps:
                        tr.step_rollout(frames[:, i:i + H + 1], actions[:, i:i + H])
                        done += 1
        model = tr.sync_to_module().eval()
        res = FME.evaluate(model, val_set, horizon=3, batch_size=batch, device=dev)
        out["H%d_horizon_mse" % H] = res["horizon_mse"].tolist()
        out["H%d_final_train_loss" % H] = float(tr.loss.item())
        out["persistence_mse"] = res["persistence_mse"].tolist()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--learn", action="store_true")
    ap.add_argument("--learn-steps", type=int, default=300)
    ap.add_argument("--learn-batch", type=int, default=8)
    ap.add_argument("--skip-timing", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_forward_rollout needs a GPU: a CPU run gives no time")
    dev = torch.device("cuda:0")
    out = {"bench": "forward_rollout", "repeats": args.repeats}
    if not args.skip_timing:
        out["timing"] = [time_steps(dev, batch, H, args.repeats) for batch in (8, 32) for H in (1, 2, 3)]
    if args.learn:
        out["learn"] = learn(dev, args.learn_steps, args.learn_batch)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
