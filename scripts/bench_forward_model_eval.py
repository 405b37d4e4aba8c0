#!/usr/bin/env python3
"""Time forward_model_eval.evaluate on an MI355X: synthetic:<N>:frames_u8 trajectories, every
start frame rolled out for `horizon` steps, against the same evaluation with the scoring stage written in torch ops (the
composition that was possible before ndp_fm_score: gathered targets and start frames, normalisation, two MSEs, denorm /
clamp / permute to bytes), alternating the two in one process after a warm-up of both.  Then, in a pass of its own with
the library's per-kernel event timers on, k_fm_score's time and achieved bytes/s against the bytes it must move (per
prediction: 196,608 read for the prediction, 49,152 each for a byte target and a byte start frame, 49,152 written as
bytes).  Needs a GPU; prints one JSON line.

    python scripts/bench_forward_model_eval.py [--trajectories 64] [--seq-length 8] [--horizon 7] [--batch-size 16] [--repeats 7]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class InMemory(torch.utils.data.Dataset):
    """The dataset's items generated once: the timed window holds no host-side frame synthesis."""

    def __init__(self, dataset):
        self.items, self.seq_length, self.mode = [dataset[i] for i in range(len(dataset))], dataset.seq_length, dataset.mode

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def torch_score(pred, target=None, target_idx=None, base=None, base_idx=None, errors=True, out_bytes=False):
    """forward_model_eval.score in torch ops."""
    def images(frames, idx):
        rows = frames if idx is None else frames.index_select(0, idx.long())
        if rows.dtype == torch.uint8:
            rows = ((rows.float() / 255.0 - 0.5) * 2.0).permute(0, 3, 1, 2)
        return rows
    tgt = images(target, target_idx) if target is not None else None
    err = ((pred - tgt) ** 2).mean(dim=(1, 2, 3)) if tgt is not None and errors else None
    base_err = ((images(base, base_idx) - tgt) ** 2).mean(dim=(1, 2, 3)) if base is not None else None
    by = (((pred + 1.0) / 2.0) * 255.0).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous() if out_bytes else None
    return err, base_err, by


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trajectories", type=int, default=64)
    ap.add_argument("--seq-length", type=int, default=8)
    ap.add_argument("--horizon", type=int, default=7)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_forward_model_eval needs a GPU: a CPU run gives no time")
    from ndivplanning_amd import _capi, forward_model_eval as FME
    from ndivplanning_amd.models.forward_encoder import ForwardAutoencoder
    from ndivplanning_amd.utils.trajectory_loader import SyntheticPushDataset
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = ForwardAutoencoder()
    model.decoder.weight_init(mean=0.0, std=0.02)
    model.encoder.weight_init(mean=0.0, std=0.02)
    model = model.to(dev).eval()
    ds = InMemory(SyntheticPushDataset(args.trajectories, seq_length=args.seq_length, mode="frames_u8", seed=2))
    keep = args.trajectories * (args.seq_length - args.horizon)      # bytes of every prediction, as the torch composition's
    fused_score = FME.score

    def run(score, keep_):
        FME.score = score
        try:
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            res = FME.evaluate(model, ds, horizon=args.horizon, batch_size=args.batch_size, keep=keep_)
            end.record()
            end.synchronize()
            return start.elapsed_time(end), res
        finally:
            FME.score = fused_score

    variants = {"fused_bytes": (fused_score, keep), "torch_bytes": (torch_score, keep), "fused_errors_only": (fused_score, 0),
                "torch_errors_only": (torch_score, 0)}
    results = {}
    for name, (score, k) in variants.items():                       # warm-up of every variant's shapes
        for _ in range(2):
            _, results[name] = run(score, k)
    times = {name: [] for name in variants}
    for _ in range(args.repeats):                                    # alternating
        for name, (score, k) in variants.items():
            times[name].append(run(score, k)[0])
    diff = float((results["fused_bytes"]["horizon_mse"] - results["torch_bytes"]["horizon_mse"]).abs().max())
    same_bytes = float((results["fused_bytes"]["strips"]["predictions"] == results["torch_bytes"]["strips"]["predictions"])
                       .float().mean())
    # k_fm_score alone: the library's event timers, in a pass of their own
    predictions = int(results["fused_bytes"]["counts"].sum())
    _capi.timing_enable(True)
    run(fused_score, keep)
    torch.cuda.synchronize()
    timed = _capi.timing_collect()
    _capi.timing_enable(False)
    ms, launches = timed.get("k_fm_score", (0.0, 0))
    moved = predictions * (196608 + 49152 + 49152 + 49152)
    out = {"bench": "forward_model_eval", "trajectories": args.trajectories, "seq_length": args.seq_length,
           "horizon": args.horizon, "batch_size": args.batch_size, "predictions": predictions,
           "horizon_mse_max_abs_diff_fused_vs_torch": diff, "bytes_equal_share": same_bytes,
           "k_fm_score_ms_total": ms, "k_fm_score_launches": launches,
           "k_fm_score_us_per_launch": 1e3 * ms / max(launches, 1),
           "k_fm_score_GBps": moved / (ms * 1e-3) / 1e9 if ms > 0 else None, "bytes_moved": moved}
    for name, t in times.items():
        out[name + "_ms_median"] = statistics.median(t)
        out[name + "_ms_min_max"] = [min(t), max(t)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
