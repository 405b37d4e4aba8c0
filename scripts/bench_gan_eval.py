#!/usr/bin/env python3
"""Time gan_eval.evaluate on an MI355X: synthetic:<N>:codes trajectories, K samples per
conditioning row, with a discriminator, at K = 6 and K = 32 -- and the scoring stage alone, through ndp_gan_score (one
launch) against the same stage written in torch ops on the device (broadcast differences and norms, sums, relu, min,
cummin, argmax, gather: the composition that was possible before the kernel), on one batch's tensors.  HIP events, after
a warm-up of both variants, the two alternating, median of `--repeats`.  Needs a GPU; prints one JSON line.

    python scripts/bench_gan_eval.py [--trajectories 64] [--seq-length 15] [--batch-size 16] [--repeats 7]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class InMemory(torch.utils.data.Dataset):
    """The dataset's items generated once: the timed window holds no host-side synthesis."""

    def __init__(self, dataset):
        self.items, self.seq_length, self.mode = [dataset[i] for i in range(len(dataset))], dataset.seq_length, dataset.mode

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def torch_score(action_hat, actions=None, noise=None, fake_logits=None, outputs=None):
    """gan_eval.score in torch ops (fp32 throughout; NaN rules as torch's min / max have them)."""
    n, k = action_hat.shape[:2]
    pairwise = lambda z: torch.linalg.vector_norm(z[:, :, None, :] - z[:, None, :, :], ord=2, dim=3)      # noqa: E731
    out = {}
    sq = (action_hat - actions[:, None, :]) ** 2
    out["sample_err"] = sq.mean(2)
    out["mean_err"] = sq.mean((1, 2))
    out["best_err"], best_k = out["sample_err"].min(1)
    out["best_k"] = best_k.int()
    out["best_curve"] = torch.cummin(out["sample_err"], dim=1).values
    dx = pairwise(action_hat)
    out["spread"] = dx.sum((1, 2)) / (k * (k - 1))
    dz = pairwise(noise)
    out["ndiv"] = torch.relu(dz / dz.sum(2, keepdim=True) * 0.8 - dx / dx.sum(2, keepdim=True)).sum((1, 2))
    if fake_logits is not None:
        logits = fake_logits.view(n, k)
        out["d_fake_prob"] = torch.sigmoid(logits).mean(1)
        pick = logits.argmax(1)
        out["d_pick_k"] = pick.int()
        out["d_pick_err"] = out["sample_err"].gather(1, pick[:, None])[:, 0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trajectories", type=int, default=64)
    ap.add_argument("--seq-length", type=int, default=15)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gan_eval needs a GPU: a CPU run gives no time")
    from ndivplanning_amd import gan_eval as GE
    from ndivplanning_amd.models.gan import Decoder, Discriminator
    from ndivplanning_amd.utils.trajectory_loader import SyntheticPushDataset
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    g, d = Decoder(noise_dim=2).to(dev).eval(), Discriminator().to(dev).eval()
    ds = InMemory(SyntheticPushDataset(args.trajectories, seq_length=args.seq_length, mode="codes", seed=2))
    fused_score = GE.score

    def timed(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        res = fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end), res

    def run_evaluate(score, k):
        GE.score = score
        try:
            return timed(lambda: GE.evaluate(g, ds, discriminator=d, num_sample=k, batch_size=args.batch_size, seed=1))
        finally:
            GE.score = fused_score

    out = {"bench": "gan_eval", "trajectories": args.trajectories, "seq_length": args.seq_length, "batch_size": args.batch_size,
           "rows": args.trajectories * (args.seq_length - 1), "repeats": args.repeats}
    variants = {"fused": fused_score, "torch": torch_score}
    for k in (6, 32):
        results = {}
        for name, score in variants.items():                         # warm-up of both variants' shapes
            for _ in range(2):
                results[name] = run_evaluate(score, k)[1]
        # one batch's tensors for the stage alone
        n = args.batch_size * (args.seq_length - 1)
        rows = results["fused"]["rows"]
        hat, noise = rows["action_hat"][:n].contiguous(), rows["noise"][:n].contiguous()
        acts = torch.stack([ds[i][2] for i in range(args.batch_size)]).to(dev)[:, :-1].reshape(-1, 4).contiguous()
        logits = torch.randn(n, k, generator=torch.Generator().manual_seed(3)).to(dev)
        for score in variants.values():
            for _ in range(3):
                score(hat, acts, noise, logits)
        torch.cuda.synchronize()
        times = {"evaluate_" + name: [] for name in variants}
        times.update({"stage_" + name: [] for name in variants})
        for _ in range(args.repeats):                                # alternating
            for name, score in variants.items():
                times["evaluate_" + name].append(run_evaluate(score, k)[0])
            for name, score in variants.items():
                times["stage_" + name].append(timed(lambda s=score: s(hat, acts, noise, logits))[0])
        f, t = results["fused"], results["torch"]
        entry = {"stage_rows": n,
                 "best_curve_max_abs_diff_fused_vs_torch": float((f["best_of_k_curve"] - t["best_of_k_curve"]).abs().max()),
                 "ndiv_per_row_abs_diff_fused_vs_torch": float((f["ndiv_per_row"] - t["ndiv_per_row"]).abs().max()),
                 "best_k_equal_share": float((f["rows"]["best_k"] == t["rows"]["best_k"]).float().mean())}
        for name, ts in times.items():
            entry[name + "_ms_median"] = statistics.median(ts)
            entry[name + "_ms_min_max"] = [min(ts), max(ts)]
        entry["stage_torch_over_fused"] = entry["stage_torch_ms_median"] / entry["stage_fused_ms_median"]
        entry["evaluate_torch_over_fused"] = entry["evaluate_torch_ms_median"] / entry["evaluate_fused_ms_median"]
        out["K%d" % k] = entry
    print(json.dumps(out))


if __name__ == "__main__":
    main()
