#!/usr/bin/env python3
"""Time ndp_image_quality on an MI355X: 64 and 224 pairs of byte frames against float images,
SSIM and PSNR of each, against the same definition written in torch ops on the same device -- the byte frames normalised
and permuted, both operands scaled and clamped, five grouped conv2d pairs (11 x 1 then 1 x 11, the same fp32 taps) over
x, y, x*x, y*y, x*y, the elementwise S expression, means -- alternating the two in one process after a warm-up of both;
the median of the repeats, by device events.  A timed run of the kernel includes its workspace allocation (the caching
allocator) and both launches.  Needs a GPU; prints one JSON line.

    python scripts/bench_image_quality.py [--pairs 64 224] [--repeats 7]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def taps():
    i = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-i * i / (2 * 1.5 ** 2))
    return torch.from_numpy((g / g.sum()).astype(np.float32))


def torch_quality(a_u8, b_f32, g):
    """The definition in torch ops: (ssim [n], psnr [n]) of byte frames [n,128,128,3] against floats [n,3,128,128]."""
    unit = lambda x: ((x + 1.0) * 0.5).clamp(0.0, 1.0)           # noqa: E731
    x = unit(((a_u8.float() / 255.0 - 0.5) * 2.0).permute(0, 3, 1, 2))
    y = unit(b_f32)
    mse = ((x - y).double() ** 2).mean(dim=(1, 2, 3))
    psnr = (10.0 * torch.log10(1.0 / mse)).float()
    wh, wv = g.view(1, 1, 1, 11).repeat(3, 1, 1, 1), g.view(1, 1, 11, 1).repeat(3, 1, 1, 1)
    f = lambda m: torch.nn.functional.conv2d(torch.nn.functional.conv2d(m, wh, groups=3), wv, groups=3)   # noqa: E731
    ux, uy, uxx, uyy, uxy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return s.double().mean(dim=(1, 2, 3)).float(), psnr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[64, 224])
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_quality needs a GPU: a CPU run gives no time")
    from ndivplanning_amd.image_quality import image_quality
    from ndivplanning_amd.utils.trajectory_loader import synthetic_scene
    dev = torch.device("cuda:0")
    g = taps().to(dev)
    gen = torch.Generator().manual_seed(7)
    scenes = torch.from_numpy(np.stack([synthetic_scene(gen) for _ in range(8)]))
    out = {"bench": "image_quality", "repeats": args.repeats}
    for n in args.pairs:
        a = scenes[torch.arange(n) % 8].contiguous().to(dev)                                   # byte frames
        noise = torch.randn(n, 3, 128, 128, generator=gen) * 0.1
        b = (((a.cpu().float() / 255.0 - 0.5) * 2.0).permute(0, 3, 1, 2) + noise).contiguous().to(dev)   # float predictions
        runs = {"kernel": lambda: image_quality(a, b), "torch": lambda: torch_quality(a, b, g)}

        def timed(fn):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            res = fn()
            end.record()
            end.synchronize()
            return start.elapsed_time(end), res
        results = {}
        for name, fn in runs.items():                               # warm-up of both
            for _ in range(3):
                _, results[name] = timed(fn)
        times = {name: [] for name in runs}
        for _ in range(args.repeats):                               # alternating
            for name, fn in runs.items():
                times[name].append(timed(fn)[0])
        key = "pairs_%d" % n
        out[key] = {name + "_ms_median": statistics.median(t) for name, t in times.items()}
        out[key].update({name + "_ms_min_max": [min(t), max(t)] for name, t in times.items()})
        out[key]["torch_over_kernel"] = out[key]["torch_ms_median"] / out[key]["kernel_ms_median"]
        out[key]["ssim_max_abs_diff"] = float((results["kernel"][0] - results["torch"][0]).abs().max())
        out[key]["psnr_max_abs_diff"] = float((results["kernel"][1] - results["torch"][1]).abs().max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
