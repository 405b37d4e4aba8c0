#!/usr/bin/env python3
"""Device Lanczos resize (ndp_resize_lanczos_u8) against the path a user of the reference has today, on 500x500 camera
frames (MuJoCo's render size), and one closed-loop control step (evaluation.MpcController.act) split into its phases.

  * n = 1 / 8 / 64 frames.  Device arm: upload of the raw frames from pinned memory plus the kernel (bytes and floats).
    Host arm: PIL's Image.LANCZOS resize (one process at n = 1, 16 processes at n = 8 / 64, wall clock) plus the upload
    of the 128x128 bytes and ndp_eval_frames_u8.  The arms alternate; median of 20 after 5 warm-ups; the device side of
    both from device events.
  * the kernel alone for every rows_per_band at n = 1 and n = 64, with and without the float output: what the
    automatic choice was picked from.
  * one MpcController.act at R = 5, Th = 5 on a 500x500 frame: resize (upload + kernel) and plan, from device events.
Prints one JSON line."""
import argparse
import json
import multiprocessing as mp
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, RUNS = 5, 20
H = W = 500


def _pil_resize(chunk):
    from PIL import Image
    return [np.array(Image.fromarray(f).resize((128, 128), Image.LANCZOS)) for f in chunk]


def _events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def device_arm(resizer, pinned, dev):
    a, b = _events()
    a.record()
    out, img = resizer(pinned.to(dev, non_blocking=True))
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def host_arm(pool, frames, procs, models, dev, staging):
    t0 = time.perf_counter()
    if pool is None:
        small = _pil_resize(frames)
    else:
        small = [f for part in pool.map(_pil_resize, [frames[i::procs] for i in range(procs)]) for f in part]
    staging.copy_(torch.from_numpy(np.stack(small)))
    pil = (time.perf_counter() - t0) * 1e3
    a, b = _events()
    a.record()
    models_images = models(staging.to(dev, non_blocking=True))
    b.record()
    b.synchronize()
    return pil, a.elapsed_time(b), models_images


def kernel_ms(resizer, frames_dev, rb, floats):
    times = []
    for i in range(WARMUP + RUNS):
        a, b = _events()
        a.record()
        resizer(frames_dev, floats=floats, rows_per_band=rb)
        b.record()
        b.synchronize()
        if i >= WARMUP:
            times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--procs", type=int, default=16)
    args = ap.parse_args()
    from ndivplanning_amd import _capi
    from ndivplanning_amd import evaluation as E
    from ndivplanning_amd.resize import LanczosResizer
    from bench_mpc import modules
    dev = torch.device("cuda", 0)
    resizer = LanczosResizer(dev)
    lib = _capi.load()

    def frames_u8(x):
        out = torch.empty(int(x.shape[0]), 3, 128, 128, dtype=torch.float32, device=dev)
        _capi.check(lib.ndp_eval_frames_u8(_capi.ptr(x), int(x.shape[0]), _capi.ptr(out), _capi.stream_ptr(dev)), "frames_u8")
        return out
    rng = np.random.RandomState(0)
    out = {"frame": [H, W], "device_ms": {}, "host_pil_ms": {}, "host_upload_ms": {}, "kernel_ms": {}}
    ctx = mp.get_context("spawn")
    with ctx.Pool(args.procs) as pool:
        for n in (1, 8, 64):
            frames = rng.randint(0, 256, (n, H, W, 3)).astype(np.uint8)
            pinned = torch.from_numpy(frames).pin_memory()
            staging = torch.empty(n, 128, 128, 3, dtype=torch.uint8).pin_memory()
            dev_t, pil_t, up_t = [], [], []
            for i in range(WARMUP + RUNS):                                      # the arms alternate
                d = device_arm(resizer, pinned, dev)
                p, u, _ = host_arm(None if n == 1 else pool, list(frames), args.procs, frames_u8, dev, staging)
                if i >= WARMUP:
                    dev_t.append(d)
                    pil_t.append(p)
                    up_t.append(u)
            out["device_ms"][n] = round(statistics.median(dev_t), 4)
            out["host_pil_ms"][n] = round(statistics.median(pil_t), 3)
            out["host_upload_ms"][n] = round(statistics.median(up_t), 4)
            got, _ = resizer(pinned.to(dev))
            assert torch.equal(got.cpu(), staging), "device bytes differ from PIL's"
            if n in (1, 64):
                fd = pinned.to(dev)
                out["kernel_ms"][n] = {("rb%d%s" % (rb, "" if fl else "_bytes_only")): round(kernel_ms(resizer, fd, rb, fl), 4)
                                       for rb in (0, 1, 2, 4, 8, 16) for fl in (True, False)}
    enc, fm, gen = modules()
    models = E.EvalModels(enc, fm, gen, dev)
    ctrl = E.MpcController(models, 5, 5, (H, W))
    ctrl.reset(torch.from_numpy(rng.randint(0, 256, (1, 128, 128, 3)).astype(np.uint8)))
    frame = rng.randint(0, 256, (1, H, W, 3)).astype(np.uint8)
    rs, pl, wall = [], [], []
    for i in range(WARMUP + RUNS):
        a, b = _events()
        c = torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        state_u8, state = ctrl.observe(frame)
        b.record()
        ctrl.plan(state)
        c.record()
        c.synchronize()
        if i >= WARMUP:
            wall.append((time.perf_counter() - t0) * 1e3)
            rs.append(a.elapsed_time(b))
            pl.append(b.elapsed_time(c))
    out["act_ms"] = {"resize": round(statistics.median(rs), 4), "plan": round(statistics.median(pl), 4),
                     "wall": round(statistics.median(wall), 4), "rollouts": 5, "horizon": 5}
    print(json.dumps(out))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
