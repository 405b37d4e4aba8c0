#!/usr/bin/env python3
"""Device JPEG decode (ndp_jpeg_decode_u8) against PIL, on frames like the reference's (PIL, quality 95, 128x128).

  * decode time of 64 / 240 / 1,024 frames (one loader batch of the forward model, the autoencoder, GAN config 4) from
    device events: median of 20 runs after 5 warm-up runs;
  * PIL on 16 host processes on the same streams (median of 5 batches, wall clock);
  * a forward-model iteration at batch 8 (8 trajectories x 8 frames: one decode + 7 training steps) fed from JPEG,
    against the same iteration fed from decoded bytes, in one process;
  * the split between the four kernels (library timing events).

`--profile-only`: just 20 decodes of 1,024 frames, for `rocprofv3 --kernel-trace --stats -- python scripts/bench_jpeg.py
--profile-only` (the stage split without the event brackets).  Prints one JSON line."""
import argparse
import io
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


def make_streams(n, seed=0):
    from ndivplanning_amd.utils.trajectory_loader import encode_jpeg, synthetic_scene
    gen = torch.Generator().manual_seed(seed)
    return [encode_jpeg(synthetic_scene(gen)) for _ in range(n)]


def _pil_decode(chunk):
    from PIL import Image
    return [np.asarray(Image.open(io.BytesIO(s)).convert("RGB")).shape for s in chunk]


def pil_ms(pool, streams, procs, reps=5):
    chunks = [streams[i::procs] for i in range(procs)]
    times = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        pool.map(_pil_decode, chunks)
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times[1:])


def decode_ms(dec, buf, off, warmup=5, runs=20):
    for _ in range(warmup):
        dec.decode(buf, off, check=False)
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dec.decode(buf, off, check=False)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def fm_iteration_ms(dec, streams, dev, source, runs=10):
    """One forward-model loader batch at batch 8: 8 x 8 frames -> 7 training steps."""
    from ndivplanning_amd.forward_trainer import ForwardModelTrainer
    from ndivplanning_amd.jpeg import pack_jpegs
    from ndivplanning_amd.models.forward_encoder import ForwardAutoencoder
    torch.manual_seed(0)
    model = ForwardAutoencoder().to(dev).train()
    tr = ForwardModelTrainer(model, batch=8)
    buf, off = pack_jpegs(streams[:64])
    frames_host = dec.decode(buf, off, check=True).cpu().pin_memory()
    actions = torch.rand(8, 8, 4, device=dev) * 2 - 1
    times = []
    for it in range(runs + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if source == "jpeg":
            images = dec.decode(buf, off, check=False).view(8, 8, 128, 128, 3)
        else:
            images = frames_host.to(dev, non_blocking=True).view(8, 8, 128, 128, 3)
        for s in range(7):
            tr.step(images[:, s].contiguous(), images[:, s + 1].contiguous(), actions[:, s].contiguous())
        b.record()
        b.synchronize()
        if it >= 2:
            times.append(a.elapsed_time(b))
    tr.close()
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--procs", type=int, default=16)
    args = ap.parse_args()
    from ndivplanning_amd import _capi
    from ndivplanning_amd.jpeg import JpegDecoder, pack_jpegs
    dev = torch.device("cuda", 0)
    streams = make_streams(1024)
    dec = JpegDecoder(dev, check=False)
    buf, off = pack_jpegs(streams)
    buf, off = buf.to(dev), off.to(dev)
    if args.profile_only:
        for _ in range(20):
            dec.decode(buf, off)
        torch.cuda.synchronize()
        print(json.dumps({"profile_only": True, "frames": 1024}))
        return
    frames = dec.decode(buf, off, check=True)
    sizes = [len(s) for s in streams]
    out = {"stream_bytes_mean": float(np.mean(sizes)), "decode_ms": {}, "pil_ms": {}}
    ctx = mp.get_context("spawn")
    with ctx.Pool(args.procs) as pool:
        for n in (64, 240, 1024):
            b_, o_ = pack_jpegs(streams[:n])
            b_, o_ = b_.to(dev), o_.to(dev)
            out["decode_ms"][n] = round(decode_ms(dec, b_, o_), 4)
            out["pil_ms"][n] = round(pil_ms(pool, streams[:n], args.procs), 3)
    _capi.timing_enable(True)
    for _ in range(20):
        dec.decode(buf, off, check=False)
    torch.cuda.synchronize()
    split = _capi.timing_collect()
    _capi.timing_enable(False)
    out["stages_ms_1024"] = {k: round(v[0] / v[1], 4) for k, v in split.items() if k.startswith("k_jpeg")}
    out["fm_iteration_ms"] = {"jpeg": round(fm_iteration_ms(dec, streams, dev, "jpeg"), 3),
                              "bytes": round(fm_iteration_ms(dec, streams, dev, "bytes"), 3)}
    out["frames_ok"] = bool(frames.any())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
