#!/usr/bin/env python3
"""The device-resident trajectory store (ndp_store_gather, ndivplanning_amd/trajectory_store.py) against the host route,
per batch, at (B, T) = (16, 8), (128, 8) and (1,024, 15), on a `bundle synth` directory made here (64 distinct seeded
trajectories of 15 frames, repeated to 2,048 so that the largest batch has two batches to an epoch):

  (a) StoreLoader, gather only;
  (b) StoreLoader, then JpegDecoder.decode_frames;
  (c) the host route: DataLoader(num_workers=0, shuffle=True, collate_fn=collate_jpeg) over the same streams held in
      memory as bytes objects, then the upload of the packed buffer, the offsets and the float tensors -- without and
      with the decode.

Each figure is wall-clock milliseconds per batch over whole epochs that end in a device synchronise (at least 20 batches
and half a second, after one warm-up epoch), the median of 3 such windows, the routes alternating.  The gather's two
kernels are also timed by the library's events (50 gathers of one fixed batch), and their bytes/s is the bytes the gather
moves -- streams read and written, offsets written, float rows read and written, indices read -- over that time.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((16, 8), (128, 8), (1024, 15))
DISTINCT, TOTAL, STEPS = 64, 2048, 15


def make_directory(root, seed=0):
    """DISTINCT seeded trajectories (`bundle synth`), repeated to TOTAL in 4 bundle files."""
    from ndivplanning_amd import bundle
    seed_dir, data = os.path.join(root, "seed"), os.path.join(root, "data")
    bundle.synth(DISTINCT, seed_dir, steps=STEPS, seed=seed)
    ds = bundle.BundleDataset(seed_dir, seq_length=STEPS, raw_jpeg=True)
    items = [ds[i] for i in range(DISTINCT)]
    os.makedirs(data)
    per_file = TOTAL // 4
    for f in range(4):
        bundle.write_bundle(os.path.join(data, "trajectory_bundle_%05d.ndpt" % (f + 1)),
                            (items[(f * per_file + i) % DISTINCT] for i in range(per_file)))
    return data


class InMemory(torch.utils.data.Dataset):
    """The bundle directory's trajectories as `BundleDataset(raw_jpeg=True)` yields them, read once and kept."""
    mode = "jpeg"

    def __init__(self, data, steps):
        from ndivplanning_amd.bundle import BundleDataset
        ds = BundleDataset(data, seq_length=steps, raw_jpeg=True)
        self.items = [ds[i] for i in range(len(ds))]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, index):
        return self.items[index]


def ms_per_batch(epoch, min_batches=20, min_seconds=0.5):
    """epoch(): one pass over a loader, returns its batch count; the device is synchronised at the window's end."""
    batches, t0 = 0, time.perf_counter()
    while batches < min_batches or time.perf_counter() - t0 < min_seconds:
        batches += epoch()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / batches


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--windows", type=int, default=3)
    args = ap.parse_args()
    from torch.utils.data import DataLoader
    from ndivplanning_amd import _capi
    from ndivplanning_amd.jpeg import JpegDecoder, collate_jpeg
    from ndivplanning_amd.trajectory_store import DeviceTrajectoryStore, StoreLoader
    dev = torch.device("cuda", 0)
    out = {"trajectories": TOTAL, "shapes": {}}
    with tempfile.TemporaryDirectory() as root:
        data = make_directory(root)
        store = DeviceTrajectoryStore(data, dev)
        out["store_bytes"], out["max_stream_bytes"] = store.nbytes, store.max_stream_bytes
        dec = JpegDecoder(dev, check=False)
        for batch, steps in SHAPES:
            host_loader = DataLoader(InMemory(data, steps), batch_size=batch, shuffle=True, num_workers=0, collate_fn=collate_jpeg)
            store_loader = StoreLoader(store, batch, 0, steps, shuffle=True)

            def store_epoch(decode):
                n = 0
                for frames, states, actions, goal in store_loader:
                    if decode:
                        dec.decode_frames(frames)
                    n += 1
                return n

            def host_epoch(decode):
                n = 0
                for frames, states, actions, goal in host_loader:
                    frames.buffer, frames.offsets = frames.buffer.to(dev, non_blocking=True), frames.offsets.to(dev, non_blocking=True)
                    states, actions, goal = states.to(dev), actions.to(dev), goal.to(dev)
                    if decode:
                        dec.decode_frames(frames)
                    n += 1
                return n

            routes = {"store_gather": lambda: store_epoch(False), "store_gather_decode": lambda: store_epoch(True),
                      "host_upload": lambda: host_epoch(False), "host_upload_decode": lambda: host_epoch(True)}
            for fn in routes.values():                                 # warm-up: every shape once
                fn()
            torch.cuda.synchronize()
            samples = {k: [] for k in routes}
            for _ in range(args.windows):
                for k, fn in routes.items():
                    samples[k].append(ms_per_batch(fn))
            row = {k + "_ms": round(statistics.median(v), 4) for k, v in samples.items()}
            row.update({k + "_spread_ms": round(max(v) - min(v), 4) for k, v in samples.items()})
            row["host_over_store"] = round(row["host_upload_ms"] / row["store_gather_ms"], 2)
            row["host_over_store_with_decode"] = round(row["host_upload_decode_ms"] / row["store_gather_decode_ms"], 2)
            # the kernels alone, one fixed batch
            indices = torch.randperm(len(store), generator=torch.Generator().manual_seed(1))[:batch].to(dev)
            frames = store.gather(indices, 0, steps)[0]
            stream_bytes = int(frames.offsets[-1])
            n = batch * steps
            moved = 2 * stream_bytes + 8 * (n + 1) + 2 * 4 * (n * 29 + batch * 3) + 8 * batch
            _capi.timing_enable(True)
            for _ in range(50):
                store.gather(indices, 0, steps)
            torch.cuda.synchronize()
            split = _capi.timing_collect()
            _capi.timing_enable(False)
            kernels = {k: v[0] / v[1] for k, v in split.items() if k.startswith("k_store")}
            row["kernel_ms"] = {k: round(v, 5) for k, v in kernels.items()}
            row["stream_bytes"], row["bytes_moved"] = stream_bytes, moved
            row["gather_gb_per_s"] = round(moved / (sum(kernels.values()) * 1e-3) / 1e9, 2)
            out["shapes"]["%dx%d" % (batch, steps)] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
