#!/usr/bin/env python3
"""Golden vector for the device JPEG encoder (ndp_jpeg_encode_u8).

The reference writes every camera frame with PIL, `im.save(..., format="jpeg", quality=95)` (generate_trajectories.py:
113-122); the encoder must write PIL's bytes exactly, so the oracle is PIL built on libjpeg-turbo (asserted below).

Stored (tests/golden/jpeg_encode_case.npz):
  names [n] str, kind [n] int32, ref [n] int64  what each frame is; kind 0: row `ref` of `frames`; 1 / 2 / 3: uniform
                                                noise / noise of only 0 and 255 / a flat frame whose last MCU is such
                                                noise, from np.random.RandomState(ref) (tests/jpeg_enc_core_host.py)
  frames [m,128,128,3] uint8                    the frames that are not made again from a seed
  streams [bytes] uint8, offsets [n+1] int64    PIL's streams, back to back
  header [623] uint8                            SOI .. SOS, common to every stream (asserted)
  digest [n,16] uint8                           blake2b of PIL's decode of PIL's stream (tests/jpeg_core_host.digest)
  total_bits, entropy_bytes, stuffed, last_ff, zrl, eob_only, max_dc_cat [n] int32
                                                census of each stream: entropy bits before padding, entropy bytes with
                                                stuffing, 0x00 bytes stuffed, final padded byte is 0xFF, ZRL symbols,
                                                blocks that are a DC symbol and EOB only, the largest DC category
  env_index [4] int64                           the corpus rows that are tests/fake_push_env.py frames
                                                (jpeg_enc_core_host.env_frames) resized by PIL (LANCZOS)

The census comes from the encoder's host driver (tests/host_drivers/jpeg_enc.inc, built without sanitizers here), and is
kept only because the driver's streams equal PIL's for every frame (asserted).  The two padding classes are found by a
seeded search over corner-noise frames.  check_classes (tests/jpeg_enc_core_host.py) asserts that every class is present.

Usage: python tests/golden/make_golden_jpeg_encode.py
"""
import io
import os
import sys
import tempfile

import numpy as np
import torch
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import jpeg_core_host as H  # noqa: E402
import jpeg_enc_core_host as E  # noqa: E402
from ndivplanning_amd.utils.trajectory_loader import synthetic_scene  # noqa: E402


def stored_frames():
    yy, xx = np.mgrid[0:128, 0:128]
    out = []

    def add(name, img):
        img = np.asarray(img)
        if img.ndim == 2:
            img = np.repeat(img[..., None], 3, axis=2)
        out.append((name, np.clip(img, 0, 255).astype(np.uint8)))

    add("flat_37", np.full((128, 128), 37))
    add("black", np.zeros((128, 128)))
    add("white", np.full((128, 128), 255))
    add("checker_8", ((yy // 8 + xx // 8) % 2) * 255)
    add("checker_16", ((yy // 16 + xx // 16) % 2) * 255)
    add("checker_8_colour", np.stack([((yy // 8 + xx // 8) % 2) * 255, ((yy // 8) % 2) * 255, ((xx // 8) % 2) * 255], axis=2))
    add("checker_16_colour", np.stack([((yy // 16 + xx // 16) % 2) * 255, ((xx // 16) % 2) * 255, ((yy // 16) % 2) * 255], axis=2))
    add("gradient_x", xx * 2)
    add("gradient_y", yy * 2)
    add("gradient_colour", np.stack([xx * 2, yy * 2, 255 - xx - yy], axis=2))
    add("gradient_steep", np.stack([(xx * 7) % 256, (yy * 5) % 256, ((xx + yy) * 3) % 256], axis=2))
    for k, (level, bright, step) in enumerate(((100, 255, 23), (20, 230, 37), (200, 0, 29), (128, 140, 31))):
        img = np.full((128, 128, 3), level)                    # isolated pixels on a flat field: long zero runs
        rng = np.random.RandomState(70 + k)
        for j in range(0, 128 * 128, step * 41):
            img[(j // 128) % 128, j % 128] = bright if k % 2 == 0 else rng.randint(0, 256, 3)
        add("pixels_%d" % k, img)
    one = np.full((128, 128, 3), 90)
    one[7, 7] = (255, 255, 255)
    one[64 + 7, 64 + 7] = (0, 0, 0)
    add("pixels_block_corner", one)
    for seed in (0, 1, 2, 3, 4, 5, 6):
        gen = torch.Generator().manual_seed(seed)
        add("synthetic_scene_%d" % seed, synthetic_scene(gen))
    env_index = []
    for j, frame in enumerate(E.env_frames()):
        env_index.append(len(out))
        add("fake_push_env_%d" % j, np.array(Image.fromarray(frame).resize((128, 128), Image.LANCZOS)))
    return out, env_index


def main():
    assert features.check_feature("libjpeg_turbo"), "the oracle is PIL on libjpeg-turbo"
    stored, env_index = stored_frames()
    names = [n for n, _ in stored]
    kind = [E.STORED] * len(stored)
    ref = list(range(len(stored)))
    for seed in (11, 12, 13, 14):
        names.append("uniform_noise_%d" % seed); kind.append(E.UNIFORM_NOISE); ref.append(seed)
    for seed in (21, 22, 23):
        names.append("binary_noise_%d" % seed); kind.append(E.BINARY_NOISE); ref.append(seed)
    with tempfile.TemporaryDirectory() as tmp:
        exe = E.build_driver(tmp, sanitize=False)
        # the two padding classes: a seeded search over corner-noise frames
        seeds = np.arange(1000, 1400)
        cand = np.stack([E.seeded_frame(E.CORNER_NOISE, s) for s in seeds])
        rec, streams = E.run_driver(exe, cand, np.zeros((0, 384, 64), np.int16), tmp)
        for j, s in enumerate(seeds):
            assert streams[j] == E.pil_encode(cand[j]), "corner noise %d: the driver's stream is not PIL's" % s
        last_ff = seeds[np.flatnonzero(rec["last_ff"] == 1)[:2]]
        no_pad = seeds[np.flatnonzero((rec["total_bits"] % 8 == 0) & (rec["last_ff"] == 0))[:2]]
        assert len(last_ff) == 2 and len(no_pad) == 2, (last_ff, no_pad)
        for s in last_ff:
            names.append("corner_noise_last_ff_%d" % s); kind.append(E.CORNER_NOISE); ref.append(int(s))
        for s in no_pad:
            names.append("corner_noise_no_padding_%d" % s); kind.append(E.CORNER_NOISE); ref.append(int(s))
        g = {"names": np.array(names), "kind": np.array(kind, np.int32), "ref": np.array(ref, np.int64),
             "frames": np.stack([f for _, f in stored])}
        frames = E.corpus_frames(g)
        pil = [E.pil_encode(f) for f in frames]
        rec, streams = E.run_driver(exe, frames, np.zeros((0, 384, 64), np.int16), tmp)
    for i, n in enumerate(names):
        assert streams[i] == pil[i], "%s: the driver's stream is not PIL's" % n
        assert rec["equal"][i] == 1, n
    g["streams"] = np.frombuffer(b"".join(pil), np.uint8)
    g["offsets"] = np.concatenate([[0], np.cumsum([len(s) for s in pil])]).astype(np.int64)
    g["header"] = np.frombuffer(pil[0][:E.HEADER], np.uint8)
    assert all(s[:E.HEADER] == pil[0][:E.HEADER] for s in pil), "the 623 header bytes are not common to every stream"
    assert pil[0][E.HEADER - 14:E.HEADER - 12] == b"\xff\xda", "SOS does not end the header"
    g["digest"] = np.stack([H.digest(np.array(Image.open(io.BytesIO(s)))) for s in pil])
    for k in E.CENSUS:
        g[k] = rec[k].astype(np.int32)
    g["env_index"] = np.array(env_index, np.int64)
    E.check_classes(g)
    path = os.path.join(HERE, "jpeg_encode_case.npz")
    np.savez_compressed(path, **g)
    size = os.path.getsize(path)
    assert size <= 1000000, size
    print("%s: %d frames, %d stream bytes, longest %d, file %d bytes" % (path, len(names), g["streams"].size,
                                                                         int(np.diff(g["offsets"]).max()), size))
    for i, n in enumerate(names):
        print("  %-34s %6d bytes  bits %% 8 = %d  stuffed %4d  last_ff %d  zrl %4d  eob_only %3d  dc_cat %2d"
              % (n, len(pil[i]), g["total_bits"][i] % 8, g["stuffed"][i], g["last_ff"][i], g["zrl"][i], g["eob_only"][i],
                 g["max_dc_cat"][i]))


if __name__ == "__main__":
    main()
