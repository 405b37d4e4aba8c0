#!/usr/bin/env python3
"""Golden vector for the device JPEG decoder (ndp_jpeg_decode_u8).

The reference writes every camera frame with PIL, `format="jpeg", quality=95` (generate_trajectories.py:113-122), and its
loader decodes them with PIL (utils/hdf5_load.py:9-11).  The decoder must return PIL's bytes exactly, so the oracle is
PIL built on libjpeg-turbo (asserted below: IJG libjpeg upsamples chroma differently).

Stored (tests/golden/jpeg_case.npz):
  streams [bytes] uint8, offsets [n+1] int64   every stream, back to back
  names [n] str                                 what each stream is
  status [n] int32                              the expected NDP_JPEG_* status (include/ndp.h)
  frames_dx [n_ok,128,128,3] uint8              PIL's bytes of the decodable streams, in stream order, stored as
                                                differences along x (mod 256; frames = cumsum(frames_dx, axis=2) in
                                                uint8) -- they compress three times better than the bytes
  frame_of [n] int64                            the row of `frames` for a decodable stream, -1 otherwise

Decodable: eight 128x128 scenes (gradients, saturated discs and blocks, hard edges, stripes, texture) at quality 95 4:2:0
(the reference's setting), the same scenes at quality 75 and 50, and at quality 95 with optimize=True.  Rejected:
4:4:4, 4:2:2, progressive, grayscale, restart markers (unsupported); 64x64 and 100x75 (size); truncated streams and one
whose first segment length points past the end (corrupt).

Usage: python tests/golden/make_golden_jpeg.py
"""
import io
import os

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
OK, UNSUPPORTED, SIZE, CORRUPT = 0, 1, 2, 3


def scene(seed, size=(128, 128)):
    """A synthetic RGB frame with saturated colours and hard edges (the IDCT's range limit and the upsampler's edges)."""
    h, w = size
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    kind = seed % 5
    if kind == 0:
        img = np.stack([40 + 1.6 * xx, 220 - 1.5 * yy, 60 + 0.8 * (xx + yy)], axis=2)
    elif kind == 1:
        img = np.zeros((h, w, 3), np.float32) + rng.randint(0, 256, 3)
    elif kind == 2:                                     # stripes of saturated primaries
        band = (xx // 7 + yy // 11).astype(int) % 6
        pal = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]], np.float32)
        img = pal[band]
    elif kind == 3:                                     # checkerboard black / white
        img = (((xx // 4 + yy // 4) % 2) * 255)[..., None].repeat(3, axis=2)
    else:
        img = 128 + 100 * np.stack([np.sin(xx / 5.0), np.cos(yy / 3.0), np.sin((xx + yy) / 9.0)], axis=2)
    for _ in range(rng.randint(3, 8)):
        cy, cx, r = rng.randint(0, h), rng.randint(0, w), rng.randint(4, 30)
        img[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = rng.choice([0, 255], 3)
    y0, x0 = rng.randint(0, max(1, h - 20)), rng.randint(0, max(1, w - 20))
    img[y0:y0 + 20, x0:x0 + 17] = rng.randint(0, 256, 3)
    img[0:3, :] = rng.choice([0, 255], 3)              # saturated first rows / last columns: the edge cases
    img[:, w - 2:] = rng.choice([0, 255], 3)
    img += rng.normal(0, 2.0, img.shape) if seed % 2 else 0.0
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(arr, **kw):
    buf = io.BytesIO()
    mode = "L" if arr.ndim == 2 else "RGB"
    Image.fromarray(arr, mode).save(buf, format="jpeg", **kw)
    return buf.getvalue()


def pil_decode(data):
    img = Image.open(io.BytesIO(data))
    img.load()
    assert img.mode == "RGB", img.mode
    return np.array(img, dtype=np.uint8)


def delta_x(frames):
    d = frames.copy()
    d[:, :, 1:] = frames[:, :, 1:] - frames[:, :, :-1]
    return d


def frames_of(npz):
    """The decoded frames of a loaded jpeg_case.npz."""
    return np.cumsum(npz["frames_dx"], axis=2, dtype=np.uint8)


def all_ones_dc_table(data):
    """`data` with one more length-9 code in its first DHT table (the DC luminance one, whose longest codes are 9 bits):
    the new code is all ones, which libjpeg rejects (JERR_BAD_HUFF_TABLE)."""
    p = data.index(b"\xff\xc4")
    seglen = int.from_bytes(data[p + 2:p + 4], "big")
    body = bytearray(data[p + 4:p + 2 + seglen])
    assert body[0] == 0x00 and max(i for i in range(1, 17) if body[i]) == 9, "not the standard DC luminance table"
    total = sum(body[1:17])
    body[9] += 1
    body[17 + total:17 + total] = b"\x00"
    table_end = 17 + total + 1
    assert table_end == len(body), "the first DHT holds more than one table"
    out = data[:p] + b"\xff\xc4" + (seglen + 1).to_bytes(2, "big") + bytes(body) + data[p + 2 + seglen:]
    try:
        pil_decode(out)
    except OSError:
        return out
    raise AssertionError("PIL decoded a stream with an all-ones Huffman code")


def cases():
    """(name, stream, expected status)."""
    out = []
    scenes = [scene(s) for s in range(8)]
    for q in (95, 75, 50):
        for i, s in enumerate(scenes):
            out.append(("q%d_scene%d" % (q, i), encode(s, quality=q), OK))
    for i, s in enumerate(scenes[:4]):
        out.append(("q95_optimize_scene%d" % i, encode(s, quality=95, optimize=True), OK))
    # more entropy data than the decoder keeps in LDS (24 KB): the read path for long streams
    noise = np.random.RandomState(99).randint(0, 256, (128, 128, 3)).astype(np.uint8)
    big = encode(noise, quality=100)
    assert len(big) > 26000, len(big)
    out.append(("q100_noise", big, OK))
    s = scenes[0]
    out.append(("q95_444", encode(s, quality=95, subsampling=0), UNSUPPORTED))
    out.append(("q95_422", encode(s, quality=95, subsampling=1), UNSUPPORTED))
    out.append(("q95_progressive", encode(s, quality=95, progressive=True), UNSUPPORTED))
    out.append(("q95_grayscale", encode(s[..., 0], quality=95), UNSUPPORTED))
    out.append(("q95_restart", encode(s, quality=95, restart_marker_blocks=4), UNSUPPORTED))
    out.append(("q95_64x64", encode(scene(11, (64, 64)), quality=95), SIZE))
    out.append(("q95_100x75", encode(scene(12, (75, 100)), quality=95), SIZE))
    full = encode(scenes[1], quality=95)
    for cut in (1, 2, 100, 400, len(full) // 2, len(full) - 40, len(full) - 2, len(full) - 1):
        out.append(("q95_truncated_%d" % cut, full[:cut], CORRUPT))
    bad = bytearray(full)
    assert bad[2:4] == b"\xff\xe0"                  # APP0's length -> past the end of the stream
    bad[4:6] = (len(full) + 100).to_bytes(2, "big")
    out.append(("q95_app0_length_past_end", bytes(bad), CORRUPT))
    out.append(("q95_dht_all_ones_code", all_ones_dc_table(full), CORRUPT))
    return out


def main():
    assert features.check_feature("libjpeg_turbo"), "the oracle is PIL on libjpeg-turbo (IJG libjpeg upsamples differently)"
    rows = cases()
    names, streams, status, frames, frame_of = [], [], [], [], []
    for name, data, st in rows:
        names.append(name)
        streams.append(np.frombuffer(data, np.uint8))
        status.append(st)
        if st == OK:
            frame_of.append(len(frames))
            frames.append(pil_decode(data))
        else:
            frame_of.append(-1)
    offsets = np.zeros(len(streams) + 1, np.int64)
    offsets[1:] = np.cumsum([len(s) for s in streams])
    path = os.path.join(HERE, "jpeg_case.npz")
    np.savez_compressed(path, streams=np.concatenate(streams), offsets=offsets, names=np.array(names),
                        status=np.array(status, np.int32), frames_dx=delta_x(np.stack(frames)), frame_of=np.array(frame_of, np.int64))
    print("wrote %s: %d streams (%d decodable), %d bytes" % (path, len(rows), len(frames), os.path.getsize(path)))


if __name__ == "__main__":
    main()
