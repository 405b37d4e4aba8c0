"""Writes tests/golden/resize_case.npz: two seeded camera frames and what Pillow's
`Image.fromarray(frame).resize((128, 128), Image.LANCZOS)` makes of them -- the pin that tells a change of Pillow's resampler
from a change of the kernel.  frame_a is 53 rows x 37 columns (enlarged on both axes), frame_b 120 x 160 (the size
tests/fake_push_env.py renders; reduced on one axis, both passes run).  Run from the repository root:
    python tests/golden/make_golden_resize.py
"""
import os
import sys

import numpy as np
import PIL

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resize_core_host as R  # noqa: E402


def tiles(h, w, size, seed):
    """uint8 [h,w,3] of size x size tiles, each of one seeded colour."""
    rng = np.random.RandomState(seed)
    colours = rng.randint(0, 256, ((h + size - 1) // size, (w + size - 1) // size, 3)).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(colours, size, axis=0), size, axis=1)[:h, :w])


def main():
    # flat seeded tiles (sharp edges in both directions) with small patches of noise and of 0/255 pixels: every path of
    # the filter, and a file of a few tens of KB
    a = tiles(53, 37, 6, 1)
    a[10:22, 8:20] = R.make_frame(12, 12, "noise", seed=1)
    a[30:42, 15:30] = R.make_frame(12, 15, "binary", seed=4)
    b = tiles(120, 160, 20, 2)
    b[20:44, 100:130] = R.make_frame(24, 30, "noise", seed=2)
    b[60:80, 40:70] = R.make_frame(20, 30, "binary", seed=3)
    out = {"frame_a": a, "frame_b": b, "resized_a": R.pil_resize(a), "resized_b": R.pil_resize(b),
           "pillow_version": np.array(PIL.__version__)}
    assert out["resized_a"].min() == 0 and out["resized_a"].max() == 255      # enlarged 0/255 pixels: both clamps fire
    path = os.path.join(HERE, "resize_case.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
