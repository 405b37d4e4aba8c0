#!/usr/bin/env python3
"""Golden vector for ndp_image_quality (SSIM and PSNR).  Nothing in the reference computes either; the expected
values come from a route that is deliberately not the kernel's: scikit-image's recipe for structural_similarity with
gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range=1 -- scipy.ndimage.gaussian_filter(a, 1.5,
truncate=3.5, mode="reflect") over each whole channel in fp64, S cropped by 5 pixels -- where the kernel sums the valid
windows directly in fp32.  Needs scipy; the .npz holds data only.

The images (bytes [128,128,3], from `synthetic_scene` with fixed seeds and one RandomState):
    scene0, scene1        two seeded scenes
    scene0_light / heavy  scene0 + N(0, 5) / N(0, 50) per byte, clipped
    scene0_inverse        255 - scene0
    black, white          all 0 / all 255
    noise0, noise1        uniform byte noise
The pairs, in tests/quality_common.NAMES' order: the eight kinds the definition was checked on -- identical, light noise,
heavy noise, unrelated scenes, a flat grey frame with 1e-4 noise, black against white, byte noise, the inverse image --
then two float pairs whose values leave [-1, 1] and one pair with a single NaN.  Seven exist as bytes; "grey" and the last
three are fp32 functions of the stored bytes (quality_common.golden_pairs), so the file stays small.

Stored per pair: ssim64 (the scipy route on the fp32 unit images, NaN for the NaN pair), ssim64_direct (the direct
valid-window sum in fp64: the two routes' distance is printed), psnr64 (the stated definition in fp64; +Inf for the
identical pair), ssim32 (the plain numpy fp32 restatement of the direct route), and d32 = max |ssim32 - ssim64| over the
pairs without a NaN: the allowance of the kernel tests is 4 * d32.

Usage: python tests/golden/make_golden_image_quality.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import quality_common as Q  # noqa: E402
from ndivplanning_amd.utils.trajectory_loader import synthetic_scene  # noqa: E402

SCENE_SEED, NOISE_SEED = 5, 0


def build_images():
    gen = torch.Generator().manual_seed(SCENE_SEED)
    rng = np.random.RandomState(NOISE_SEED)
    s0, s1 = synthetic_scene(gen), synthetic_scene(gen)
    noisy = lambda sd: np.clip(np.rint(s0.astype(np.float64) + rng.randn(*s0.shape) * sd), 0, 255).astype(np.uint8)  # noqa: E731
    images = {
        "scene0": s0, "scene1": s1, "scene0_light": noisy(5.0), "scene0_heavy": noisy(50.0), "scene0_inverse": 255 - s0,
        "black": np.zeros_like(s0), "white": np.full_like(s0, 255),
        "noise0": rng.randint(0, 256, s0.shape).astype(np.uint8), "noise1": rng.randint(0, 256, s0.shape).astype(np.uint8),
    }
    pairs = [("identical", "scene0", "scene0"), ("light_noise", "scene0", "scene0_light"),
             ("heavy_noise", "scene0", "scene0_heavy"), ("unrelated", "scene0", "scene1"), ("black_white", "black", "white"),
             ("byte_noise", "noise0", "noise1"), ("inverse", "scene0", "scene0_inverse")]
    return images, pairs


def main():
    images, pairs = build_images()
    names = list(images)
    rec = {
        "images_u8": np.stack([images[n] for n in names]), "image_names": np.array(names),
        "pair_names": np.array([p[0] for p in pairs]),
        "pair_a": np.array([names.index(p[1]) for p in pairs], np.int32),
        "pair_b": np.array([names.index(p[2]) for p in pairs], np.int32),
    }
    ssim64, direct64, psnr, ssim32 = [], [], [], []
    for name, a, b in Q.golden_pairs(rec):
        ua, ub = Q.as_unit(a), Q.as_unit(b)
        ssim64.append(Q.ssim_scipy(ua, ub))
        direct64.append(Q.ssim_direct(ua, ub, np.float64)[0])
        psnr.append(Q.psnr64(ua, ub))
        s32, s_map = Q.ssim_direct(ua, ub, np.float32)
        ssim32.append(s32)
        if name == "identical":
            assert (s_map == 1).all() and s32 == 1.0, "the fp32 restatement must give exactly 1 on identical images"
        print("%-12s ssim64 %.12f  direct64 - scipy %+.2e  fp32 - scipy %+.2e  psnr %.6f"
              % (name, ssim64[-1], direct64[-1] - ssim64[-1], s32 - ssim64[-1], psnr[-1]))
    ssim64, direct64, ssim32 = np.array(ssim64), np.array(direct64), np.array(ssim32)
    finite = ~np.isnan(ssim64)
    assert finite.sum() == len(Q.NAMES) - 1 and np.isnan(ssim64[Q.NAMES.index("one_nan")])
    routes = np.abs(direct64 - ssim64)[finite].max()
    d32 = np.abs(ssim32 - ssim64)[finite].max()
    print("routes agree to %.2e; d32 = %.3e" % (routes, d32))
    assert routes < 1e-12
    rec.update(ssim64=ssim64, ssim64_direct=direct64, psnr64=np.array(psnr), ssim32=ssim32, d32=np.float64(d32),
               scene_seed=np.int32(SCENE_SEED), noise_seed=np.int32(NOISE_SEED))
    path = os.path.join(HERE, "image_quality_case.npz")
    np.savez_compressed(path, **rec)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
