"""Shared by the image-quality tests (tests/test_image_quality.py, tests/test_image_quality_host.py,
tests/test_gpu_image_quality.py) and by tests/golden/make_golden_image_quality.py: the plain numpy restatements of
ndp_image_quality's definition -- the fp32 scaling, PSNR, SSIM by the direct valid-window sum in fp64 and in
fp32, and SSIM by the scikit-image route (scipy's gaussian_filter over the whole channel, cropped by 5) -- the golden
file's pairs, and the run of tests/host_drivers/image_quality.inc through tests/host_driver.py.  `norm_table`,
`as_float_images` and `ulps` are also the forward-model and generator evaluation tests' (fm_eval_common, gan_eval_common)."""
import numpy as np

import host_driver

VALUES = 3 * 128 * 128
OUT = 118
F32 = np.float32
C1, C2 = 0.01 ** 2, 0.03 ** 2
# the golden pairs, in the file's order; the first eight are the kinds of the definition's check, "grey" and the last
# three exist as floats only
NAMES = ("identical", "light_noise", "heavy_noise", "unrelated", "grey", "black_white", "byte_noise", "inverse",
         "outside_1", "outside_2", "one_nan")
FLOAT_ONLY = ("grey", "outside_1", "outside_2", "one_nan")


# ------------------------------------------------------------------------------------------ the stated definition
def norm_table():
    """The 256-entry table of ndp_eval_frames_u8: ((float)i / 255 - 0.5) * 2 in fp32."""
    return (np.arange(256, dtype=F32) / F32(255.0) - F32(0.5)) * F32(2.0)


def as_float_images(frames):
    """float32 [m,3,128,128] of float images (as they are) or byte frames [m,128,128,3] (through the table)."""
    frames = np.asarray(frames)
    if frames.dtype == np.uint8:
        return np.ascontiguousarray(norm_table()[frames].transpose(0, 3, 1, 2))
    return frames.astype(F32, copy=False)


def unit(x):
    """u = (x + 1) * 0.5 in fp32, clamped to [0, 1]; -Inf -> 0, +Inf -> 1, NaN stays NaN."""
    with np.errstate(invalid="ignore"):
        u = (np.asarray(x, F32) + F32(1.0)) * F32(0.5)
        assert u.dtype == F32
        u = np.where(u < 0, F32(0.0), np.where(u > 1, F32(1.0), u))
    return u.astype(F32)


def taps(dtype):
    """g[i] ~ exp(-(i - 5)^2 / (2 * 1.5^2)), normalised to sum 1 in double, rounded to `dtype` once."""
    i = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-i * i / (2 * 1.5 ** 2))
    return (g / g.sum()).astype(dtype)


def psnr64(ua, ub):
    """float64: 10 log10(1 / mse) of the fp32 difference of two unit images [3,128,128], squares summed in fp64 (np.sum's
    pairwise order: only the summation order differs from the kernel's); mse == 0: +Inf."""
    with np.errstate(invalid="ignore", divide="ignore"):
        d = ua - ub
        assert d.dtype == F32
        mse = (d.astype(np.float64) ** 2).sum() / VALUES
        return np.inf if mse == 0 else float(10.0 * np.log10(1.0 / mse))


def _s_map(ux, uy, uxx, uyy, uxy, dt):
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    c1, c2 = dt(C1), dt(C2)
    return ((dt(2) * ux * uy + c1) * (dt(2) * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))


def ssim_direct(ua, ub, dt):
    """(mean, S [3,118,118]): the direct route in `dt` (np.float64: the definition; np.float32: the plain restatement of
    what the kernel computes, taps summed in order by separate multiplies and adds) over the windows wholly inside the
    image; the mean of S is taken in fp64."""
    g, x, y = taps(dt), ua.astype(dt), ub.astype(dt)

    def f(a):
        h = np.zeros((3, 128, OUT), dt)
        for k in range(11):
            h = h + g[k] * a[:, :, k:k + OUT]
        v = np.zeros((3, OUT, OUT), dt)
        for k in range(11):
            v = v + g[k] * h[:, k:k + OUT, :]
        assert v.dtype == dt
        return v
    with np.errstate(invalid="ignore"):
        s = _s_map(f(x), f(y), f(x * x), f(y * y), f(x * y), dt)
    return float(s.astype(np.float64).mean()), s


def ssim_scipy(ua, ub):
    """float64: scikit-image's route (structural_similarity with gaussian_weights=True, sigma=1.5,
    use_sample_covariance=False, data_range=1, per channel, averaged): gaussian_filter(truncate=3.5, mode="reflect") over
    the whole channel, S cropped by 5 pixels."""
    from scipy.ndimage import gaussian_filter
    x, y = ua.astype(np.float64), ub.astype(np.float64)
    out = []
    for c in range(3):
        f = lambda a: gaussian_filter(a, 1.5, truncate=3.5, mode="reflect")      # noqa: E731
        s = _s_map(f(x[c]), f(y[c]), f(x[c] * x[c]), f(y[c] * y[c]), f(x[c] * y[c]), np.float64)
        out.append(s[5:-5, 5:-5].mean())
    return float(np.mean(out))


def ulps(got, want64):
    """|got - want| in units of the fp32 spacing at want (got float32, want float64)."""
    want64 = np.asarray(want64, np.float64)
    return np.abs(np.asarray(got, np.float64) - want64) / np.spacing(np.abs(want64).astype(F32)).astype(np.float64)


# ------------------------------------------------------------------------------------------ the golden pairs
def golden_pairs(rec):
    """[(name, a, b)] of the golden record `rec` (image_quality_case.npz): a, b are byte frames uint8 [128,128,3] where
    the pair exists as bytes, else float32 [3,128,128].  The float-only pairs are fp32 functions of stored bytes (one
    rounding per operation, so every machine builds the same bits):
      grey       x = 0 against (noise bytes' floats) * 3.5e-4: a flat grey frame with noise of standard deviation 1e-4 in unit scale
      outside_1  scene floats * 1.5 against the light-noise floats * 1.5: both leave [-1, 1]
      outside_2  scene floats * 1.25 + 0.5 against the unrelated scene's floats * 3 - 1
      one_nan    the heavy-noise pair as floats with one NaN in a (channel 1, row 60, column 70)"""
    img = rec["images_u8"]
    fl = as_float_images(img)
    by_name = {str(n): i for i, n in enumerate(rec["image_names"])}
    pairs = []
    for name, ia, ib in zip(rec["pair_names"], rec["pair_a"], rec["pair_b"]):
        pairs.append((str(name), img[ia], img[ib]))
    s0, light, heavy, s1, noise = (by_name[k] for k in ("scene0", "scene0_light", "scene0_heavy", "scene1", "noise0"))
    nan_a = fl[s0].copy()
    nan_a[1, 60, 70] = np.nan
    extra = {
        "grey": (np.zeros((3, 128, 128), F32), fl[noise] * F32(3.5e-4)),
        "outside_1": (fl[s0] * F32(1.5), fl[light] * F32(1.5)),
        "outside_2": (fl[s0] * F32(1.25) + F32(0.5), fl[s1] * F32(3.0) - F32(1.0)),
        "one_nan": (nan_a, fl[heavy]),
    }
    pairs += [(k, extra[k][0], extra[k][1]) for k in FLOAT_ONLY]
    pairs.sort(key=lambda p: NAMES.index(p[0]))
    assert tuple(p[0] for p in pairs) == NAMES
    return pairs


def as_unit(x):
    """The unit image float32 [3,128,128] of one operand: a byte frame [128,128,3] or a float image [3,128,128]."""
    return unit(as_float_images(np.asarray(x)[None])[0])


def as_float(x):
    return as_float_images(np.asarray(x)[None])[0]


# ------------------------------------------------------------------------------------------ the host driver
def build_driver(out_dir=None, sanitize=True):
    return host_driver.build(sanitize)


def run_driver(exe, cases, work_dir, timeout=900):
    """cases: dicts with a, b (float32 [m,3,128,128] or uint8 [m,128,128,3]), a_idx / b_idx (int32 [n] or None), n
    (pairs), rows (output rows per band), ssim / psnr (bool, default True).  Asserts that the child exits 0 with no
    sanitizer report.  Returns [(ssim float32 [n], psnr float32 [n])], -7 where not wanted."""
    parts = [np.int32(len(cases)).tobytes()]
    for c in cases:
        kind = lambda a: 2 if a.dtype == np.uint8 else 1       # noqa: E731
        maps = (1 if c.get("a_idx") is not None else 0) | (2 if c.get("b_idx") is not None else 0)
        want = (1 if c.get("ssim", True) else 0) | (2 if c.get("psnr", True) else 0)
        head = [c["n"], len(c["a"]), len(c["b"]), kind(c["a"]), kind(c["b"]), maps, c["rows"], want]
        parts += [np.array(head, np.int32).tobytes(), np.ascontiguousarray(c["a"]).tobytes(), np.ascontiguousarray(c["b"]).tobytes()]
        for idx in (c.get("a_idx"), c.get("b_idx")):
            if idx is not None:
                assert len(idx) == c["n"]
                parts.append(np.ascontiguousarray(idx, np.int32).tobytes())
    raw = np.frombuffer(host_driver.run("image_quality", b"".join(parts), work_dir, timeout=timeout, exe=exe), F32)
    out, pos = [], 0
    for c in cases:
        n = c["n"]
        out.append((raw[pos:pos + n].copy(), raw[pos + n:pos + 2 * n].copy()))
        pos += 2 * n
    assert pos == raw.size, (pos, raw.size)
    return out
