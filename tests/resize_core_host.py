"""Shared by the resize tests (tests/test_resize_core_host.py, tests/test_gpu_resize.py, tests/golden/make_golden_resize.py):
the frame sizes and contents, PIL's resize, and the run of tests/host_drivers/resize.inc through tests/host_driver.py."""
import numpy as np

import host_driver

SIZES = ((500, 500), (480, 640), (37, 53), (129, 127), (128, 300), (300, 128), (128, 128), (1, 1), (1, 2048), (2048, 1),
         (2048, 2048))                                        # (H, W)
CONTENTS = ("noise", "binary", "gradient")
FIELDS = ("equal", "mismatches", "schedules", "kx", "ky", "worst_lo", "worst_hi", "max_tile_rows")
FRAME = 128 * 128 * 3


def make_frame(h, w, content, seed=0):
    """uint8 [h,w,3]: seeded uniform noise, random 0/255 pixels (Lanczos overshoots past both ends of the byte range, so
    both clamps fire), or gradients that differ per channel."""
    rng = np.random.RandomState(1000 * h + w + 7919 * seed)
    if content == "noise":
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if content == "binary":
        return (rng.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    if content == "gradient":
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 3) % 256], axis=2).astype(np.uint8)
    raise ValueError(content)


def pil_resize(frame):
    """MPC_gym_eval.get_state's resize: Image.fromarray(frame).resize((128, 128), Image.LANCZOS)."""
    from PIL import Image
    return np.array(Image.fromarray(frame).resize((128, 128), Image.LANCZOS))


def build_driver(out_dir=None, sanitize=True):
    return host_driver.build(sanitize)


def run_driver(exe, cases, work_dir, timeout=900):
    """cases: [(frame uint8 [h,w,3], expected uint8 [128,128,3])].  Asserts that the child exits 0 with no sanitizer
    report.  Returns ({field: int32 [n]}, resized uint8 [n,128,128,3])."""
    parts = [np.int32(len(cases)).tobytes()]
    for frame, want in cases:
        parts += [np.array(frame.shape[:2], np.int32).tobytes(), np.ascontiguousarray(frame, np.uint8).tobytes(),
                  np.ascontiguousarray(want, np.uint8).tobytes()]
    raw = np.frombuffer(host_driver.run("resize", b"".join(parts), work_dir, timeout=timeout, exe=exe), np.uint8)
    per = 4 * len(FIELDS) + FRAME
    assert raw.size == len(cases) * per, (raw.size, len(cases), per)
    raw = raw.reshape(len(cases), per)
    ints = raw[:, :4 * len(FIELDS)].copy().view(np.int32)
    return {k: ints[:, i].copy() for i, k in enumerate(FIELDS)}, raw[:, 4 * len(FIELDS):].reshape(-1, 128, 128, 3)
