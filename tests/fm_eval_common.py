"""Shared by the forward-model evaluation tests (tests/test_forward_model_eval.py, tests/test_fm_score_host.py,
tests/test_gpu_forward_model_eval.py): the plain numpy restatement of ndp_fm_score's definition, the inputs that sit on
the byte boundaries, the golden file's recipe replayed through the oracle, and the run of
tests/host_drivers/fm_score.inc through tests/host_driver.py."""
import importlib.util
import os

import numpy as np
import torch

import host_driver
from quality_common import as_float_images, norm_table, ulps  # noqa: F401  (the tests reach them through this module)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VALUES = 3 * 128 * 128
F32 = np.float32


def recipe():
    """tests/golden/make_golden_fm_eval.py as a module: the fixture's recipe (build_module, inputs, norm_frames, order)."""
    spec = importlib.util.spec_from_file_location("make_golden_fm_eval", os.path.join(HERE, "golden", "make_golden_fm_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------ the stated definition
def want_bytes(pred):
    """uint8 [n,128,128,3]: trunc(((y + 1) / 2) * 255) in fp32, in that order, saturated to 0 / 255, NaN -> 0."""
    y = np.asarray(pred, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = ((y + F32(1.0)) / F32(2.0)) * F32(255.0)
        assert v.dtype == F32
        out = np.zeros(v.shape, np.uint8)
        mid = (v > 0) & (v < 255)
        out[mid] = np.trunc(v[mid]).astype(np.uint8)
        out[v >= 255] = 255
    return np.ascontiguousarray(out.transpose(0, 2, 3, 1))


def want_mse(a, a_idx, b, b_idx):
    """float64 [n]: mean over the 49,152 values of the square of the fp32 difference a[a_idx[i]] - b[b_idx[i]], summed in
    fp64 (np.sum's pairwise order: only the summation order differs from the kernel's); NaN where an index is outside its
    array.  a, b: float32 [m,3,128,128]."""
    out = np.full(len(a_idx), np.nan)
    for i, (ia, ib) in enumerate(zip(a_idx, b_idx)):
        if 0 <= ia < len(a) and 0 <= ib < len(b):
            d = a[ia] - b[ib]
            assert d.dtype == F32
            out[i] = (d.astype(np.float64) ** 2).sum() / VALUES
    return out


def boundary_images(n, seed=0):
    """float32 [n,3,128,128] predictions for the byte test: image 0 plane 0 sits exactly on the byte boundaries 2k/255 - 1
    and one fp32 ulp either side of them, plane 1 runs beyond +-1 (both saturations), plane 2 holds NaN, +-inf and noise;
    the other images are noise reaching a little past +-1."""
    rng = np.random.RandomState(seed)
    x = (rng.rand(n, 3, 128, 128).astype(F32) * F32(2.4) - F32(1.2))
    k = np.arange(256, dtype=np.float64)
    edge = (2.0 * k / 255.0 - 1.0).astype(F32)
    plane = np.concatenate([edge, np.nextafter(edge, F32(-4)), np.nextafter(edge, F32(4))])        # 768 values
    x[0, 0] = np.resize(plane, 128 * 128).reshape(128, 128)
    x[0, 1] = np.linspace(-3.0, 3.0, 128 * 128).astype(F32).reshape(128, 128)
    x[0, 2, 0, :8] = [np.nan, np.inf, -np.inf, 1.0, -1.0, 1e30, -1e30, 0.0]
    x[0, 2, 5, 5] = np.nan
    return x


# ------------------------------------------------------------------------------------------ the host driver
def build_driver(out_dir=None, sanitize=True):
    return host_driver.build(sanitize)


def run_driver(exe, cases, work_dir, timeout=900):
    """cases: dicts with pred float32 [n,3,128,128], target / base (float32 NCHW or uint8 HWC; base may be None),
    target_idx / base_idx (int32 [n] or None), bytes (bool).  Asserts that the child exits 0 with no sanitizer report.
    Returns [(pred_err float32 [n], base_err float32 [n], bytes uint8 [n,128,128,3])]."""
    parts = [np.int32(len(cases)).tobytes()]
    for c in cases:
        n, base = len(c["pred"]), c.get("base")
        kind = lambda a: 0 if a is None else 2 if a.dtype == np.uint8 else 1       # noqa: E731
        head = [n, len(c["target"]), 0 if base is None else len(base), kind(c["target"]), kind(base),
                c.get("target_idx") is not None, c.get("base_idx") is not None, bool(c.get("bytes"))]
        parts += [np.array(head, np.int32).tobytes(), np.ascontiguousarray(c["pred"], F32).tobytes()]
        parts += [np.ascontiguousarray(a).tobytes() for a in (c["target"], base) if a is not None]
        parts += [np.ascontiguousarray(i, np.int32).tobytes() for i in (c.get("target_idx"), c.get("base_idx")) if i is not None]
    raw = np.frombuffer(host_driver.run("fm_score", b"".join(parts), work_dir, timeout=timeout, exe=exe), np.uint8)
    out, pos = [], 0
    for c in cases:
        n = len(c["pred"])
        err = raw[pos:pos + 4 * n].copy().view(F32)
        base_err = raw[pos + 4 * n:pos + 8 * n].copy().view(F32)
        by = raw[pos + 8 * n:pos + 8 * n + n * VALUES].reshape(n, 128, 128, 3)
        out.append((err, base_err, by))
        pos += 8 * n + n * VALUES
    assert pos == raw.size, (pos, raw.size)
    return out


# ------------------------------------------------------------------------------------------ the golden case's oracle
def oracle_rollouts(state, frames, actions, order, dtype=torch.float64):
    """The eval-mode rollouts of the golden recipe through the oracle's restatement (oracle.forward_model_oracle.forward,
    training=False), every step on the rollout's own prediction: [(prediction [3,128,128] of `dtype`)] in `order`
    [(trajectory, start, h)], which lists h = 1, 2, ... of one (trajectory, start) consecutively.
    state: the module's state_dict (CPU); frames float32 [B,T,3,128,128]; actions float32 [B,T,4]."""
    from oracle import forward_model_oracle as FO
    s = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in state.items()}
    preds, cur = [], None
    with torch.no_grad():
        for b, t, h in order:
            if h == 1:
                cur = frames[b, t:t + 1].to(dtype)
            cur = FO.forward(s, cur, actions[b, t + h - 1:t + h].to(dtype), training=False)
            preds.append(cur[0])
    return preds
