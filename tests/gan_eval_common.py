"""Shared by the generator evaluation tests (tests/test_gan_eval.py, tests/test_gan_score_host.py,
tests/test_gpu_gan_eval.py): the plain numpy restatement of ndp_gan_score's definition (include/ndp.h), the same formulas
in fp64 and in fp32 through torch on the CPU (the yardstick of the bounds), the cases, the comparison that both the host
driver and the kernel must pass, and the run of tests/host_drivers/gan_score.inc through tests/host_driver.py."""
import os

import numpy as np
import torch

import host_driver
from quality_common import ulps

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "gan_eval_case.npz")
F32 = np.float32
OUTPUTS = ("sample_err", "mean_err", "best_err", "best_k", "best_curve", "spread", "ndiv", "d_fake_prob", "d_pick_k", "d_pick_err")
INT_OUTPUTS = ("best_k", "d_pick_k")
NEED_ACTION = ("sample_err", "mean_err", "best_err", "best_k", "best_curve", "d_pick_err")
NEED_NOISE = ("ndiv",)
NEED_LOGITS = ("d_fake_prob", "d_pick_k", "d_pick_err")
SHAPES = ((1, 1, 1), (1, 2, 2), (11, 6, 2), (3, 7, 5), (2, 64, 2), (2, 65, 16), (1, 256, 2))
EPS = 2.0 ** -24


def out_shape(name, n, k):
    return (n, k) if name in ("sample_err", "best_curve") else (n,)


def available(case):
    """The outputs the case's inputs allow."""
    return tuple(o for o in OUTPUTS if not ((o in NEED_ACTION and case["action"] is None) or
                                            (o in NEED_NOISE and case["noise"] is None) or
                                            (o in NEED_LOGITS and case["logits"] is None)))


# ------------------------------------------------------------------------------------------ the stated definition
def _first_best(values, larger):
    """(index, running best [K]) under the rule: the first extremum wins, NaN is never chosen while a non-NaN exists,
    all NaN: index 0."""
    best, bk, run = values[0], 0, []
    for i, v in enumerate(values):
        if not np.isnan(v) and (np.isnan(best) or (v > best if larger else v < best)):
            best, bk = v, i
        run.append(best)
    return bk, np.array(run, F32)


def pair_distances(v):
    """[n,K,K] Euclidean distances inside each row of v [n,K,C], in v's own precision."""
    d = v[:, :, None, :] - v[:, None, :, :]
    return np.sqrt((d * d).sum(3))


def want_scores(x, action=None, noise=None, logits=None):
    """The definition, restated: x float32 [n,K,4], action float32 [n,4], noise float32 [n,K,nz], logits float32 [n,K]
    (each of the three may be None).  The error metrics are reproduced operation for operation (fp32 difference, fp64
    squares summed in index order, one rounding); spread, ndiv and d_fake_prob are evaluated in fp64 ("*64") -- the
    kernel's fp32 arithmetic is measured against them."""
    n, k = x.shape[:2]
    out = {}
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if action is not None:
            d = x - action[:, None, :]
            assert d.dtype == F32
            sq = d.astype(np.float64) ** 2
            s = sq[..., 0]
            for c in range(1, 4):
                s = s + sq[..., c]
            out["sample_err"] = s / 4.0                                         # float64: the kernel rounds it once
            e32 = out["sample_err"].astype(F32)
            out["mean_err"] = sq.reshape(n, -1).sum(1) / (4.0 * k)
            picks = [_first_best(e32[r], larger=False) for r in range(n)]
            out["best_k"] = np.array([p[0] for p in picks], np.int32)
            out["best_curve"] = np.stack([p[1] for p in picks])
            out["best_err"] = e32[np.arange(n), out["best_k"]]
        x64 = x.astype(np.float64)
        dx = pair_distances(x64)
        out["spread"] = dx.sum((1, 2)) / np.float64(k * (k - 1)) if k > 1 else np.full(n, np.nan)
        if noise is not None:
            dz = pair_distances(noise.astype(np.float64))
            h = 0.8 * (dz / dz.sum(2)[..., None]) - dx / dx.sum(2)[..., None]
            out["ndiv"] = np.where((h > 0) | np.isnan(h), h, 0.0).sum((1, 2))
        if logits is not None:
            out["d_fake_prob"] = (1.0 / (1.0 + np.exp(-logits.astype(np.float64)))).mean(1)
            out["d_pick_k"] = np.array([_first_best(logits[r], larger=True)[0] for r in range(n)], np.int32)
            if action is not None:
                out["d_pick_err"] = e32[np.arange(n), out["d_pick_k"]]
    return out


def torch_fp32(x, noise=None, logits=None):
    """spread, ndiv and d_fake_prob by the same formulas in fp32 through torch on the CPU (the reference's expressions:
    diversity.py:8-19, 36-41 with the sum kept per row; torch.sigmoid): float64 arrays of the fp32 results."""
    n, k = x.shape[:2]
    out = {}
    pairwise = lambda z: torch.norm(z[:, :, None, :] - z[:, None, :, :], p=2, dim=3)      # noqa: E731
    tx = torch.from_numpy(np.ascontiguousarray(x))
    dx = pairwise(tx)
    out["spread"] = (dx.sum((1, 2)) / F32(k * (k - 1))).numpy().astype(np.float64) if k > 1 else np.full(n, np.nan)
    if noise is not None:
        dz = pairwise(torch.from_numpy(np.ascontiguousarray(noise)))
        z_delta, x_delta = dz / dz.sum(2)[..., None], dx / dx.sum(2)[..., None]
        out["ndiv"] = torch.relu(z_delta * 0.8 - x_delta).sum((1, 2)).numpy().astype(np.float64)
    if logits is not None:
        out["d_fake_prob"] = torch.sigmoid(torch.from_numpy(np.ascontiguousarray(logits))).mean(1).numpy().astype(np.float64)
    return out


def tolerance(name, want64, want32, k):
    """The bound on |got - want64| for spread / ndiv / d_fake_prob: max(4 x the distance of the same formula in fp32
    through torch on the CPU, a floor) -- the floor is 4 ulp of the value (spread, d_fake_prob) or 8 K 2^-24 absolute
    (ndiv: K^2 hinge terms of size ~1/K, each a difference of two fp32 quotients)."""
    ref = 4.0 * np.abs(want32 - want64)
    floor = np.full(want64.shape, 8.0 * k * EPS) if name == "ndiv" else 4.0 * np.spacing(np.abs(want64).astype(F32)).astype(np.float64)
    return np.fmax(ref, floor)                                                  # fmax: a NaN side is ignored


def check_scores(case, got, wanted=None):
    """Asserts everything the definition fixes about `got` ({output: array}) for `case`; returns {output: (max distance
    of the kernel from the fp64 value, max distance of torch's fp32 from it, max bound)} for spread / ndiv / d_fake_prob
    over the rows that are not NaN."""
    x, k, name = case["x"], case["x"].shape[1], case["name"]
    want = want_scores(x, case["action"], case["noise"], case["logits"])
    t32 = torch_fp32(x, case["noise"], case["logits"])
    wanted = available(case) if wanted is None else wanted
    measured = {}
    for o in wanted:
        g, w = np.asarray(got[o]), np.asarray(want[o])
        assert g.shape == w.shape, (name, o, g.shape, w.shape)
        if o in INT_OUTPUTS:
            assert np.array_equal(g, w), (name, o, g, w)
            continue
        bad = np.isnan(w)
        assert np.array_equal(np.isnan(g), bad), (name, o, g, w)
        if o in ("spread", "ndiv", "d_fake_prob"):
            dist, tol = np.abs(g.astype(np.float64) - w)[~bad], tolerance(o, w, t32[o], k)[~bad]
            if dist.size:
                measured[o] = (dist.max(), np.abs(t32[o] - w)[~bad].max(), tol.max())
            assert (dist <= tol).all(), (name, o, dist, tol)
        else:
            assert (ulps(g[~bad], w[~bad]) <= 1).all(), (name, o, g, w)
    return measured


# ------------------------------------------------------------------------------------------ the cases
def random_case(n, k, nz, seed, name=None):
    rng = np.random.RandomState(seed)
    return dict(x=(rng.rand(n, k, 4).astype(F32) * F32(2) - F32(1)), action=(rng.rand(n, 4).astype(F32) * F32(2) - F32(1)),
                noise=rng.rand(n, k, nz).astype(F32), logits=(rng.randn(n, k).astype(F32) * F32(3)),
                name=name or ("random", n, k, nz))


def special_case(k, nz, seed):
    """4 rows of K >= 4 samples: row 0 has two equal samples (dx_ij = 0) that tie for the minimum error and for the
    largest logit, row 1 one NaN sample -- sample 0, where the running best starts -- with a NaN logit, row 2 is all NaN
    (samples and logits), row 3 is ordinary."""
    c = random_case(4, k, nz, seed, name=("special", 4, k, nz))
    near = c["action"][0] + F32(1e-3)
    c["x"][0, 1] = c["x"][0, 3] = near
    c["logits"][0, 1] = c["logits"][0, 3] = F32(50.0)
    c["x"][1, 0, 2] = np.nan
    c["logits"][1, 0] = np.nan
    c["x"][2] = np.nan
    c["logits"][2] = np.nan
    return c


def without(case, *inputs):
    c = dict(case)
    for i in inputs:
        c[i] = None
    c["name"] = tuple(case["name"]) + ("without",) + inputs
    return c


def cases():
    """[(case, wanted outputs)]: the seven shapes, the special rows on both sides of the one-wave limit, and -- on the
    (11,6,2) data -- every optional input and every output absent in turn."""
    out = [(random_case(n, k, nz, seed=100 + i), None) for i, (n, k, nz) in enumerate(SHAPES)]
    out += [(special_case(6, 2, seed=7), None), (special_case(65, 3, seed=8), None)]
    base = out[2][0]
    for missing in ("action", "noise", "logits"):
        out.append((without(base, missing), None))
    for o in OUTPUTS:
        c = dict(base, name=tuple(base["name"]) + ("no output", o))
        out.append((c, tuple(w for w in OUTPUTS if w != o)))
    return out


# ------------------------------------------------------------------------------------------ the host driver
def build_driver(out_dir=None, sanitize=True):
    return host_driver.build(sanitize)


def run_driver(exe, case_list, work_dir, timeout=600):
    """case_list: [(case, wanted outputs or None)].  Asserts that the child exits 0 with no sanitizer report.  Returns
    [{output: array}] with every output at its full size; one that was not wanted holds the sentinel -7."""
    parts = [np.int32(len(case_list)).tobytes()]
    for c, wanted in case_list:
        n, k = c["x"].shape[:2]
        wanted = available(c) if wanted is None else wanted
        mask = sum(1 << i for i, o in enumerate(OUTPUTS) if o in wanted)
        nz = c["noise"].shape[2] if c["noise"] is not None else 1
        head = [n, k, nz, c["action"] is not None, c["noise"] is not None, c["logits"] is not None, mask]
        parts.append(np.array(head, np.int32).tobytes())
        parts += [np.ascontiguousarray(a, F32).tobytes() for a in (c["x"], c["action"], c["noise"], c["logits"]) if a is not None]
    raw = np.frombuffer(host_driver.run("gan_score", b"".join(parts), work_dir, timeout=timeout, exe=exe), np.uint8)
    results, pos = [], 0
    for c, _ in case_list:
        n, k = c["x"].shape[:2]
        got = {}
        for o in OUTPUTS:
            shape = out_shape(o, n, k)
            size = 4 * int(np.prod(shape))
            got[o] = raw[pos:pos + size].copy().view(np.int32 if o in INT_OUTPUTS else F32).reshape(shape)
            pos += size
        results.append(got)
    assert pos == raw.size, (pos, raw.size)
    return results
