"""What the tests of the planner's MPPI weighting and warm start share (tests/test_plan_warm_host.py and
tests/test_plan_warm.py on the CPU, tests/test_gpu_plan_warm.py on the GPU): the plain numpy restatements of
ndp_plan_update and ndp_plan_warm as include/ndp.h states them (fp64, np.exp, one rounding to fp32 per stored value), the
cases, the comparison with its exact / 1-ulp split, the build of the host-driver program of
tests/host_drivers/plan_warm_main.hip and the packing for its body plan_warm.inc, the refused arguments, and
`RecordingWarmModels`, plan_common.RecordingModels with the two new calls."""
import ctypes
import os
import struct

import numpy as np
import torch

import plan_common as C

ELITES, MPPI = 0, 1                                                   # NDP_PLAN_ELITES, NDP_PLAN_MPPI
# (B, W, steps_prev, steps): the smallest, a few rows, a shrinking horizon, W across a wave, the limits
WARM_SHAPES = ((1, 1, 1, 1), (3, 2, 3, 3), (3, 2, 3, 2), (2, 64, 32, 32), (1, 255, 32, 31))
UPDATE_OUTPUTS = C.OUTPUTS
WARM_OUTPUTS = ("mean", "std", "warm")


# ---------------------------------------------------------------------------------------------- the restatements
def mppi_weights(e, temperature):
    """w_k of the elites' errors e (rank order, no NaN): 1 for the best and its equals, else exp(-(e_k - e_0) / T) in
    fp64."""
    t = np.float64(np.float32(temperature))
    with np.errstate(all="ignore"):
        return [np.float64(1.0) if ek == e[0] else np.exp(-(np.float64(ek) - np.float64(e[0])) / t) for ek in e]


def plan_update(c):
    """ndp_plan_update on the case `c` (plan_common's keys and weighting, temperature, smooth, first)."""
    err, seq, normal = c["err"], c["seq_in"], c["normal"]
    th, b_n, r, _ = seq.shape
    e_n, smooth, first = c["elites"], c["smooth"], c["first"]
    mo, least = np.float64(np.float32(c["momentum"])), np.float64(np.float32(c["min_std"]))
    low, high = c["low"].astype(np.float32), c["high"].astype(np.float32)
    mean, std, best = c["mean"].copy(), c["std"].copy(), c["best_err"].copy()
    out = np.empty_like(seq)
    elite_idx = np.full((b_n, e_n), -1, np.int32)
    for b in range(b_n):
        order = C.rank_order(err[b])
        ne = min(e_n, int((~np.isnan(err[b])).sum()))
        elite_idx[b, :ne] = order[:ne]
        if ne == 0:
            if not smooth:
                mean[b], std[b] = 0.0, np.float32(c["min_std"])
        else:
            rows = [seq[:, b, k, :].astype(np.float64) for k in order[:ne]]
            if c["weighting"] == MPPI:
                w = mppi_weights([err[b, k] for k in order[:ne]], c["temperature"])
                weight, total = np.float64(0.0), np.zeros((th, 4), np.float64)
                for wk, x in zip(w, rows):
                    weight = weight + wk
                    total = total + wk * x
                m = total / weight
                dev = np.zeros((th, 4), np.float64)
                for wk, x in zip(w, rows):
                    d = x - m
                    dev = dev + wk * (d * d)
                s = np.sqrt(dev / weight)
            else:
                total = np.zeros((th, 4), np.float64)
                for x in rows:
                    total = total + x
                m = total / np.float64(ne)
                dev = np.zeros((th, 4), np.float64)
                for x in rows:
                    d = x - m
                    dev = dev + d * d
                s = np.sqrt(dev / np.float64(ne))
            if smooth:
                keep = np.float64(1.0) - mo
                m = mo * mean[b].astype(np.float64) + keep * m
                s = mo * std[b].astype(np.float64) + keep * s
            with np.errstate(invalid="ignore"):
                s = np.where(s > least, s, least)
            mean[b], std[b] = m.astype(np.float32), s.astype(np.float32)
        out[:, b] = _draw(std[b], normal[:, b], mean[b], low, high)
        out[:, b, 0] = seq[:, b, order[0]]
        e0 = err[b, order[0]]
        if first or e0 < best[b] or np.isnan(best[b]):
            best[b] = e0
    return {"mean": mean, "std": std, "seq_out": out, "best_err": best, "elite_idx": elite_idx}


def _clamp(v, low, high):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v), v, np.minimum(np.maximum(v, low), high))


def _draw(std, normal, mean, low, high):
    """(float)((double)std * (double)n + (double)mean), clamped: std, mean [Th,4], normal [Th,rows,4]."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = (std.astype(np.float64)[:, None, :] * normal.astype(np.float64) + mean.astype(np.float64)[:, None, :])
        return _clamp(v.astype(np.float32), low, high)


def plan_warm(c):
    """ndp_plan_warm on the case `c`: mean_prev, std_prev [B,steps_prev,4], normal [steps,B,W,4], warm_std, low, high."""
    mean_prev, std_prev, normal = c["mean_prev"], c["std_prev"], c["normal"]
    steps, b_n, w, _ = normal.shape
    sp = mean_prev.shape[1]
    floor = np.float32(c["warm_std"])
    low, high = c["low"].astype(np.float32), c["high"].astype(np.float32)
    src = [min(ts + 1, sp - 1) for ts in range(steps)]
    mean = mean_prev[:, src].copy()
    with np.errstate(invalid="ignore"):
        std = np.where(std_prev[:, src] > floor, std_prev[:, src], floor).astype(np.float32)
    warm = np.empty_like(normal)
    for b in range(b_n):
        warm[:, b] = _draw(std[b], normal[:, b], mean[b], low, high)
        warm[:, b, 0] = _clamp(mean[b], low, high)
    return {"mean": mean, "std": std, "warm": warm}


# ---------------------------------------------------------------------------------------------- the cases
def _update_case(name, shape, seed, weighting, smooth, first, temperature=0.1, **kw):
    c = C._case(name, shape, seed, first, **kw)
    c.update(weighting=weighting, temperature=temperature, smooth=int(smooth), first=int(first))
    return c


def update_cases():
    """Every shape of plan_common.SHAPES with: smooth / first in all four combinations, ties, NaN errors, +inf errors
    (among the elites, and as e_0), fewer numbers than E, all NaN (smoothed and not), a binding min_std, clamping bounds;
    each with both weightings."""
    out = []
    for si, shape in enumerate(C.SHAPES):
        b, r, e, th = shape
        for weighting in (MPPI, ELITES):
            seed = 1000 + 100 * si + 50 * weighting

            def case(tag, k, smooth=0, first=1, **kw):
                return _update_case((tag, shape, weighting, smooth, first), shape, seed + k, weighting, smooth, first, **kw)
            for k, (smooth, first) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                out.append(case("flags", k, smooth, first))
            c = case("ties", 4, 1, 0)
            c["err"][:, r - 1] = c["err"][:, 0] = c["err"].min(axis=1) * np.float32(0.5)   # the minimum twice: row 0 wins
            if r > 3:
                c["err"][:, 2] = c["err"][:, 1]
            out.append(c)
            c = case("nan", 5, 1, 1)
            c["err"][:, ::2] = np.nan                                 # every other error; rows 1, 3, .. stay numbers
            out.append(c)
            c = case("inf", 6, 0, 0)
            c["err"][:, 1:] = np.inf                                  # one finite error: the other elites weigh 0
            c["err"][b - 1, r - 1] = np.nan
            out.append(c)
            c = case("e0 inf", 7, 1, 0)
            c["err"][:] = np.inf                                      # nothing finite: all ones by the equality rule
            if r > 2:
                c["err"][0, 1] = np.nan
            out.append(c)
            c = case("fewer", 8, 0, 1)
            c["err"][:] = np.nan                                      # one number, E' = 1 (E = 1: as many as E)
            c["err"][:, r // 2] = np.float32(0.7)
            out.append(c)
            for k, smooth in enumerate((0, 1)):
                c = case("all nan", 9 + k, smooth, smooth)
                c["err"][:] = np.nan
                out.append(c)
            out.append(case("min_std binds", 11, 1, 0, min_std=2.0, momentum=0.5))
            out.append(case("clamp", 12, 0, 1, low=-0.25, high=0.3, spread=1.0))
    return out


def limit_cases():
    """The two exact properties of the MPPI refit, on every shape: at temperature 1e30 every weight of a finite error rounds
    to 1 and the refit is the elites' operation for operation; at 1e-30 on distinct errors every weight but w_0 is 0."""
    out = []
    for si, shape in enumerate(C.SHAPES):
        for smooth in (0, 1):
            hot = _update_case(("hot", shape, smooth), shape, 2000 + si, MPPI, smooth, 1 - smooth, temperature=1e30)
            out.append((hot, dict(hot, weighting=ELITES)))
        cold = _update_case(("cold", shape), shape, 2100 + si, MPPI, 0, 1, temperature=1e-30, min_std=0.125)
        assert all(len(set(row.tolist())) == len(row) for row in cold["err"])
        out.append((cold, None))
    return out


def warm_cases():
    """Every shape of WARM_SHAPES with a binding and a non-binding warm_std, a NaN deviation, and clamping bounds."""
    out = []
    for si, (b, w, sp, steps) in enumerate(WARM_SHAPES):
        for k, (tag, warm_std, low, high, spread) in enumerate((("floor binds", 0.5, -1.0, 1.0, 0.2),
                                                                ("floor idle", 0.01, -1.0, 1.0, 0.2),
                                                                ("nan std", 0.25, -1.0, 1.0, 0.2),
                                                                ("clamp", 0.05, -0.25, 0.3, 1.0))):
            g = np.random.default_rng(3000 + 10 * si + k)
            c = {"name": (tag, (b, w, sp, steps)), "warm_std": warm_std,
                 "low": np.full(4, low, np.float32), "high": np.full(4, high, np.float32),
                 "mean_prev": (spread * g.standard_normal((b, sp, 4))).astype(np.float32),
                 "std_prev": (0.05 + 0.3 * g.random((b, sp, 4))).astype(np.float32),
                 "normal": g.standard_normal((steps, b, w, 4)).astype(np.float32)}
            if tag == "nan std":
                c["std_prev"][:, sp - 1, 1] = np.nan                  # read at every ts >= steps_prev - 2
                c["mean_prev"][0, sp - 1, 3] = np.nan                 # a NaN mean stays a NaN
            if tag == "clamp":
                c["low"], c["high"] = np.float32([-0.25, -1.0, 0.125, -2.0]), np.float32([0.3, -0.75, 0.125, 2.0])
            out.append(c)
    return out


def check_warm_special(c, got):
    b, w, sp, steps = c["name"][1]
    floor = np.float32(c["warm_std"])
    if c["name"][0] == "floor binds":
        assert (got["std"] == floor).all()
    if c["name"][0] == "floor idle":
        assert (got["std"] > floor).all()
        assert C.bits_equal(got["std"], c["std_prev"][:, [min(ts + 1, sp - 1) for ts in range(steps)]])
    if c["name"][0] == "nan std":
        assert (got["std"][:, steps - 1, 1] == floor).all() and not np.isnan(got["std"]).any()
        assert np.isnan(got["mean"][0, steps - 1, 3]) and np.isnan(got["warm"][steps - 1, 0, :, 3]).all()
    if c["name"][0] == "clamp":
        assert (got["warm"] >= c["low"]).all() and (got["warm"] <= c["high"]).all()
        assert (got["warm"][..., 2] == np.float32(0.125)).all()


# ---------------------------------------------------------------------------------------------- the comparison
def _ulp(x):
    with np.errstate(invalid="ignore"):
        return np.spacing(np.abs(x.astype(np.float32))).astype(np.float64)


def _same(got, want):
    return (got == want) | (np.isnan(got) & np.isnan(want))


def compare_update(c, got, want):
    """Asserts what must be exact -- elite_idx, best_err, row 0 of seq_out, and with weighting = elites every output --
    and holds what passes through exp to the bound that follows from two fp64 results that agree to a few fp64 ulp
    before the one rounding: mean and std 1 fp32 ulp, seq_out ulp(mean) + |n| ulp(std) + ulp(result).  Returns (the
    elements of mean, std and seq_out that differ at all, the elements compared)."""
    name = c["name"]
    for o in ("elite_idx", "best_err"):
        assert C.bits_equal(got[o], want[o]), (name, o)
    assert C.bits_equal(got["seq_out"][:, :, 0], want["seq_out"][:, :, 0]), (name, "row 0")
    if c["weighting"] == ELITES:
        for o in ("mean", "std", "seq_out"):
            assert C.bits_equal(got[o], want[o]), (name, o, np.flatnonzero(~_same(got[o], want[o]).reshape(-1))[:8])
        return 0, sum(got[o].size for o in ("mean", "std", "seq_out"))
    differ = total = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for o in ("mean", "std"):
            near = np.abs(got[o].astype(np.float64) - want[o].astype(np.float64)) <= _ulp(want[o])
            assert (_same(got[o], want[o]) | near).all(), (name, o)
        n = np.abs(c["normal"].astype(np.float64))
        bound = (_ulp(want["mean"]).transpose(1, 0, 2)[:, :, None, :] + n * _ulp(want["std"]).transpose(1, 0, 2)[:, :, None, :]
                 + _ulp(want["seq_out"]))
        near = np.abs(got["seq_out"].astype(np.float64) - want["seq_out"].astype(np.float64)) <= bound
        assert (_same(got["seq_out"], want["seq_out"]) | near).all(), (name, "seq_out")
    for o in ("mean", "std", "seq_out"):
        differ += int((~_same(got[o], want[o])).sum())
        total += got[o].size
    return differ, total


def compare_warm(c, got, want):
    for o in WARM_OUTPUTS:
        assert C.bits_equal(got[o], want[o]), (c["name"], o, np.flatnonzero(~_same(got[o], want[o]).reshape(-1))[:8])


def check_limits(pair, got, got_elites):
    """limit_cases(): the hot case has the bits of the same call with weighting = elites, the cold one is the rank-0 row
    and the floor."""
    c, twin = pair
    if twin is not None:
        for o in UPDATE_OUTPUTS:
            assert C.bits_equal(got[o], got_elites[o]), (c["name"], o)
    else:
        top = got["elite_idx"][:, 0]
        th, b_n = c["seq_in"].shape[:2]
        assert C.bits_equal(got["mean"], np.stack([c["seq_in"][:, b, top[b]] for b in range(b_n)]))
        assert (got["std"] == np.float32(c["min_std"])).all()


# ---------------------------------------------------------------------------------------------- the host driver
DRIVER_SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_drivers", "plan_warm_main.hip")


def build_driver():
    """The program of tests/host_drivers/plan_warm_main.hip -- the library's source and the body plan_warm.inc behind a
    main of its own --, compiled by host_driver.build itself: its one command line, its sanitizers, its check of the
    linked runtime.  build() compiles host_driver.SOURCE and keeps one program per value of `sanitize`, any true value
    meaning "sanitized": this program is the entry "plan_warm_main".  Returns its path, for host_driver.run(..., exe=)."""
    import host_driver
    keep = host_driver.SOURCE
    host_driver.SOURCE = DRIVER_SOURCE
    try:
        return host_driver.build(sanitize="plan_warm_main")
    finally:
        host_driver.SOURCE = keep


def pack(updates, warms):
    """IN of plan_warm.inc: int32 update cases; per case 7 int32 (B, R, E, Th, weighting, smooth, first), 3 floats
    (momentum, min_std, temperature), low[4], high[4], err [B,R], seq_in and normal [Th,B,R,4], mean and std [B,Th,4],
    best_err [B]; then int32 warm cases; per case 4 int32 (B, W, steps_prev, steps), 1 float (warm_std), low[4], high[4],
    mean_prev and std_prev [B,steps_prev,4], normal [steps,B,W,4]."""
    blob = [struct.pack("<i", len(updates))]
    for c in updates:
        th, b, r, _ = c["seq_in"].shape
        blob.append(struct.pack("<7i3f", b, r, c["elites"], th, c["weighting"], c["smooth"], c["first"], c["momentum"],
                                c["min_std"], c["temperature"]))
        for key in ("low", "high", "err", "seq_in", "normal", "mean", "std", "best_err"):
            blob.append(np.ascontiguousarray(c[key], np.float32).tobytes())
    blob.append(struct.pack("<i", len(warms)))
    for c in warms:
        steps, b, w, _ = c["normal"].shape
        blob.append(struct.pack("<4if", b, w, c["mean_prev"].shape[1], steps, c["warm_std"]))
        for key in ("low", "high", "mean_prev", "std_prev", "normal"):
            blob.append(np.ascontiguousarray(c[key], np.float32).tobytes())
    return b"".join(blob)


def unpack(updates, warms, report):
    """OUT: per update case mean, std [B,Th,4], seq_out [Th,B,R,4], best_err [B], elite_idx [B,E] int32; per warm case
    mean, std [B,steps,4], warm [steps,B,W,4]."""
    off = 0

    def take(shape, dt):
        nonlocal off
        n = int(np.prod(shape))
        a = np.frombuffer(report, dt, n, off).reshape(shape)
        off += 4 * n
        return a
    got_u, got_w = [], []
    for c in updates:
        th, b, r, _ = c["seq_in"].shape
        got_u.append({"mean": take((b, th, 4), np.float32), "std": take((b, th, 4), np.float32),
                      "seq_out": take((th, b, r, 4), np.float32), "best_err": take((b,), np.float32),
                      "elite_idx": take((b, c["elites"]), np.int32)})
    for c in warms:
        steps, b, w, _ = c["normal"].shape
        got_w.append({"mean": take((b, steps, 4), np.float32), "std": take((b, steps, 4), np.float32),
                      "warm": take((steps, b, w, 4), np.float32)})
    assert off == len(report), (off, len(report))
    return got_u, got_w


# ---------------------------------------------------------------------------------------------- refused arguments
def refused_update(lib, **over):
    """ndp_plan_update with made-up, 16-byte aligned addresses and exactly one refused argument (an accepted call would
    launch)."""
    a = dict(err=0x1000, seq_in=0x2000, normal=0x3000, b=2, r=8, th=3, e=2, weighting=MPPI, temperature=0.1, smooth=1,
             first=1, momentum=0.1, min_std=0.05, low=[-1.0] * 4, high=[1.0] * 4, mean=0x4000, std=0x5000, seq_out=0x6000,
             best=0x7000, idx=0x8000)
    a.update(over)
    low = None if a["low"] is None else (ctypes.c_float * 4)(*a["low"])
    high = None if a["high"] is None else (ctypes.c_float * 4)(*a["high"])
    return lib.ndp_plan_update(a["err"], a["seq_in"], a["normal"], a["b"], a["r"], a["th"], a["e"], a["weighting"],
                               a["temperature"], a["smooth"], a["first"], a["momentum"], a["min_std"], low, high, a["mean"],
                               a["std"], a["seq_out"], a["best"], a["idx"], None)


REFUSED_UPDATE = [{"weighting": 2}, {"weighting": -1}, {"temperature": 0.0}, {"temperature": -0.1},
                  {"temperature": float("inf")}, {"temperature": float("nan")}, {"smooth": 2}, {"smooth": -1}, {"first": 2},
                  {"err": None}, {"mean": None}, {"low": None}, {"b": 0}, {"r": 1}, {"r": 257}, {"e": 9}, {"th": 33},
                  {"momentum": 1.0}, {"min_std": -1.0}, {"high": [1, float("nan"), 1, 1]}, {"seq_out": 0x2000},
                  {"seq_out": 0x3000}, {"normal": 0x3008}, {"seq_out": 0x600c}]


def refused_warm(lib, **over):
    """ndp_plan_warm likewise."""
    a = dict(mean_prev=0x1000, std_prev=0x2000, normal=0x3000, b=2, w=2, sp=3, steps=3, warm_std=0.05, low=[-1.0] * 4,
             high=[1.0] * 4, mean=0x4000, std=0x5000, warm=0x6000)
    a.update(over)
    low = None if a["low"] is None else (ctypes.c_float * 4)(*a["low"])
    high = None if a["high"] is None else (ctypes.c_float * 4)(*a["high"])
    return lib.ndp_plan_warm(a["mean_prev"], a["std_prev"], a["normal"], a["b"], a["w"], a["sp"], a["steps"], a["warm_std"],
                             low, high, a["mean"], a["std"], a["warm"], None)


REFUSED_WARM = [{"mean_prev": None}, {"std_prev": None}, {"normal": None}, {"low": None}, {"high": None}, {"mean": None},
                {"std": None}, {"warm": None}, {"mean_prev": 0x1004}, {"std_prev": 0x2008}, {"normal": 0x300c},
                {"mean": 0x4004}, {"std": 0x5008}, {"warm": 0x6004}, {"steps": 4}, {"steps": 0}, {"sp": 33, "steps": 33},
                {"sp": 0, "steps": 0}, {"w": 0}, {"w": 256}, {"b": 0}, {"b": 65536}, {"warm_std": -0.5},
                {"warm_std": float("nan")}, {"warm_std": float("inf")}, {"low": [-1, -1, 2, -1]}, {"mean": 0x1000},
                {"std": 0x2000}, {"warm": 0x3000}, {"mean": 0x2000}, {"warm": 0x1000}, {"std": 0x4000}]


# ---------------------------------------------------------------------------------------------- the planner's calls
class RecordingWarmModels(C.RecordingModels):
    """plan_common.RecordingModels with the two new calls, computed by the restatements above:
      plan_update (Th, B, R, smooth, first)   plan_warm (steps, B, W, steps_prev)
    `forward` also records, as ("forward_rows", ...), how the action rows it was given relate to the last generate call
    and the last plan_warm call (see tests/test_plan_warm.py)."""

    def __init__(self):
        super().__init__()
        self.warm = self.generated = None
        self.forward_actions = []

    def generate(self, code, noise, code_rep=1, out=None):
        out = super().generate(code, noise, code_rep, out)
        self.generated = out.clone()
        return out

    def forward(self, state, actions):
        self.forward_actions.append(actions.clone())
        return super().forward(state, actions)

    def _case(self, err, seq_in, normal, settings, mean, std, best_err):
        th, b, r = (int(v) for v in seq_in.shape[:3])
        return {"err": err.numpy(), "seq_in": seq_in.numpy(), "normal": normal.reshape(th, b, r, 4).numpy(),
                "elites": settings.elite_count(r), "momentum": settings.momentum, "min_std": settings.min_std,
                "low": np.float32(settings.low), "high": np.float32(settings.high), "mean": mean.numpy(), "std": std.numpy(),
                "best_err": best_err.numpy()}

    def plan_update(self, err, seq_in, normal, settings, smooth, first, mean, std, seq_out, best_err, elite_idx=None):
        th, b, r = (int(v) for v in seq_in.shape[:3])
        self.calls.append(("plan_update", th, b, r, bool(smooth), bool(first)))
        c = self._case(err, seq_in, normal, settings, mean, std, best_err)
        c.update(weighting=("elites", "mppi").index(settings.weighting), temperature=settings.temperature or 0.0,
                 smooth=int(bool(smooth)), first=int(bool(first)))
        got = plan_update(c)
        for dst, key in ((mean, "mean"), (std, "std"), (seq_out, "seq_out"), (best_err, "best_err")):
            dst.copy_(torch.from_numpy(got[key]))

    def plan_warm(self, mean_prev, std_prev, normal, settings, mean, std, warm):
        steps, b, w = (int(v) for v in warm.shape[:3])
        self.calls.append(("plan_warm", steps, b, w, int(mean_prev.shape[1])))
        got = plan_warm({"mean_prev": mean_prev.numpy(), "std_prev": std_prev.numpy(),
                         "normal": normal.reshape(steps, b, w, 4).numpy(), "warm_std": settings.carried_floor(),
                         "low": np.float32(settings.low), "high": np.float32(settings.high)})
        for dst, key in ((mean, "mean"), (std, "std"), (warm, "warm")):
            dst.copy_(torch.from_numpy(got[key]))
        self.warm = warm.clone()
