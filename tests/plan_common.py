"""What the tests of the planner's cross-entropy refinement share (tests/test_plan_cem_host.py on the CPU,
tests/test_gpu_plan_cem.py on the GPU): the plain numpy restatement of ndp_plan_cem_update as include/ndp.h states it,
the fp64 restatement of ndp_normal_noise's Box-Muller, the cases, and the packing for
tests/host_drivers/plan_cem.inc (a body of tests/host_driver.py's program); and `RecordingModels`, the stand-in for
evaluation.EvalModels on which tests/test_planner_calls.py reads the planner's call sequence on the CPU."""
import ctypes
import struct

import numpy as np
import torch

# (B, R, E, Th): the smallest, a few rows, R across a wave, the limits with E = R
SHAPES = ((1, 2, 1, 1), (3, 5, 2, 3), (2, 65, 16, 4), (1, 256, 256, 32))
OUTPUTS = ("mean", "std", "seq_out", "best_err", "elite_idx")


# ---------------------------------------------------------------------------------------------- the restatement
def rank_order(e):
    """Rows in rank order: numbers before NaNs, smaller before larger, the index among equals (-0.0 == 0.0)."""
    return sorted(range(len(e)), key=lambda i: (1, 0.0, i) if np.isnan(e[i]) else (0, float(e[i]), i))


def cem_update(c):
    """ndp_plan_cem_update on the case `c`: fp64 sums in rank order, np.sqrt, one rounding to fp32 per stored value."""
    err, seq, normal = c["err"], c["seq_in"], c["normal"]
    th, b_n, r, _ = seq.shape
    e_n, first = c["elites"], c["first"]
    mo, least = np.float64(np.float32(c["momentum"])), np.float64(np.float32(c["min_std"]))
    low, high = c["low"].astype(np.float32), c["high"].astype(np.float32)
    mean, std, best = c["mean"].copy(), c["std"].copy(), c["best_err"].copy()
    out = np.empty_like(seq)
    elite_idx = np.full((b_n, e_n), -1, np.int32)
    for b in range(b_n):
        order = rank_order(err[b])
        ne = min(e_n, int((~np.isnan(err[b])).sum()))
        elite_idx[b, :ne] = order[:ne]
        if ne == 0:
            if first:
                mean[b], std[b] = 0.0, np.float32(c["min_std"])
        else:
            total = np.zeros((th, 4), np.float64)
            for k in order[:ne]:
                total = total + seq[:, b, k, :].astype(np.float64)
            m = total / np.float64(ne)
            dev = np.zeros((th, 4), np.float64)
            for k in order[:ne]:
                d = seq[:, b, k, :].astype(np.float64) - m
                dev = dev + d * d
            s = np.sqrt(dev / np.float64(ne))
            if not first:
                keep = np.float64(1.0) - mo
                m = mo * mean[b].astype(np.float64) + keep * m
                s = mo * std[b].astype(np.float64) + keep * s
            with np.errstate(invalid="ignore"):
                s = np.where(s > least, s, least)
            mean[b], std[b] = m.astype(np.float32), s.astype(np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            v = (std[b].astype(np.float64)[:, None, :] * normal[:, b].astype(np.float64)
                 + mean[b].astype(np.float64)[:, None, :]).astype(np.float32)
            v = np.where(np.isnan(v), v, np.minimum(np.maximum(v, low), high))
        out[:, b] = v
        out[:, b, 0] = seq[:, b, order[0]]
        e0 = err[b, order[0]]
        if first:
            best[b] = e0
        elif e0 < best[b] or np.isnan(best[b]):
            best[b] = e0
    return {"mean": mean, "std": std, "seq_out": out, "best_err": best, "elite_idx": elite_idx}


def box_muller(u):
    """ndp_normal_noise's definition in fp64 on the fp32 uniforms `u` (an even count): pair j = (u[2j], u[2j+1])."""
    u = np.asarray(u, np.float64).reshape(-1, 2)
    r = np.sqrt(-2.0 * np.log(1.0 - u[:, 0]))
    ang = 2.0 * np.pi * u[:, 1]
    return np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1).reshape(-1)


# ---------------------------------------------------------------------------------------------- the cases
def _case(name, shape, seed, first, momentum=0.1, min_std=0.05, low=-1.0, high=1.0, spread=0.4, with_idx=True):
    b, r, e, th = shape
    g = np.random.default_rng(seed)
    c = {"name": name, "elites": e, "first": int(first), "momentum": momentum, "min_std": min_std, "with_idx": with_idx,
         "low": np.full(4, low, np.float32), "high": np.full(4, high, np.float32),
         "err": g.random((b, r), dtype=np.float32) + np.float32(0.01),
         "seq_in": (spread * g.standard_normal((th, b, r, 4))).astype(np.float32),
         "normal": g.standard_normal((th, b, r, 4)).astype(np.float32),
         "mean": (0.2 * g.standard_normal((b, th, 4))).astype(np.float32),
         "std": (0.1 + g.random((b, th, 4))).astype(np.float32),
         "best_err": (g.random(b) * 0.5).astype(np.float32)}
    return c


def cases():
    out = []
    for i, shape in enumerate(SHAPES):
        out.append(_case(("shape", shape, "first"), shape, 10 + i, True))
        out.append(_case(("shape", shape, "smoothed"), shape, 20 + i, False))
    edge = SHAPES[1]                                                  # B = 3, R = 5, E = 2, Th = 3
    for first in (True, False):
        c = _case(("edges", first), edge, 30 + first, first)
        c["err"][0, 1] = c["err"][0, 3] = np.float32(0.001)           # trajectory 0: a tie for the minimum, row 1 wins
        c["err"][0, 4] = c["err"][0, 2]                               # ... and one further down
        c["err"][1] = np.nan                                          # trajectory 1: one number, fewer than E
        c["err"][1, 3] = np.float32(0.7)
        c["err"][2] = np.nan                                          # trajectory 2: nothing to fit
        c["best_err"][0] = np.nan                                     # a NaN minimum is replaced by a number,
        c["best_err"][1] = np.float32(0.1)                            # a smaller one stays,
        c["best_err"][2] = np.float32(0.2)                            # and a NaN replaces nothing
        out.append(c)
    out.append(_case(("clamp",), SHAPES[2], 40, True, low=-0.25, high=0.3, spread=1.0))
    c = _case(("clamp", "per component"), edge, 41, False, spread=1.0)
    c["low"], c["high"] = np.float32([-0.5, -1.0, 0.125, -2.0]), np.float32([0.5, -0.75, 0.125, 2.0])
    out.append(c)
    out.append(_case(("min_std binds",), SHAPES[2], 42, True, min_std=0.5, spread=0.01))
    out.append(_case(("min_std binds", "smoothed"), edge, 43, False, min_std=2.0, momentum=0.5))
    out.append(_case(("momentum 0",), edge, 44, False, momentum=0.0, min_std=0.0))
    c = _case(("one elite",), (2, 7, 1, 2), 45, True, min_std=0.125)   # E = 1: the deviation is 0, min_std alone
    out.append(c)
    c = _case(("inf inside",), edge, 46, True)
    c["normal"][2, 1, 3, 0] = np.inf                                  # an infinite draw is clamped
    c["err"][2, 0] = np.inf                                           # an infinite error ranks behind every finite one
    c["err"][2, 1] = np.nan                                           # ... and before a NaN
    out.append(c)
    out.append(_case(("no elite_idx",), edge, 47, True, with_idx=False))
    return out


def check_special(c, got):
    """What the edge cases must show, whatever computed `got`."""
    if c["name"][0] == "edges":
        assert got["elite_idx"].tolist() == [[1, 3], [3, -1], [-1, -1]]
        assert np.array_equal(got["seq_out"][:, 0, 0], c["seq_in"][:, 0, 1])
        assert np.array_equal(got["seq_out"][:, 2, 0], c["seq_in"][:, 2, 0])
        if c["first"]:
            # trajectory 1 has one elite: its own values and the floor
            assert np.array_equal(got["mean"][1], c["seq_in"][:, 1, 3])
            assert (got["std"][1] == np.float32(c["min_std"])).all()
            assert (got["mean"][2] == 0).all() and (got["std"][2] == np.float32(c["min_std"])).all()
            assert got["best_err"][0] == np.float32(0.001) and got["best_err"][1] == np.float32(0.7)
            assert np.isnan(got["best_err"][2])
        else:
            assert np.array_equal(got["mean"][2], c["mean"][2]) and np.array_equal(got["std"][2], c["std"][2])
            assert got["best_err"].tolist() == [np.float32(0.001), np.float32(0.1), np.float32(0.2)]
    if c["name"][0] == "clamp":
        rest = got["seq_out"][:, :, 1:]
        assert (rest >= c["low"]).all() and (rest <= c["high"]).all()
        assert (rest == c["low"]).any() and (rest == c["high"]).any()
    if c["name"][0] == "min_std binds":
        assert (got["std"] == np.float32(c["min_std"])).all()
    if c["name"][0] == "one elite":
        assert (got["std"] == np.float32(0.125)).all()
        assert np.array_equal(got["mean"], np.moveaxis(c["seq_in"][:, np.arange(2), got["elite_idx"][:, 0]], 0, 1))
    if c["name"][0] == "inf inside":
        assert got["seq_out"][2, 1, 3, 0] == 1.0                      # std * inf + mean, clamped to high
        assert 0 not in got["elite_idx"][2].tolist() and 1 not in got["elite_idx"][2].tolist()


# ---------------------------------------------------------------------------------------------- the host driver
def pack(case_list):
    """IN of plan_cem.inc: int32 cases; per case 6 int32 (B, R, E, Th, first, elite_idx wanted), 2 floats (momentum,
    min_std), low[4], high[4], err [B,R], seq_in and normal [Th,B,R,4], mean and std [B,Th,4], best_err [B]."""
    blob = [struct.pack("<i", len(case_list))]
    for c in case_list:
        th, b, r, _ = c["seq_in"].shape
        blob.append(struct.pack("<6i2f", b, r, c["elites"], th, c["first"], int(c["with_idx"]), c["momentum"], c["min_std"]))
        for key in ("low", "high", "err", "seq_in", "normal", "mean", "std", "best_err"):
            blob.append(np.ascontiguousarray(c[key], np.float32).tobytes())
    return b"".join(blob)


def unpack(case_list, report):
    """OUT: per case mean, std [B,Th,4], seq_out [Th,B,R,4], best_err [B], elite_idx [B,E] int32 (-7 where not wanted)."""
    out, off = [], 0
    for c in case_list:
        th, b, r, _ = c["seq_in"].shape
        got = {}
        for key, shape, dt in (("mean", (b, th, 4), np.float32), ("std", (b, th, 4), np.float32),
                               ("seq_out", (th, b, r, 4), np.float32), ("best_err", (b,), np.float32),
                               ("elite_idx", (b, c["elites"]), np.int32)):
            n = int(np.prod(shape))
            got[key] = np.frombuffer(report, dt, n, off).reshape(shape)
            off += 4 * n
        out.append(got)
    assert off == len(report), (off, len(report))
    return out


def bits_equal(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------- refused arguments
def refused_call(lib, **over):
    """ndp_plan_cem_update with made-up, 16-byte aligned addresses: an accepted call would launch, so every call made
    here carries exactly one refused argument."""
    a = dict(err=0x1000, seq_in=0x2000, normal=0x3000, b=2, r=8, th=3, e=2, first=1, momentum=0.1, min_std=0.05,
             low=[-1.0] * 4, high=[1.0] * 4, mean=0x4000, std=0x5000, seq_out=0x6000, best=0x7000, idx=0x8000)
    a.update(over)
    low = None if a["low"] is None else (ctypes.c_float * 4)(*a["low"])
    high = None if a["high"] is None else (ctypes.c_float * 4)(*a["high"])
    return lib.ndp_plan_cem_update(a["err"], a["seq_in"], a["normal"], a["b"], a["r"], a["th"], a["e"], a["first"],
                                   a["momentum"], a["min_std"], low, high, a["mean"], a["std"], a["seq_out"], a["best"],
                                   a["idx"], None)


REFUSED = [{"err": None}, {"seq_in": None}, {"normal": None}, {"low": None}, {"high": None}, {"mean": None}, {"std": None},
           {"seq_out": None}, {"best": None}, {"b": 0}, {"b": 65536}, {"r": 1}, {"r": 257}, {"e": 0}, {"e": 9}, {"th": 0},
           {"th": 33}, {"first": 2}, {"momentum": 1.0}, {"momentum": -0.5}, {"momentum": float("nan")}, {"min_std": -1.0},
           {"min_std": float("nan")}, {"low": [-1, -1, 2, -1]}, {"high": [1, float("nan"), 1, 1]}, {"seq_out": 0x2000},
           {"seq_out": 0x3000}, {"seq_in": 0x2004}, {"normal": 0x3008}, {"seq_out": 0x600c}]


# ---------------------------------------------------------------------------------------------- the planner's calls
class RecordingModels:
    """evaluation.EvalModels' calls as small deterministic torch functions on the CPU; every call appends
    (name, sizes...) to `calls`:
      images (n)   encode (n)   g_input (state rows, state_rep, goal rows, goal_rep, rows)   generate (rows)
      forward (n)   mse (pairs)   score_select (B, R, pred0 given, pred_out given, forced given)   uniform (n)
      normal (n)   cem_update (Th, B, R, first)"""
    VALUES = 3 * 128 * 128

    def __init__(self):
        self.device, self.noise_dim, self.calls = torch.device("cpu"), 2, []

    def images(self, frames):
        self.calls.append(("images", int(frames.shape[0])))
        return frames.float().contiguous()

    def encode(self, images):
        n = int(images.shape[0])
        self.calls.append(("encode", n))
        return images.reshape(n, 128, -1).mean(dim=2) * 8

    def g_input(self, state_code, state_rep, goal_code, goal_rep, rows):
        self.calls.append(("g_input", int(state_code.shape[0]), int(state_rep), int(goal_code.shape[0]), int(goal_rep), int(rows)))
        return torch.cat([state_code.repeat_interleave(int(state_rep), 0)[:rows],
                          goal_code.repeat_interleave(int(goal_rep), 0)[:rows]], dim=1)

    def generate(self, code, noise, code_rep=1, out=None):
        m = int(code.shape[0]) * int(code_rep)
        self.calls.append(("generate", m))
        act = torch.tanh(code.repeat_interleave(int(code_rep), 0).view(m, 4, 64).sum(dim=2)
                         + 3 * noise.reshape(m, self.noise_dim).repeat(1, 2) - 1.5)
        if out is None:
            return act
        out.view(m, 4).copy_(act)
        return out

    def forward(self, state, actions):
        n = int(state.shape[0])
        self.calls.append(("forward", n))
        a = actions.reshape(n, 4)
        return 0.9 * state + 0.1 * a[:, :3].reshape(n, 3, 1, 1) * (1 + a[:, 3]).reshape(n, 1, 1, 1)

    def mse(self, a, b, n_pairs, values, group=1, a_idx=None, b_idx=None, out=None, acc=None):
        n_pairs, group = int(n_pairs), int(group)
        self.calls.append(("mse", n_pairs))
        a, b = a.reshape(-1, int(values)), b.reshape(-1, int(values))
        a = a[:n_pairs] if a_idx is None else a[a_idx.long()]
        b = b[:n_pairs] if b_idx is None else b[b_idx.long()]
        res = ((a - b) ** 2).view(n_pairs // group, -1).mean(dim=1)
        if out is None:
            out = torch.empty(n_pairs // group)
        out.copy_(res)
        if acc is not None:
            acc.add_(res)
        return out

    def score_select(self, pred, n_traj, rollouts, target, actions0, pred0, forced, err, choice, action_out, pred_out):
        b, r = int(n_traj), int(rollouts)
        self.calls.append(("score_select", b, r, pred0 is not None, pred_out is not None, forced is not None))
        err.copy_(((pred.reshape(b, r, -1) - target.reshape(b, 1, -1)) ** 2).mean(dim=2))
        for i in range(b):
            best, pick = 10000000000.0, 0                             # the rollout rule: the first strict minimum
            for k in range(r):
                if err[i, k] < best:
                    best, pick = float(err[i, k]), k
            pick = pick if forced is None else int(forced[i])
            choice[i] = pick
            action_out[i] = actions0.reshape(b, r, 4)[i, pick]
            if pred_out is not None:
                pred_out[i] = pred0.reshape(b, r, *pred_out.shape[1:])[i, pick]

    def uniform(self, n, seed):
        self.calls.append(("uniform", int(n)))
        return torch.rand(max(int(n), 1), generator=torch.Generator().manual_seed(int(seed)))

    def normal(self, n, seed):
        self.calls.append(("normal", int(n)))
        return torch.randn(max(int(n), 1), generator=torch.Generator().manual_seed(int(seed) + (1 << 32)))

    def cem_update(self, err, seq_in, normal, settings, first, mean, std, seq_out, best_err, elite_idx=None):
        th, b, r = (int(v) for v in seq_in.shape[:3])
        self.calls.append(("cem_update", th, b, r, bool(first)))
        got = cem_update({"err": err.numpy(), "seq_in": seq_in.numpy(), "normal": normal.reshape(th, b, r, 4).numpy(),
                          "elites": settings.elite_count(r), "first": int(bool(first)), "momentum": settings.momentum,
                          "min_std": settings.min_std, "low": np.float32(settings.low), "high": np.float32(settings.high),
                          "mean": mean.numpy(), "std": std.numpy(), "best_err": best_err.numpy()})
        for dst, key in ((mean, "mean"), (std, "std"), (seq_out, "seq_out"), (best_err, "best_err")):
            dst.copy_(torch.from_numpy(got[key]))
