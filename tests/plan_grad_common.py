"""What the tests of the planner's gradient stage share (tests/test_plan_grad_host.py and tests/test_plan_grad.py on the
CPU, tests/test_gpu_plan_grad.py on the GPU): the plain numpy restatements of ndp_plan_goal_grad, ndp_plan_grad_gather and
ndp_plan_grad_step as include/ndp.h states them, the cases, the build of the host-driver program of
tests/host_drivers/plan_grad_main.hip and the packing for its body plan_grad.inc, and the refused arguments."""
import ctypes
import os
import struct

import numpy as np

import plan_common as C

SGD, ADAM = 0, 1                                                      # NDP_PLAN_SGD, NDP_PLAN_ADAM
VALUES = 3 * 128 * 128
THREADS = 256
# (B, R, G, Th): the issue's smallest shapes -- R 4 and 5, G 1 and 2, Th 1..3, odd R with G = R // 2 -- and R across a wave
GATHER_SHAPES = ((2, 4, 1, 1), (2, 4, 2, 2), (2, 5, 1, 2), (2, 5, 2, 3), (3, 70, 35, 2))
GATHER_TAGS = ("plain", "ties", "nan", "inf", "all nan")
STEP_SHAPES = ((2, 4, 1, 1), (2, 4, 2, 2), (2, 5, 2, 3), (70, 8, 4, 2))      # the last: more than one block of rows
STEP_TAGS = ("sgd", "adam t1", "adam t3", "nan grad", "inf grad", "zero grad", "clamp", "no dst")
# (n rows, goals, rows_per_goal, in place): rows_per_goal 1 and G, a last goal with fewer rows, one goal for every row
# (rows_per_goal above n), and more goals than the 8 residues the rows are dealt to
GOAL_SHAPES = ((2, 2, 1, 0), (4, 2, 2, 0), (4, 2, 2, 1), (3, 2, 2, 1), (3, 1, 5, 0), (19, 10, 2, 0))
GOAL_TAGS = ("plain", "nan")


# ---------------------------------------------------------------------------------------------- fused multiply-add
def fma_exact(a, b, c):
    """fma(a, b, c) of three Python floats by integer arithmetic: the exact a * b + c, rounded once (CPython's int / int
    is correctly rounded).  The slow reference of `fma` below."""
    if not all(np.isfinite(x) for x in (a, b, c)):
        return a * b + c
    (na, da), (nb, db), (nc, dc) = (float(x).as_integer_ratio() for x in (a, b, c))
    num, den = na * nb * dc + nc * da * db, da * db * dc
    if num == 0:
        return a * b + c                                             # the sign of a zero: every rounding gives it
    return num / den


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker / Veltkamp; no overflow or underflow at the magnitudes of the tests)."""
    p = a * b
    split = np.float64(134217729.0)                                   # 2^27 + 1

    def halves(x):
        t = split * x
        hi = t - (t - x)
        return hi, x - hi
    ah, al = halves(a)
    bh, bl = halves(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _round_odd_sum(a, b):
    """a + b rounded to odd: exact sums stay, an inexact one takes the neighbour whose last mantissa bit is 1."""
    s, e = _two_sum(a, b)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(e > 0, np.inf, -np.inf)
    return np.where((e != 0) & even, np.nextafter(s, toward), s)


def fma(a, b, c):
    """fma(a, b, c) on fp64 arrays, one rounding (Boldo and Melquiond 2008: the product exactly as two doubles, its head
    added exactly to c, the two tails summed with rounding to odd, one last rounding to nearest).  Elements that are not
    finite take a * b + c, which has the same NaN or infinity."""
    a, b, c = (np.asarray(x, np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        uh, ul = _two_prod(a, b)
        th, tl = _two_sum(c, uh)
        out = th + _round_odd_sum(tl, ul)
        plain = a * b + c
    return np.where(np.isfinite(plain) & np.isfinite(uh), out, plain)


# ---------------------------------------------------------------------------------------------- the restatements
def goal_grad(c):
    """ndp_plan_goal_grad on the case `c` (pred [n,V], goal [n_goal,V], rows_per_goal): err [n] by the documented order --
    thread t of 256 folds elements t, t + 256, ... with one fused multiply-add each, then the tree, then the mean rounded
    to fp32 -- and d_pred = (pred - goal) * c in fp32."""
    pred, goal, rpg = c["pred"], c["goal"], c["rows_per_goal"]
    n = pred.shape[0]
    tgt = goal[np.arange(n) // rpg]
    with np.errstate(invalid="ignore"):
        d_pred = ((pred - tgt).astype(np.float32) * np.float32(2.0 / VALUES)).astype(np.float32)
        d = (pred.astype(np.float64) - tgt.astype(np.float64)).reshape(n, VALUES // THREADS, THREADS)
        s = np.zeros((n, THREADS), np.float64)
        for k in range(VALUES // THREADS):
            s = fma(d[:, k], d[:, k], s)
        w = THREADS // 2
        while w > 0:
            s = s.copy()
            s[:, :w] = s[:, :w] + s[:, w:2 * w]
            w //= 2
        err = (s[:, 0] / np.float64(VALUES)).astype(np.float32)
    return {"err": err, "d_pred": d_pred}


def grad_gather(c):
    """ndp_plan_grad_gather: src = the G first rows in rank order, dst = the G last, seq_g = the source rows, m = v = 0."""
    err, seq, g = c["err"], c["seq"], c["rows"]
    th, b_n, r, _ = seq.shape
    src, dst = np.empty((b_n, g), np.int32), np.empty((b_n, g), np.int32)
    seq_g = np.empty((th, b_n, g, 4), np.float32)
    for b in range(b_n):
        order = C.rank_order(err[b])
        src[b], dst[b] = order[:g], order[r - g:]
        seq_g[:, b] = seq[:, b, order[:g]]
    return {"src": src, "dst": dst, "seq_g": seq_g, "m": np.zeros_like(seq_g), "v": np.zeros_like(seq_g)}


def pow_steps(beta, t):
    p = np.float64(1.0)
    for _ in range(t):
        p = p * np.float64(beta)
    return p


def _clamp(v, low, high):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v), v, np.minimum(np.maximum(v, low), high))


def grad_step(c):
    """ndp_plan_grad_step on the case `c`: fp64 from the fp32 inputs, every operation rounded on its own, one rounding to
    fp32 per stored value, the clamp, rows with a gradient component that is not finite left alone, the copies to
    curve_out and to the rows dst of seq_full."""
    grad, seq_g = c["grad"], c["seq_g"]
    th, b_n, g_n, _ = seq_g.shape
    lr, b1, b2, eps = (np.float64(np.float32(c[k])) for k in ("lr", "beta1", "beta2", "eps"))
    low, high = c["low"].astype(np.float32), c["high"].astype(np.float32)
    a, g = seq_g.astype(np.float64), grad.astype(np.float64)
    m, v = c["m"].copy(), c["v"].copy()
    with np.errstate(all="ignore"):
        if c["optimizer"] == ADAM:
            c1, c2 = np.float64(1.0) - pow_steps(b1, c["t"]), np.float64(1.0) - pow_steps(b2, c["t"])
            mn = b1 * m.astype(np.float64) + (np.float64(1.0) - b1) * g
            vn = b2 * v.astype(np.float64) + (np.float64(1.0) - b2) * (g * g)
            nxt = a - (lr * (mn / c1)) / (np.sqrt(vn / c2) + eps)
        else:
            mn, vn = m.astype(np.float64), v.astype(np.float64)
            nxt = a - lr * g
        moved = _clamp(nxt.astype(np.float32), low, high).astype(np.float32)
    ok = np.isfinite(grad).all(axis=(0, 3))                            # [B,G]: every component of the row
    out = np.where(ok[None, :, :, None], moved, seq_g)
    if c["optimizer"] == ADAM:
        m = np.where(ok[None, :, :, None], mn.astype(np.float32), m)
        v = np.where(ok[None, :, :, None], vn.astype(np.float32), v)
    res = {"seq_g": out, "m": m, "v": v, "curve": c["err_g"].copy()}
    if c["dst"] is not None:
        full = c["seq_full"].copy()
        for b in range(b_n):
            for k in range(g_n):
                full[:, b, c["dst"][b, k]] = out[:, b, k]
        res["seq_full"] = full
    return res


# ---------------------------------------------------------------------------------------------- the cases
def goal_cases():
    out = []
    for si, shape in enumerate(GOAL_SHAPES):
        n, n_goal, rpg, inplace = shape
        for k, tag in enumerate(GOAL_TAGS):
            g = np.random.default_rng(5000 + 100 * n + 10 * rpg + k)  # in place or apart: the same operands
            c = {"name": (tag, shape), "rows_per_goal": rpg, "inplace": inplace,
                 "pred": (g.random((n, VALUES)) * 2.4 - 1.2).astype(np.float32),
                 "goal": (g.random((n_goal, VALUES)) * 2.0 - 1.0).astype(np.float32)}
            c["pred"][0, ::97] = c["goal"][0, ::97]                   # exact zeros among the differences
            c["pred"][n - 1, 5::1031] *= np.float32(1e-6)             # operands of unlike magnitude
            if tag == "nan":
                c["pred"][n - 1, 12345] = np.nan                      # one NaN: that row's err, and that element of d_pred
                c["pred"][0, 777] = np.inf
            out.append(c)
    return out


def gather_cases():
    out = []
    for si, shape in enumerate(GATHER_SHAPES):
        b, r, g_n, th = shape
        for k, tag in enumerate(GATHER_TAGS):
            g = np.random.default_rng(6000 + 10 * si + k)
            c = {"name": (tag, shape), "rows": g_n, "err": (0.05 + g.random((b, r))).astype(np.float32),
                 "seq": (0.4 * g.standard_normal((th, b, r, 4))).astype(np.float32)}
            if tag == "ties":
                c["err"][:, r - 1] = c["err"][:, 0] = c["err"].min(axis=1) * np.float32(0.5)     # the minimum twice
                c["err"][:, 1] = c["err"][:, 2] = c["err"].max(axis=1) * np.float32(2.0)         # the maximum twice
            if tag == "nan":
                c["err"][:, ::2] = np.nan                             # NaNs rank last, by index among themselves
            if tag == "inf":
                c["err"][:, 1:] = np.inf
                c["err"][b - 1, r - 1] = np.nan
            if tag == "all nan":
                c["err"][:] = np.nan
            out.append(c)
    return out


def _step_case(tag, shape, seed):
    b, r, g_n, th = shape
    g = np.random.default_rng(seed)
    c = {"name": (tag, shape), "optimizer": ADAM, "t": 1, "lr": 0.05, "beta1": 0.9, "beta2": 0.999, "eps": 1e-8,
         "low": np.full(4, -1.0, np.float32), "high": np.full(4, 1.0, np.float32), "rollouts": r,
         "grad": (0.3 * g.standard_normal((th, b, g_n, 4))).astype(np.float32),
         "seq_g": (0.4 * g.standard_normal((th, b, g_n, 4))).astype(np.float32),
         "m": np.zeros((th, b, g_n, 4), np.float32), "v": np.zeros((th, b, g_n, 4), np.float32),
         "err_g": g.random((b, g_n)).astype(np.float32),
         "seq_full": (0.4 * g.standard_normal((th, b, r, 4))).astype(np.float32),
         "dst": np.stack([g.permutation(r)[:g_n] for _ in range(b)]).astype(np.int32)}
    if tag == "sgd":
        c.update(optimizer=SGD, lr=0.5)
    if tag == "adam t3":
        c["t"] = 3
        c["m"] = (0.1 * g.standard_normal((th, b, g_n, 4))).astype(np.float32)
        c["v"] = (0.02 * g.random((th, b, g_n, 4))).astype(np.float32)
    if tag == "nan grad":
        c["grad"][th - 1, 0, 0, 2] = np.nan                           # row (0, 0) stays, every other row moves
    if tag == "inf grad":
        c.update(optimizer=SGD)
        c["grad"][0, b - 1, g_n - 1, 0] = -np.inf
    if tag == "zero grad":
        c["t"] = 3
        c["grad"][:, 0, 0] = 0.0                                      # Adam: 0 / (0 + eps) with zero moments, no NaN
        c["v"][:] = 0.0
    if tag == "clamp":
        c.update(optimizer=SGD, lr=4.0)                               # both bounds bind; one component has low == high
        c["low"], c["high"] = np.float32([-0.25, -1.0, 0.125, -2.0]), np.float32([0.3, -0.75, 0.125, 2.0])
    if tag == "no dst":
        c["dst"] = c["seq_full"] = None
    return c


def step_cases():
    return [_step_case(tag, shape, 7000 + 20 * si + k) for si, shape in enumerate(STEP_SHAPES)
            for k, tag in enumerate(STEP_TAGS)]


def check_step_special(c, got):
    tag, (b, r, g_n, th) = c["name"]
    if tag == "nan grad":
        assert C.bits_equal(got["seq_g"][:, 0, 0], c["seq_g"][:, 0, 0]) and C.bits_equal(got["m"][:, 0, 0], c["m"][:, 0, 0])
        if b * g_n > 1:
            assert not np.array_equal(got["seq_g"], c["seq_g"])
    if tag == "inf grad":
        assert C.bits_equal(got["seq_g"][:, b - 1, g_n - 1], c["seq_g"][:, b - 1, g_n - 1])
    if tag == "zero grad":
        assert C.bits_equal(got["seq_g"][:, 0, 0], _clamp(c["seq_g"][:, 0, 0], c["low"], c["high"]).astype(np.float32))
        assert np.isfinite(got["seq_g"]).all()
    if tag == "clamp":
        assert (got["seq_g"] >= c["low"]).all() and (got["seq_g"] <= c["high"]).all()
        assert (got["seq_g"] == c["low"]).any() and (got["seq_g"] == c["high"]).any()
        assert (got["seq_g"][..., 2] == np.float32(0.125)).all()
    if c["dst"] is not None:
        touched = np.zeros((b, r), bool)
        for i in range(b):
            touched[i, c["dst"][i]] = True
        assert C.bits_equal(got["seq_full"][:, ~touched], c["seq_full"][:, ~touched])       # every other row keeps its bits


def same(got, want):
    return (got == want) | (np.isnan(got) & np.isnan(want))


def compare(c, got, want, outputs):
    """Every output is bit-equal to the restatement (a NaN is a NaN: its payload is not compared)."""
    for o in outputs:
        assert got[o].shape == want[o].shape and got[o].dtype == want[o].dtype, (c["name"], o)
        ok = same(got[o], want[o]) if got[o].dtype.kind == "f" else got[o] == want[o]
        assert ok.all(), (c["name"], o, np.flatnonzero(~ok.reshape(-1))[:8])
        if got[o].dtype.kind == "f":
            keep = ~np.isnan(want[o])
            assert got[o][keep].tobytes() == want[o][keep].tobytes(), (c["name"], o, "the sign of a zero")


GOAL_OUTPUTS = ("err", "d_pred")
GATHER_OUTPUTS = ("src", "dst", "seq_g", "m", "v")


def step_outputs(c):
    return ("seq_g", "m", "v", "curve") + (("seq_full",) if c["dst"] is not None else ())


# ---------------------------------------------------------------------------------------------- the host driver
DRIVER_SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_drivers", "plan_grad_main.hip")


def build_driver():
    """The program of tests/host_drivers/plan_grad_main.hip -- the library's source and the body plan_grad.inc behind a
    main of its own --, compiled by host_driver.build itself: its one command line, its sanitizers, its check of the
    linked runtime (as plan_warm_common.build_driver).  Returns its path, for host_driver.run(..., exe=)."""
    import host_driver
    keep = host_driver.SOURCE
    host_driver.SOURCE = DRIVER_SOURCE
    try:
        return host_driver.build(sanitize="plan_grad_main")
    finally:
        host_driver.SOURCE = keep


def _f32(a):
    return np.ascontiguousarray(a, np.float32).tobytes()


def pack(goals, gathers, steps):
    """IN of plan_grad.inc: int32 goal cases; per case 4 int32 (n, n_goal, rows_per_goal, in place), pred [n,V], goal
    [n_goal,V]; int32 gather cases; per case 4 int32 (B, R, G, Th), err [B,R], seq [Th,B,R,4]; int32 step cases; per case 7
    int32 (B, R, G, Th, t, optimizer, dst given), 4 floats (lr, beta1, beta2, eps), low[4], high[4], grad, seq_g, m, v
    [Th,B,G,4], err_g [B,G], and with dst: dst [B,G] int32, seq_full [Th,B,R,4]."""
    blob = [struct.pack("<i", len(goals))]
    for c in goals:
        blob += [struct.pack("<4i", c["pred"].shape[0], c["goal"].shape[0], c["rows_per_goal"], c["inplace"]),
                 _f32(c["pred"]), _f32(c["goal"])]
    blob.append(struct.pack("<i", len(gathers)))
    for c in gathers:
        th, b, r, _ = c["seq"].shape
        blob += [struct.pack("<4i", b, r, c["rows"], th), _f32(c["err"]), _f32(c["seq"])]
    blob.append(struct.pack("<i", len(steps)))
    for c in steps:
        th, b, g_n, _ = c["seq_g"].shape
        blob.append(struct.pack("<7i4f", b, c["rollouts"], g_n, th, c["t"], c["optimizer"], int(c["dst"] is not None),
                                c["lr"], c["beta1"], c["beta2"], c["eps"]))
        blob += [_f32(c[k]) for k in ("low", "high", "grad", "seq_g", "m", "v", "err_g")]
        if c["dst"] is not None:
            blob += [np.ascontiguousarray(c["dst"], np.int32).tobytes(), _f32(c["seq_full"])]
    return b"".join(blob)


def unpack(goals, gathers, steps, report):
    """OUT: per goal case err [n], d_pred [n,V]; per gather case src, dst [B,G] int32, seq_g, m, v [Th,B,G,4]; per step
    case seq_g, m, v [Th,B,G,4], curve [B,G], and with dst seq_full [Th,B,R,4]."""
    off = 0

    def take(shape, dt=np.float32):
        nonlocal off
        n = int(np.prod(shape))
        a = np.frombuffer(report, dt, n, off).reshape(shape)
        off += 4 * n
        return a
    got = [], [], []
    for c in goals:
        n = c["pred"].shape[0]
        got[0].append({"err": take((n,)), "d_pred": take((n, VALUES))})
    for c in gathers:
        th, b, r, _ = c["seq"].shape
        small = (th, b, c["rows"], 4)
        got[1].append({"src": take((b, c["rows"]), np.int32), "dst": take((b, c["rows"]), np.int32), "seq_g": take(small),
                       "m": take(small), "v": take(small)})
    for c in steps:
        th, b, g_n, _ = c["seq_g"].shape
        one = {"seq_g": take(c["seq_g"].shape), "m": take(c["seq_g"].shape), "v": take(c["seq_g"].shape),
               "curve": take((b, g_n))}
        if c["dst"] is not None:
            one["seq_full"] = take(c["seq_full"].shape)
        got[2].append(one)
    assert off == len(report), (off, len(report))
    return got


# ---------------------------------------------------------------------------------------------- refused arguments
def refused_goal(lib, **over):
    """ndp_plan_goal_grad with made-up, 16-byte aligned addresses and exactly one refused argument (an accepted call would
    launch).  Two rows of 196,608 bytes lie at 0x100000 (pred), one goal at 0x200000, d_pred at 0x300000."""
    a = dict(pred=0x100000, n=2, goal=0x200000, n_goal=1, rpg=2, err=0x1000, d_pred=0x300000)
    a.update(over)
    return lib.ndp_plan_goal_grad(a["pred"], a["n"], a["goal"], a["n_goal"], a["rpg"], a["err"], a["d_pred"], None)


REFUSED_GOAL = [{"pred": None}, {"goal": None}, {"err": None}, {"d_pred": None}, {"n": 0}, {"n_goal": 0}, {"rpg": 0},
                {"rpg": 1}, {"pred": 0x100004}, {"goal": 0x200008}, {"d_pred": 0x30000c}, {"d_pred": 0x100010},
                {"d_pred": 0x100000 + 4 * VALUES}, {"d_pred": 0x200000}, {"d_pred": 0x200000 - 16}, {"err": 0x100000},
                {"err": 0x300040}]


def refused_gather(lib, **over):
    a = dict(err=0x1000, seq=0x2000, b=2, r=8, th=3, g=2, src=0x3000, dst=0x4000, seq_g=0x5000, m=0x6000, v=0x7000)
    a.update(over)
    return lib.ndp_plan_grad_gather(a["err"], a["seq"], a["b"], a["r"], a["th"], a["g"], a["src"], a["dst"], a["seq_g"], a["m"],
                                    a["v"], None)


REFUSED_GATHER = [{"err": None}, {"seq": None}, {"src": None}, {"dst": None}, {"seq_g": None}, {"m": None}, {"v": None},
                  {"b": 0}, {"b": 65536}, {"r": 1}, {"r": 257}, {"g": 0}, {"g": 5}, {"r": 5, "g": 3}, {"th": 0}, {"th": 33},
                  {"seq": 0x2004}, {"seq_g": 0x5008}, {"m": 0x600c}, {"v": 0x7004}, {"m": 0x5000}, {"v": 0x6000},
                  {"seq_g": 0x2000}, {"v": 0x2010}, {"dst": 0x3000}]


def refused_step(lib, **over):
    a = dict(grad=0x1000, seq_g=0x2000, m=0x3000, v=0x4000, err_g=0x5000, b=2, g=2, th=3, t=1, opt=ADAM, lr=0.05, beta1=0.9,
             beta2=0.999, eps=1e-8, low=[-1.0] * 4, high=[1.0] * 4, curve=0x6000, dst=0x7000, full=0x8000, r=8)
    a.update(over)
    low = None if a["low"] is None else (ctypes.c_float * 4)(*a["low"])
    high = None if a["high"] is None else (ctypes.c_float * 4)(*a["high"])
    return lib.ndp_plan_grad_step(a["grad"], a["seq_g"], a["m"], a["v"], a["err_g"], a["b"], a["g"], a["th"], a["t"], a["opt"],
                                  a["lr"], a["beta1"], a["beta2"], a["eps"], low, high, a["curve"], a["dst"], a["full"], a["r"],
                                  None)


REFUSED_STEP = [{"grad": None}, {"seq_g": None}, {"m": None}, {"v": None}, {"low": None}, {"high": None}, {"err_g": None},
                {"dst": None}, {"full": None}, {"b": 0}, {"b": 65536}, {"g": 0}, {"g": 129}, {"r": 3}, {"r": 257}, {"th": 0},
                {"th": 33}, {"t": 0}, {"t": 65536}, {"opt": 2}, {"opt": -1}, {"lr": 0.0}, {"lr": -1.0}, {"lr": float("inf")},
                {"lr": float("nan")}, {"beta1": 1.0}, {"beta2": -0.1}, {"eps": -1.0}, {"eps": float("nan")},
                {"high": [1, float("nan"), 1, 1]}, {"low": [-1, -1, 2, -1]}, {"grad": 0x1004}, {"seq_g": 0x2008},
                {"m": 0x300c}, {"v": 0x4004}, {"full": 0x8008}, {"seq_g": 0x1000}, {"m": 0x2000}, {"v": 0x3000},
                {"full": 0x2000}, {"full": 0x1010}]
