"""Times the push world (ndivplanning_amd/push_world.py) on the GPU: device events, warm-up,
medians of alternating repeats.  Prints one JSON line per measurement; nothing here is asserted by a test.

    python scripts/bench_push_world.py [--repeats 7] [--iters 200] [--skip-mpc] [--learn] [--out FILE]

  step       ndp_world_step_render at S = 128, n = 1, 64, 1,024, against the same definition in torch ops on the device
             (n environments, vectorised) and against the numpy restatement on the host plus the upload of its frames
             (n = 1 and 64): what an environment like tests/fake_push_env.py costs per step
  bandwidth  bytes of frames written over the fused launch's time, against the HBM peak
  generate   push_world.generate of 1,024 x 15 frames end to end, the JPEG encode and the bundle write included
  mpc        one closed_loop_mpc step at B = 16 (random-weight models) and the world's share of it
  --learn    one run, recorded and claiming nothing: 300 forward-model steps at batch 8 on generated push data, then
             forward_model_eval.evaluate's horizon_mse against persistence on held-out push trajectories
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ndivplanning_amd import push_world as P  # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s, the MI355X's specified HBM3E bandwidth
DEV = "cuda:0"
S = 128
_lines = []


def emit(**row):
    line = json.dumps(row)
    print(line, flush=True)
    _lines.append(line)


def device_ms(fn, iters):
    """Milliseconds per call of `fn` over `iters` back-to-back calls, by device events."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def host_ms(fn, iters):
    """Milliseconds per call by the host clock around work that ends in a device synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def alternate(candidates, repeats, iters, timer=device_ms):
    """{name: (median ms, min, max)}: every candidate warmed up, then `repeats` rounds that time each in turn."""
    for fn in candidates.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in candidates}
    for _ in range(repeats):
        for name, fn in candidates.items():
            samples[name].append(timer(fn, iters[name] if isinstance(iters, dict) else iters))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in samples.items()}


# ------------------------------------------------------------------------------------- the same definition in torch ops
def torch_step(state, actions):
    """push_world's step on device tensors, fp64 as the definition has it."""
    s = state.to(torch.float64)
    g, o = s[:, 0:3].clone(), s[:, 3:5].clone()
    a = torch.nan_to_num(actions[:, 0:3].to(torch.float64), nan=0.0).clamp(-1.0, 1.0)
    m = P.STEP * a / P.SUB
    lo = torch.tensor([P.X0, P.Y0, P.Z_MIN], dtype=torch.float64, device=s.device)
    hi = torch.tensor([P.X0 + P.SIDE, P.Y0 + P.SIDE, P.Z_MAX], dtype=torch.float64, device=s.device)
    o_lo, o_hi = lo[0:2] + P.R_O, hi[0:2] - P.R_O
    for _ in range(P.SUB):
        g = torch.minimum(torch.maximum(g + m, lo), hi)
        d = o - g[:, 0:2]
        r2 = (d * d).sum(dim=1)
        touch = (g[:, 2] < P.Z_CONTACT) & (r2 < P.R * P.R)
        f = P.R / r2.sqrt()
        apart = g[:, 0:2] + d * f[:, None]
        centred = torch.stack([g[:, 0] + P.R, g[:, 1]], dim=1)
        pushed = torch.minimum(torch.maximum(torch.where((r2 > 0)[:, None], apart, centred), o_lo), o_hi)
        o = torch.where(touch[:, None], pushed, o)
    out = state.clone()
    out[:, 0:3] = g.float()
    out[:, 3:5] = o.float()
    return out


class TorchRender:
    """push_world's render in torch ops: the 16-sample coverage of every pixel for every layer."""

    def __init__(self, size, device):
        self.size = size
        at = 16 * torch.arange(size, device=device)[:, None] + 2 + 4 * torch.arange(4, device=device)[None, :]
        self.at = at.reshape(-1).to(torch.int64)                                   # [4S] sample coordinates
        cell = torch.arange(size, device=device) // (size // 8)
        dark = ((cell[None, :] + cell[:, None]) & 1) * 12
        self.table = (torch.tensor([168, 160, 150], device=device)[None, None, :] - dark[:, :, None]).to(torch.int64)

    def q(self, v):
        return torch.round((v * (16.0 * self.size / P.SIDE)).clamp(-8192.0, 24576.0)).to(torch.int64)

    def cover(self, cx, cy, rin, rout):
        n, s = cx.shape[0], self.size
        dx2 = (self.at[None, :] - cx[:, None]) ** 2                                # [n,4S]
        dy2 = (self.at[None, :] - cy[:, None]) ** 2
        d2 = dy2[:, :, None] + dx2[:, None, :]                                     # [n,4S,4S]
        inside = (d2 >= (rin * rin)[:, None, None]) & (d2 <= (rout * rout)[:, None, None])
        return inside.view(n, s, 4, s, 4).sum(dim=(2, 4))

    @staticmethod
    def blend(c, fg, k):
        return (c * (16 - k[..., None]) + fg * k[..., None] + 8) >> 4

    def __call__(self, state):
        s = state.to(torch.float64)
        n = s.shape[0]
        lift = s[:, 2] - P.Z_MIN
        full = lambda v: torch.full((n,), v, dtype=torch.float64, device=s.device)  # noqa: E731
        zero = torch.zeros(n, dtype=torch.int64, device=s.device)
        colour = lambda rgb: torch.tensor(rgb, dtype=torch.int64, device=s.device)  # noqa: E731
        c = self.table[None].expand(n, -1, -1, -1)
        c = self.blend(c, colour((40, 200, 60)), self.cover(self.q(s[:, 6] - P.X0), self.q(s[:, 7] - P.Y0),
                                                            self.q(full(P.R_O - 0.008)), self.q(full(P.R_O))))
        c = self.blend(c, (c * 10 + 8) >> 4, self.cover(self.q(s[:, 0] + 0.6 * lift - P.X0), self.q(s[:, 1] + 0.6 * lift - P.Y0),
                                                        zero, self.q(full(P.R_G))))
        c = self.blend(c, colour((20, 20, 235)), self.cover(self.q(s[:, 3] - P.X0), self.q(s[:, 4] - P.Y0), zero,
                                                            self.q(full(P.R_O))))
        c = self.blend(c, colour((250, 245, 10)), self.cover(self.q(s[:, 0] - P.X0), self.q(s[:, 1] - P.Y0), zero,
                                                             self.q(P.R_G * (1.0 + lift / (P.Z_MAX - P.Z_MIN)))))
        return c.to(torch.uint8)


# ------------------------------------------------------------------------------------------------------ measurements
def bench_step(repeats, iters):
    import world_common as W
    for n in (1, 64, 1024):
        world = P.PushWorld(n, DEV, frame_size=S, seed=0, start="scattered")
        actions = (torch.rand(n, 4, generator=torch.Generator().manual_seed(n)) * 2 - 1).to(DEV)
        frames = torch.empty(n, S, S, 3, dtype=torch.uint8, device=DEV)
        render = TorchRender(S, DEV)
        if n <= 64:                                                 # the two restatements agree with the kernel first
            want = W.render(W.step(world.state.cpu().numpy(), actions.cpu().numpy()), S)
            got_torch = render(torch_step(world.state, actions)).cpu().numpy()
            got = world.step(actions).cpu().numpy()
            world.reset(render=False)
            emit(bench="agreement", n=n, kernel_equals_numpy=bool(np.array_equal(got, want)),
                 torch_ops_equal_numpy=bool(np.array_equal(got_torch, want)))
        cands = {"fused": lambda: world.step(actions, out=frames),
                 "fused_no_frames": lambda: world.step(actions, render=False),
                 "render_only": lambda: world.render(out=frames)}
        its = {"fused": iters, "fused_no_frames": iters, "render_only": iters}
        tstate = [world.state.clone()]

        def torch_ops():
            tstate[0] = torch_step(tstate[0], actions)
            return render(tstate[0])
        cands["torch_ops"], its["torch_ops"] = torch_ops, max(2, iters // (4 if n < 1024 else 40))
        if n <= 64:
            hstate = [world.state.cpu().numpy()]
            hact = actions.cpu().numpy()

            def numpy_upload():
                hstate[0] = W.step(hstate[0], hact)
                W._render_cache.clear()
                return torch.from_numpy(W.render(hstate[0], S)).to(DEV)
            cands["numpy_plus_upload"], its["numpy_plus_upload"] = numpy_upload, 2
        timers = alternate({k: v for k, v in cands.items() if k != "numpy_plus_upload"}, repeats, its)
        if "numpy_plus_upload" in cands:
            timers.update(alternate({"numpy_plus_upload": cands["numpy_plus_upload"]}, max(3, repeats // 2), its, timer=host_ms))
        frame_bytes = n * S * S * 3
        for name, (med, lo, hi) in timers.items():
            row = dict(bench="step", n=n, size=S, variant=name, ms_median=round(med, 5), ms_min=round(lo, 5), ms_max=round(hi, 5))
            if name in ("fused", "render_only"):
                rate = frame_bytes / (med * 1e-3)
                row.update(frame_bytes=frame_bytes, write_GBps=round(rate / 1e9, 2), share_of_hbm_peak=round(rate / HBM_PEAK, 5))
            emit(**row)


def bench_generate(repeats):
    times = []
    for r in range(max(2, repeats // 2) + 1):
        out = tempfile.mkdtemp(prefix="push_gen_")
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            P.generate(1024, out, steps=15, seed=r, epsilon=0.2, batch=256, per_file=1000, device=DEV)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            size = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))
        finally:
            shutil.rmtree(out, ignore_errors=True)
    times = times[1:]                                               # the first run warms up
    emit(bench="generate", trajectories=1024, steps=15, s_median=round(statistics.median(times), 4), s_min=round(min(times), 4),
         s_max=round(max(times), 4), frames_per_s=round(1024 * 15 / statistics.median(times), 1), bundle_bytes=size)


def random_models():
    from ndivplanning_amd import evaluation as E
    from ndivplanning_amd.models.forward_encoder import ForwardAutoencoder
    from ndivplanning_amd.models.gan import Decoder
    from ndivplanning_amd.models.image_autoencoder import Encoder
    torch.manual_seed(0)
    mods = [m.to(DEV).eval() for m in (Encoder(), ForwardAutoencoder(), Decoder(2))]
    return E.EvalModels(mods[0], mods[1], mods[2], DEV)


def bench_mpc(repeats, rollouts=16, horizon=3):
    from ndivplanning_amd.evaluation import MpcController
    models = random_models()
    b = 16
    world = P.PushWorld(b, DEV, seed=0)
    ctrl = MpcController(models, rollouts, horizon, frame_shape=(S, S), seed=0)
    ctrl.reset(world.render())
    frames = world.render()
    host_actions = torch.zeros(b, 4)

    def loop_step():
        actions, _ = ctrl.act(frames)
        world.step(actions, out=frames)

    def world_share():
        world.step(host_actions, out=frames)
    timers = alternate({"mpc_step": loop_step, "world_step_host_actions": world_share}, repeats,
                       {"mpc_step": 20, "world_step_host_actions": 100}, timer=host_ms)
    for name, (med, lo, hi) in timers.items():
        emit(bench="mpc", envs=b, rollouts=rollouts, horizon=horizon, variant=name, ms_median=round(med, 4),
             ms_min=round(lo, 4), ms_max=round(hi, 4))
    emit(bench="mpc", envs=b, variant="world_share", share=round(timers["world_step_host_actions"][0] / timers["mpc_step"][0], 5))


def learn():
    """Recorded, claiming nothing."""
    from ndivplanning_amd import forward_model_eval
    from ndivplanning_amd.forward_trainer import ForwardModelTrainer
    from ndivplanning_amd.models.forward_encoder import ForwardAutoencoder
    from ndivplanning_amd.utils.trajectory_loader import PushDataset
    steps, batch, t_len = 300, 8, 15
    held = tempfile.mkdtemp(prefix="push_held_")
    try:
        P.generate(64, held, steps=t_len, seed=1001, epsilon=0.2, device=DEV)
        torch.manual_seed(0)
        model = ForwardAutoencoder().to(DEV).train()
        trainer = ForwardModelTrainer(model, batch=batch)
        world = P.PushWorld(256, DEV, seed=7)
        frames = torch.empty(t_len, 256, S, S, 3, dtype=torch.uint8, device=DEV)
        _, actions = P.rollout(world, t_len, 0.2, torch.Generator().manual_seed(7), frames)
        gen = torch.Generator().manual_seed(3)
        losses = []
        for it in range(steps):
            env = torch.randint(0, 256, (batch,), generator=gen).to(DEV)
            t = int(torch.randint(0, t_len - 1, (1,), generator=gen))
            cur = ((frames[t, env].permute(0, 3, 1, 2).float() / 255.0) - 0.5) * 2.0
            fut = ((frames[t + 1, env].permute(0, 3, 1, 2).float() / 255.0) - 0.5) * 2.0
            loss = trainer.step(cur.contiguous(), fut.contiguous(), actions[t, env].contiguous())
            if it % 50 == 0 or it == steps - 1:
                losses.append((it, float(loss)))
        model = trainer.sync_to_module().eval()
        result = forward_model_eval.evaluate(model, PushDataset(held, seq_length=t_len, raw_jpeg=True), horizon=5,
                                             batch_size=16, device=torch.device(DEV))
        emit(bench="learn", train_steps=steps, batch=batch, losses=losses,
             horizon_mse=[float(v) for v in result["horizon_mse"].tolist()],
             persistence_mse=[float(v) for v in result["persistence_mse"].tolist()])
    finally:
        shutil.rmtree(held, ignore_errors=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-generate", action="store_true")
    ap.add_argument("--skip-mpc", action="store_true")
    ap.add_argument("--learn", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_push_world.py measures on a GPU and found none: not measured")
    from ndivplanning_amd import _build
    _build.build()
    if not args.skip_step:
        bench_step(args.repeats, args.iters)
    if not args.skip_generate:
        bench_generate(args.repeats)
    if not args.skip_mpc:
        bench_mpc(args.repeats)
    if args.learn:
        learn()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
