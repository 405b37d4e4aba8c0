"""Time the cross-entropy planner (evaluation.plan_step with `cem`) on the GPU box: synthetic frames, random weights,
R = 32 rollouts, horizon Th = 5, B = 1 and 64 environments, per planning step:
  cem I      I = 0..3 iterations after the generator's population: (I + 1) * Th forward-model passes on B * R rows
  uniform I  the same with the uniform proposal (no generator, no encoder inside the horizon)
  single     the single-shot planner (no `cem`) with R * (I + 1) rollouts: the same number of forward-model rows, the
             equal-budget comparison
and the launches' own times (k_plan_cem_update or k_plan_update, k_plan_warm, k_normal_noise) from ndp_timing_*.
  --weighting mppi --temperature T   the refit with MPPI weights (ndp_plan_update) in the cem / uniform arms
  --warm-start                       adds the arm `warm I` (I >= 1): the same planning step started from the fit of a
                                     previous one (plan_step's `prior`: one ndp_plan_warm and Th slice copies more)
With random weights the goal error says nothing about plan quality: this script reports time only.  Median over STEPS
timed repetitions after WARMUP.  Usage: python scripts/bench_mpc_cem.py [options] [B ...]   (default: 1 64)"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ndivplanning_amd import _capi  # noqa: E402
from ndivplanning_amd import evaluation as E  # noqa: E402
from ndivplanning_amd.models.forward_encoder import ForwardAutoencoder  # noqa: E402
from ndivplanning_amd.models.gan import Decoder  # noqa: E402
from ndivplanning_amd.models.image_autoencoder import Encoder  # noqa: E402

DEV = "cuda:0"
R, TH, NZ, ITERATIONS = 32, 5, 2, 3
STEPS, WARMUP = int(os.environ.get("STEPS", 5)), int(os.environ.get("WARMUP", 2))
SINGLE_MAX_ROWS = 4096           # the forward model's workspace takes 26 MB per row (106 GiB here): the single-shot arm,
                                 # which puts B * R * (I + 1) rows into one call, stops at this many


def modules():
    torch.manual_seed(0)
    enc, fm, gen = Encoder(), ForwardAutoencoder(), Decoder(NZ)
    enc.weight_init(0.0, 0.02)
    fm.decoder.weight_init(0.0, 0.02)
    fm.encoder.weight_init(0.0, 0.02)
    return enc.to(DEV).eval(), fm.to(DEV).eval(), gen.to(DEV).eval()


def median_ms(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(STEPS):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return 1e3 * ts[len(ts) // 2]


def main(sizes, weighting="elites", temperature=None, warm_start=False):
    nets = modules()
    how = dict(weighting=weighting, temperature=temperature)
    models = E.EvalModels(*nets, DEV)
    print("R=%d Th=%d: one planning step; forward-model rows per step = B * R * Th * (I + 1)" % (R, TH))
    for b in sizes:
        state = torch.rand(b, 3, 128, 128, device=DEV) * 2 - 1
        goal = torch.rand(b, 3, 128, 128, device=DEV) * 2 - 1
        goal_code = models.encode(goal)
        print("B=%d" % b)
        with torch.no_grad():
            for i in range(ITERATIONS + 1):
                row = {}
                for proposal in ("generator", "uniform"):
                    cem = E.CemSettings(iterations=i, proposal=proposal, **how)
                    row[proposal] = median_ms(lambda: E.plan_step(models, state, goal, goal_code, R, TH, seed=1, cem=cem))
                warm = ""
                if warm_start and i >= 1:
                    cem = E.CemSettings(iterations=i, warm_start=True, **how)
                    info = E.plan_step(models, state, goal, goal_code, R, TH, seed=1, cem=cem)[4]
                    prior = info["cem_mean"], info["cem_std"]
                    warm = "   warm %9.3f ms" % median_ms(lambda: E.plan_step(models, state, goal, goal_code, R, TH, seed=1,
                                                                               cem=cem, prior=prior))
                rows = R * (i + 1)
                if b * rows <= SINGLE_MAX_ROWS and rows <= _capi.MAX_SAMPLES:
                    wide = E.EvalModels(*nets, DEV)                  # its own workspace, released after the measurement
                    single = "%9.3f ms" % median_ms(lambda: E.plan_step(wide, state, goal, goal_code, rows, TH, seed=1))
                    del wide
                    torch.cuda.empty_cache()
                else:
                    single = "not measured (%d rows in one forward-model call: its workspace does not fit)" % (b * rows)
                print("   I=%d  cem %9.3f ms%s   uniform %9.3f ms   single-shot with R=%-3d %s   (%d forward-model rows)"
                      % (i, row["generator"], warm, row["uniform"], rows, single, b * rows * TH))
            cem = E.CemSettings(iterations=ITERATIONS, warm_start=warm_start, **how)
            info = E.plan_step(models, state, goal, goal_code, R, TH, seed=1, cem=cem)[4]
            prior = (info["cem_mean"], info["cem_std"]) if warm_start else None
            E.plan_step(models, state, goal, goal_code, R, TH, seed=1, cem=cem, prior=prior)
            torch.cuda.synchronize()
            _capi.timing_enable(True)
            E.plan_step(models, state, goal, goal_code, R, TH, seed=1, cem=cem, prior=prior)
            torch.cuda.synchronize()
            split = sorted(_capi.timing_collect().items(), key=lambda kv: -kv[1][0])
            _capi.timing_enable(False)
        total = sum(v[0] for _, v in split)
        for name, (ms, cnt) in split:
            if name in ("k_plan_cem_update", "k_plan_update", "k_plan_warm", "k_normal_noise") or ms >= 0.02 * total:
                print("   %-26s %8.3f ms (%3d launches, %7.1f us each) %5.1f %%" % (name, ms, cnt, 1e3 * ms / cnt,
                                                                                  100 * ms / total))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="time the cross-entropy / MPPI planner per planning step")
    ap.add_argument("sizes", nargs="*", type=int, default=[1, 64], metavar="B")
    ap.add_argument("--weighting", choices=E.WEIGHTINGS, default="elites")
    ap.add_argument("--temperature", type=float, default=None, help="required with --weighting mppi")
    ap.add_argument("--warm-start", action="store_true")
    ns = ap.parse_args()
    main(ns.sizes or [1, 64], ns.weighting, ns.temperature, ns.warm_start)
