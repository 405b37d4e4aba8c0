"""Time the planner's gradient stage (evaluation.plan_step with `grad`) on the GPU box: synthetic frames, random weights,
R = 32 rollouts, horizon Th = 5, G = 4 refined rows, B = 1 and 64 environments, per planning step:
  step J     the whole planning step with J = 0..3 gradient iterations (no `cem`): population 0, the stage, one more
             open-loop rollout of the population, the choice
  stage J    the stage alone (evaluation._grad_stage: one selection, the gather, J x (Th kept forward passes on B * G rows,
             the seed, Th backward calls, the update))
  autograd J the same refinement the way the code before the stage offers it: evaluation.refine_actions on the gathered
             rows with torch.optim.Adam (one autograd.Function per forward pass, a torch optimiser)
and the three launches' own times from ndp_timing_*, with k_plan_goal_grad's achieved bytes per second beside the HBM
peak.  Expectation, stated and checked (exit status 1 if it fails): the stage is not slower than the autograd route at any
measured point.  No ratio is promised.
  --default-path   times only the planning step without `grad` and without `cem` (and with `cem`, I = 1..3), and imports
                   the package from --tree DIR: a job runs it on a checkout of the parent commit and on this one in turn
With random weights the goal error says nothing about plan quality: this script reports time only.  Median over STEPS
timed repetitions after WARMUP.  Usage: python scripts/bench_mpc_grad.py [--default-path] [--tree DIR] [B ...]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEV = "cuda:0"
R, TH, G, NZ, ITERATIONS = 32, 5, 4, 2, 3
STEPS, WARMUP = int(os.environ.get("STEPS", 5)), int(os.environ.get("WARMUP", 2))
HBM_PEAK = 8.0e12                # bytes per second, the MI355X's data sheet
IMAGE_BYTES = 4 * 3 * 128 * 128


def modules(torch):
    from ndivplanning_amd.models.forward_encoder import ForwardAutoencoder
    from ndivplanning_amd.models.gan import Decoder
    from ndivplanning_amd.models.image_autoencoder import Encoder
    torch.manual_seed(0)
    enc, fm, gen = Encoder(), ForwardAutoencoder(), Decoder(NZ)
    enc.weight_init(0.0, 0.02)
    fm.decoder.weight_init(0.0, 0.02)
    fm.encoder.weight_init(0.0, 0.02)
    return enc.to(DEV).eval(), fm.to(DEV).eval(), gen.to(DEV).eval()


def median_ms(torch, fn):
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


def default_path(sizes):
    """The planning step as it was before the stage: no `grad` anywhere, so the same lines run on the parent commit."""
    import torch

    from ndivplanning_amd import evaluation as E
    models = E.EvalModels(*modules(torch), DEV)
    for b in sizes:
        state = torch.rand(b, 3, 128, 128, device=DEV) * 2 - 1
        goal = torch.rand(b, 3, 128, 128, device=DEV) * 2 - 1
        goal_code = models.encode(goal)
        with torch.no_grad():
            ms = [median_ms(torch, lambda: E.plan_step(models, state, goal, goal_code, R, TH, seed=1))]
            for i in range(1, ITERATIONS + 1):
                cem = E.CemSettings(iterations=i)
                ms.append(median_ms(torch, lambda: E.plan_step(models, state, goal, goal_code, R, TH, seed=1, cem=cem)))
        print("default B=%d  no cem %.3f ms   cem I=1 %.3f  I=2 %.3f  I=3 %.3f" % (b, *ms), flush=True)


def main(sizes):
    import torch

    from ndivplanning_amd import _capi
    from ndivplanning_amd import evaluation as E
    enc, fm, gen = modules(torch)
    models = E.EvalModels(enc, fm, gen, DEV)
    held = True
    print("R=%d Th=%d G=%d: one planning step; the stage runs J * Th forward and backward passes on B * G rows" % (R, TH, G))
    for b in sizes:
        n = b * G
        # the autograd arm's workspaces are those of this batch size alone: the module's pool of input-gradient workspaces
        # looks an entry up with list.remove, which compares tensors and fails once the pool holds two sizes
        fm.invalidate_cache()
        torch.cuda.empty_cache()
        state = torch.rand(b, 3, 128, 128, device=DEV) * 2 - 1
        goal = torch.rand(b, 3, 128, 128, device=DEV) * 2 - 1
        goal_code = models.encode(goal)
        floats = models.lib.ndp_fm_workspace_floats(n)
        print("B=%d: %d refined rows; the Th = %d kept workspaces take %d x %.1f MB = %.2f GB"
              % (b, n, TH, TH, 4e-6 * floats, 4e-9 * floats * TH))
        # a scored population for the stage and the autograd arm: the planner's own population 0
        _, pick, err, _ = E.plan_step(models, state, goal, goal_code, R, TH, seed=1)
        seq = torch.rand(TH, b, R, 4, device=DEV) * 2 - 1
        rep = torch.empty(b * R, 3, 128, 128, device=DEV)
        pred, _ = E._rollout_open(models, state, seq, rep)
        act = torch.empty(b, 4, device=DEV)
        order = err.argsort(dim=1)[:, :G]                                            # the rows the stage gathers
        rows = seq.gather(2, order.view(1, b, G, 1).expand(TH, b, G, 4)).reshape(TH, n, 4).transpose(0, 1).contiguous()
        state_g, goal_g = state.repeat_interleave(G, 0), goal.repeat_interleave(G, 0)
        for j in range(ITERATIONS + 1):
            grad = E.GradSettings(iterations=j, rows=G)
            with torch.no_grad():
                step = median_ms(torch, lambda: E.plan_step(models, state, goal, goal_code, R, TH, seed=1, grad=grad))
            line = "   J=%d  step %9.3f ms" % (j, step)
            if j:
                def stage():
                    io = E._grad_buffers(grad, (), b, R, DEV)
                    E._grad_stage(models, grad, io, state, goal, b, R, seq.clone(), pred, err, pick, act)
                with torch.no_grad():
                    mine = median_ms(torch, stage)
                ref = median_ms(torch, lambda: E.refine_actions(fm, state_g, goal_g, rows, j,
                                                                lambda p: torch.optim.Adam(p, lr=grad.lr)))
                ok = mine <= ref
                held = held and ok
                line += "   stage %9.3f ms   autograd %9.3f ms   %s" % (mine, ref, "not slower" if ok else "SLOWER")
            print(line, flush=True)
        grad = E.GradSettings(iterations=ITERATIONS, rows=G)
        with torch.no_grad():
            E.plan_step(models, state, goal, goal_code, R, TH, seed=1, grad=grad)
            torch.cuda.synchronize()
            _capi.timing_enable(True)
            E.plan_step(models, state, goal, goal_code, R, TH, seed=1, grad=grad)
            torch.cuda.synchronize()
            split = _capi.timing_collect()
            _capi.timing_enable(False)
        for name in ("k_plan_goal_grad", "k_plan_grad_gather", "k_plan_grad_step"):
            ms, cnt = split[name]
            line = "   %-20s %3d launches, %7.1f us each" % (name, cnt, 1e3 * ms / cnt)
            if name == "k_plan_goal_grad":
                moved = (2 * n + b) * IMAGE_BYTES                                   # pred in, d_pred out, each goal once
                rate = moved / (1e-3 * ms / cnt)
                line += "   %.2f MB per launch, %.3f TB/s = %.1f %% of the %.1f TB/s HBM peak" % (
                    1e-6 * moved, 1e-12 * rate, 100 * rate / HBM_PEAK, 1e-12 * HBM_PEAK)
            print(line, flush=True)
    print("expectation (the stage is not slower than the autograd route at any measured point): %s"
          % ("held" if held else "NOT held"))
    return 0 if held else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="time the planner's gradient stage per planning step")
    ap.add_argument("sizes", nargs="*", type=int, default=[1, 64], metavar="B")
    ap.add_argument("--default-path", action="store_true", help="only the planning step without `grad`")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is imported (default: this one)")
    ns = ap.parse_args()
    sys.path.insert(0, os.path.abspath(ns.tree))
    if ns.default_path:
        default_path(ns.sizes or [1, 64])
        sys.exit(0)
    sys.exit(main(ns.sizes or [1, 64]))
