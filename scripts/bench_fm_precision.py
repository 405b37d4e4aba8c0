"""fp32 against bf16 operands in the eval-mode forward model (precision NDP_FM_BF16, include/ndp.h), one
process, the two arms alternating ROUNDS times; every figure is the median of the rounds with the spread (max - min) of
the rounds beside it, as in DESIGN.md 5e.

  pass      ndp_fm_forward_lp at n = 5, 32, 320 and 2,048 images: the whole pass (device events around REPS calls), the
            kernel times by label of one pass per round (the nine layers precision bf16 changes, and the rest), and
            ndp_fm_pack_params_lp
  planner   one planning step (evaluation.plan_step) at (B, R, Th) = (1, 5, 5) and (64, 32, 5)
  deviation max and rms of bf16 - fp32 over the predictions of the model of tests/golden/fm_eval_case.npz, on its own frames
            and on synthetic:64:frames_u8
  agreement the share of planning steps (B = 64 trajectories x STEPS draws of the noise, R = 32, Th = 5) whose chosen rollout
            differs between the arms.  Reported, not judged: with untrained weights the rollouts' errors lie close together.

Usage: python scripts/bench_fm_precision.py [pass] [planner] [deviation] [agreement]   (default: all four)
       SIZES="5 32" ROUNDS=3 REPS=10 python scripts/bench_fm_precision.py pass"""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ndivplanning_amd import _capi  # noqa: E402
from ndivplanning_amd import evaluation as E  # noqa: E402
from ndivplanning_amd import forward_model_eval as FME  # noqa: E402
from ndivplanning_amd.models.forward_encoder import ForwardAutoencoder, pack_module  # noqa: E402
from ndivplanning_amd.models.gan import Decoder  # noqa: E402
from ndivplanning_amd.models.image_autoencoder import Encoder  # noqa: E402

DEV = "cuda:0"
ARMS = ("fp32", "bf16")
ROUNDS, REPS = int(os.environ.get("ROUNDS", 3)), int(os.environ.get("REPS", 10))
SIZES = [int(v) for v in os.environ.get("SIZES", "5 32 320 2048").split()]
STEPS = int(os.environ.get("STEPS", 3))
NINE = ("conv2", "conv3", "conv4", "conv5", "deconv2", "deconv3", "deconv4", "deconv5", "deconv6")


def med_spread(values):
    v = sorted(values)
    return v[len(v) // 2], v[-1] - v[0]


def fmt(values, unit="ms"):
    m, s = med_spread(values)
    return "%9.3f %s (spread %.3f)" % (m, unit, s)


def golden_model():
    spec = importlib.util.spec_from_file_location("make_golden_fm_eval", os.path.join(ROOT, "tests", "golden", "make_golden_fm_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_module(ForwardAutoencoder), mod


def modules(nz=2):
    torch.manual_seed(0)
    enc, fm, gen = Encoder(), ForwardAutoencoder(), Decoder(nz)
    enc.weight_init(0.0, 0.02)
    fm.decoder.weight_init(0.0, 0.02)
    fm.encoder.weight_init(0.0, 0.02)
    return enc.to(DEV).eval(), fm.to(DEV).eval(), gen.to(DEV).eval()


class Pass:
    """The packed model, one workspace, the bf16 weights: ndp_fm_forward_lp by hand."""

    def __init__(self, model, n):
        self.lib = _capi.load()
        self.params, self.stats = pack_module(model, torch.device(DEV))
        self.ws = torch.empty(self.lib.ndp_fm_workspace_floats(n), dtype=torch.float32, device=DEV)
        self.lp = torch.empty(self.lib.ndp_fm_lp_weight_bytes(), dtype=torch.uint8, device=DEV)
        self.out = torch.empty(n, 3, 128, 128, dtype=torch.float32, device=DEV)
        _capi.check(self.lib.ndp_fm_pack_params(_capi.ptr(self.params), _capi.ptr(self.ws), _capi.stream_ptr()), "ndp_fm_pack_params")
        self.pack()

    def pack(self):
        _capi.check(self.lib.ndp_fm_pack_params_lp(_capi.ptr(self.params), _capi.ptr(self.ws), _capi.ptr(self.lp),
                                                   _capi.stream_ptr()), "ndp_fm_pack_params_lp")

    def run(self, arm, x, actions):
        u8 = x.dtype == torch.uint8
        _capi.check(self.lib.ndp_fm_forward_lp(_capi.ptr(self.params), _capi.ptr(self.stats), None if u8 else _capi.ptr(x),
                                               _capi.ptr(x) if u8 else None, _capi.ptr(actions), int(x.shape[0]), ARMS.index(arm),
                                               _capi.ptr(self.lp), _capi.ptr(self.out), _capi.ptr(self.ws), _capi.stream_ptr()),
                    "ndp_fm_forward_lp")
        return self.out


def event_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def by_label(fn):
    _capi.timing_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        return {k: v[0] for k, v in _capi.timing_collect().items()}
    finally:
        _capi.timing_enable(False)


def bench_pass(model):
    for n in SIZES:
        p = Pass(model, n)
        g = torch.Generator().manual_seed(n)
        x = torch.randint(40, 216, (n, 128, 128, 3), generator=g, dtype=torch.uint8).to(DEV)
        a = (torch.rand(n, 4, generator=g) * 2 - 1).to(DEV)
        for arm in ARMS:                                               # warm-up of both
            event_ms(lambda: p.run(arm, x, a), 2)
        whole, labels, pack = {arm: [] for arm in ARMS}, {arm: [] for arm in ARMS}, []
        for _ in range(ROUNDS):
            for arm in ARMS:
                whole[arm].append(event_ms(lambda: p.run(arm, x, a), REPS))
                labels[arm].append(by_label(lambda: p.run(arm, x, a)))
            pack.append(event_ms(p.pack, REPS))
        print("n = %d images (byte frames); whole pass, ms:" % n)
        for arm in ARMS:
            m, _ = med_spread(whole[arm])
            print("   %-5s %s   %8.2f us/image" % (arm, fmt(whole[arm]), 1e3 * m / n))
        m32, mlp = med_spread(whole["fp32"])[0], med_spread(whole["bf16"])[0]
        print("   fp32 / bf16 = %.2fx;  ndp_fm_pack_params_lp %s" % (m32 / mlp, fmt(pack)))
        print("   %-10s %28s %28s %7s" % ("layer", "fp32 kernel", "bf16 kernel", "ratio"))
        tot = {arm: 0.0 for arm in ARMS}
        for name in NINE:
            t32 = [r.get("k_fm_gemm[%s]" % name, 0.0) for r in labels["fp32"]]
            tlp = [r.get("k_fm_gemm_bf16[%s]" % name, 0.0) for r in labels["bf16"]]
            tot["fp32"] += med_spread(t32)[0]
            tot["bf16"] += med_spread(tlp)[0]
            print("   %-10s %28s %28s %6.2fx" % (name, fmt(t32), fmt(tlp), med_spread(t32)[0] / max(med_spread(tlp)[0], 1e-9)))
        rest = {arm: [sum(v for k, v in r.items() if not any(k.endswith("[%s]" % nm) for nm in NINE)) for r in labels[arm]]
                for arm in ARMS}
        reduce_ = {arm: [r.get("k_fm_splitk_reduce", 0.0) for r in labels[arm]] for arm in ARMS}
        print("   %-10s %26.3f ms %26.3f ms %6.2fx" % ("the nine", tot["fp32"], tot["bf16"], tot["fp32"] / max(tot["bf16"], 1e-9)))
        print("   %-10s %28s %28s   (of it k_fm_splitk_reduce %.3f / %.3f ms)"
              % ("the rest", fmt(rest["fp32"]), fmt(rest["bf16"]), med_spread(reduce_["fp32"])[0], med_spread(reduce_["bf16"])[0]))
        del p
        torch.cuda.empty_cache()


def planner_models(nets):
    return {arm: E.EvalModels(*nets, DEV, fm_precision=arm) for arm in ARMS}


def bench_planner(nets):
    for b, r, th in ((1, 5, 5), (64, 32, 5)):
        models = planner_models(nets)
        g = torch.Generator().manual_seed(b)
        state = (torch.rand(b, 3, 128, 128, generator=g) * 2 - 1).to(DEV)
        goal = (torch.rand(b, 3, 128, 128, generator=g) * 2 - 1).to(DEV)
        noise = torch.rand(E.plan_step_noise_floats(b, r, th, 2), generator=g).to(DEV)
        codes = {arm: models[arm].encode(goal) for arm in ARMS}
        step = lambda arm: E.plan_step(models[arm], state, goal, codes[arm], r, th, noise=noise)    # noqa: E731
        for arm in ARMS:
            event_ms(lambda: step(arm), 2)
        times = {arm: [] for arm in ARMS}
        for _ in range(ROUNDS):
            for arm in ARMS:
                times[arm].append(event_ms(lambda: step(arm), max(1, REPS // (4 if b > 1 else 1))))
        print("plan_step B = %d, R = %d, Th = %d (%d forward-model images per step):" % (b, r, th, b * r * th))
        for arm in ARMS:
            print("   %-5s %s" % (arm, fmt(times[arm])))
        print("   fp32 / bf16 = %.2fx" % (med_spread(times["fp32"])[0] / med_spread(times["bf16"])[0]))
        del models
        torch.cuda.empty_cache()


def bench_deviation(model, recipe):
    frames_u8, actions = recipe.inputs()
    cases = [("fm_eval_case frames", frames_u8.reshape(-1, 128, 128, 3), actions.reshape(-1, 4))]
    ds = FME.make_dataset("synthetic:64:frames_u8", seq_length=2)
    items = [ds[i] for i in range(len(ds))]
    cases.append(("synthetic:64:frames_u8", torch.stack([torch.as_tensor(it[0][0]) for it in items]),
                  torch.stack([torch.as_tensor(it[2][0]) for it in items]).float()))
    for name, x, a in cases:
        p = Pass(model, int(x.shape[0]))
        x, a = x.contiguous().to(DEV), a.contiguous().to(DEV)
        out32 = p.run("fp32", x, a).clone()
        d = (p.run("bf16", x, a) - out32).double()
        resid = out32.double() - ((x.double() / 255 - 0.5) * 2).permute(0, 3, 1, 2)
        print("deviation bf16 - fp32 on %s (%d images): max |d| %.4g, rms %.4g%s"
              % (name, x.shape[0], float(d.abs().max()), float(d.pow(2).mean().sqrt()),
                 "; rms of the fp32 residual itself %.4g" % float(resid.pow(2).mean().sqrt())))


def bench_agreement(nets):
    b, r, th = 64, 32, 5
    models = planner_models(nets)
    differ = total = 0
    gaps = []
    for s in range(STEPS):
        g = torch.Generator().manual_seed(100 + s)
        state = (torch.rand(b, 3, 128, 128, generator=g) * 2 - 1).to(DEV)
        goal = (torch.rand(b, 3, 128, 128, generator=g) * 2 - 1).to(DEV)
        noise = torch.rand(E.plan_step_noise_floats(b, r, th, 2), generator=g).to(DEV)
        picks, errs = {}, {}
        for arm in ARMS:
            _, picks[arm], errs[arm], _ = E.plan_step(models[arm], state, goal, models[arm].encode(goal), r, th, noise=noise)
        differ += int((picks["fp32"] != picks["bf16"]).sum())
        total += b
        e = errs["fp32"].sort(dim=1).values
        gaps.append(((e[:, 1] - e[:, 0]) / e[:, 0]).median().item())
    print("rollout agreement (untrained weights, B = %d, R = %d, Th = %d, %d draws): the chosen rollout differs in %d of %d "
          "planning steps (%.1f %%); median relative gap between the best and the second-best fp32 error %.3g"
          % (b, r, th, STEPS, differ, total, 100.0 * differ / total, sorted(gaps)[len(gaps) // 2]))


def main(what):
    what = what or ["pass", "planner", "deviation", "agreement"]
    model, recipe = golden_model()
    with torch.no_grad():
        if "pass" in what:
            bench_pass(model)
        if "deviation" in what:
            bench_deviation(model, recipe)
        if "planner" in what:
            bench_planner(modules())
        if "agreement" in what:
            bench_agreement(modules())


if __name__ == "__main__":
    main(sys.argv[1:])
