"""fp32 against bf16 in the image encoder's pass (precision NDP_ENC_BF16, include/ndp.h), one process, the
arms alternating ROUNDS times; every figure is the median of the rounds with the spread (max - min) of the rounds beside
it, as in DESIGN.md 5e.

  pass      ndp_encoder_forward_lp at n = 5, 32, 320 and 2,048 images, from byte frames and from float frames: the whole
            pass (device events around REPS calls), the kernel times by label of one pass per round (byte frames), and
            ndp_encoder_pack_params_lp
  planner   one planning step (evaluation.plan_step) at (B, R, Th) = (1, 5, 5) and (64, 32, 5) with fm_precision="bf16" and
            both encoder precisions, and with both precisions at fp32
  deviation max and rms of the codes bf16 - fp32, relative to the rms of the fp32 codes, on the encoder of
            tests/golden/encoder_case.npz and synthetic:64:frames_u8
  agreement the share of planning steps (B = 64 trajectories x STEPS draws of the noise, R = 32, Th = 5, fm_precision="bf16")
            whose chosen rollout differs between the encoder precisions.  Reported, not judged.

Usage: python scripts/bench_enc_precision.py [pass] [planner] [deviation] [agreement]   (default: all four)
       SIZES="5 32" ROUNDS=3 REPS=10 python scripts/bench_enc_precision.py pass"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ndivplanning_amd import _capi  # noqa: E402
from ndivplanning_amd import evaluation as E  # noqa: E402
from ndivplanning_amd import forward_model_eval as FME  # noqa: E402
from ndivplanning_amd.models.forward_encoder import ForwardAutoencoder  # noqa: E402
from ndivplanning_amd.models.gan import Decoder  # noqa: E402
from ndivplanning_amd.models.image_autoencoder import Encoder, pack_encoder_params  # noqa: E402

DEV = "cuda:0"
ARMS = ("fp32", "bf16")
ROUNDS, REPS = int(os.environ.get("ROUNDS", 3)), int(os.environ.get("REPS", 10))
SIZES = [int(v) for v in os.environ.get("SIZES", "5 32 320 2048").split()]
STEPS = int(os.environ.get("STEPS", 3))
LAYERS = ("conv1", "conv2", "conv3", "conv4", "conv5", "conv6")
LABELS = {"fp32": ("k_enc_conv1",) + tuple("k_conv_gemm[%d]" % i for i in range(2, 7)),
          "bf16": ("k_enc_conv1_bf16",) + tuple("k_conv_gemm_bf16[%d]" % i for i in range(2, 7))}


def med_spread(values):
    v = sorted(values)
    return v[len(v) // 2], v[-1] - v[0]


def fmt(values, unit="ms"):
    m, s = med_spread(values)
    return "%9.3f %s (spread %.3f)" % (m, unit, s)


def golden_encoder():
    from oracle import encoder_oracle as EO
    g = np.load(os.path.join(ROOT, "tests", "golden", "encoder_case.npz"))
    seed, bn_seed, _ = (int(v) for v in g["seeds"])
    enc = Encoder()
    enc.load_state_dict(EO.init_encoder_state(seed, bn_seed=bn_seed), strict=False)
    return enc.eval()


def modules(nz=2):
    torch.manual_seed(0)
    enc, fm, gen = Encoder(), ForwardAutoencoder(), Decoder(nz)
    enc.weight_init(0.0, 0.02)
    fm.decoder.weight_init(0.0, 0.02)
    fm.encoder.weight_init(0.0, 0.02)
    return enc.to(DEV).eval(), fm.to(DEV).eval(), gen.to(DEV).eval()


class Pass:
    """The packed encoder, one workspace, the bf16 weights: ndp_encoder_forward_lp by hand."""

    def __init__(self, enc, n):
        self.lib = _capi.load()
        self.params = pack_encoder_params(enc).to(DEV).contiguous()
        self.ws = torch.empty(self.lib.ndp_encoder_workspace_floats(n), dtype=torch.float32, device=DEV)
        self.lp = torch.empty(self.lib.ndp_encoder_lp_weight_bytes(), dtype=torch.uint8, device=DEV)
        self.codes = torch.empty(n, 128, dtype=torch.float32, device=DEV)
        self.pack()

    def pack(self):
        _capi.check(self.lib.ndp_encoder_pack_params_lp(_capi.ptr(self.params), _capi.ptr(self.lp), _capi.stream_ptr()),
                    "ndp_encoder_pack_params_lp")

    def run(self, arm, x):
        u8 = x.dtype == torch.uint8
        _capi.check(self.lib.ndp_encoder_forward_lp(_capi.ptr(self.params), None if u8 else _capi.ptr(x), _capi.ptr(x) if u8 else None,
                                                    int(x.shape[0]), ARMS.index(arm), _capi.ptr(self.lp), _capi.ptr(self.codes),
                                                    _capi.ptr(self.ws), _capi.stream_ptr()), "ndp_encoder_forward_lp")
        return self.codes


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


def bench_pass(enc):
    lut = ((torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255) - 0.5) * 2.0).to(DEV)
    for n in SIZES:
        p = Pass(enc, n)
        g = torch.Generator().manual_seed(n)
        xb = torch.randint(40, 216, (n, 128, 128, 3), generator=g, dtype=torch.uint8).to(DEV)
        inputs = {"byte": xb, "float": lut[xb.long()].permute(0, 3, 1, 2).contiguous()}
        for arm in ARMS:                                               # warm-up of both
            for x in inputs.values():
                event_ms(lambda: p.run(arm, x), 2)
        whole = {(arm, kind): [] for arm in ARMS for kind in inputs}
        labels, pack = {arm: [] for arm in ARMS}, []
        for _ in range(ROUNDS):
            for arm in ARMS:
                for kind, x in inputs.items():
                    whole[(arm, kind)].append(event_ms(lambda: p.run(arm, x), REPS))
                labels[arm].append(by_label(lambda: p.run(arm, xb)))
            pack.append(event_ms(p.pack, REPS))
        print("n = %d images; whole pass, ms:" % n)
        for kind in inputs:
            for arm in ARMS:
                m, _ = med_spread(whole[(arm, kind)])
                print("   %-5s frames %-5s %s   %8.2f us/image" % (kind, arm, fmt(whole[(arm, kind)]), 1e3 * m / n))
            print("   %-5s frames fp32 / bf16 = %.2fx" % (kind, med_spread(whole[("fp32", kind)])[0] / med_spread(whole[("bf16", kind)])[0]))
        print("   ndp_encoder_pack_params_lp %s" % fmt(pack))
        print("   %-10s %28s %28s %7s" % ("layer", "fp32 kernel", "bf16 kernel", "ratio"))
        for i, name in enumerate(LAYERS):
            t32 = [r.get(LABELS["fp32"][i], 0.0) for r in labels["fp32"]]
            tlp = [r.get(LABELS["bf16"][i], 0.0) for r in labels["bf16"]]
            print("   %-10s %28s %28s %6.2fx" % (name, fmt(t32), fmt(tlp), med_spread(t32)[0] / max(med_spread(tlp)[0], 1e-9)))
        red32 = [r.get("k_splitk_reduce", 0.0) for r in labels["fp32"]]
        redlp = [r.get("k_splitk_reduce", 0.0) + r.get("k_splitk_reduce_bf16", 0.0) for r in labels["bf16"]]
        print("   %-10s %28s %28s" % ("reductions", fmt(red32), fmt(redlp)))
        del p
        torch.cuda.empty_cache()


PLANNER_ARMS = (("fp32", "fp32"), ("bf16", "fp32"), ("bf16", "bf16"))   # (fm_precision, enc_precision)


def planner_models(nets, arms=PLANNER_ARMS):
    return {arm: E.EvalModels(*nets, DEV, fm_precision=arm[0], enc_precision=arm[1]) for arm in arms}


def bench_planner(nets):
    for b, r, th in ((1, 5, 5), (64, 32, 5)):
        models = planner_models(nets)
        g = torch.Generator().manual_seed(b)
        state = (torch.rand(b, 3, 128, 128, generator=g) * 2 - 1).to(DEV)
        goal = (torch.rand(b, 3, 128, 128, generator=g) * 2 - 1).to(DEV)
        noise = torch.rand(E.plan_step_noise_floats(b, r, th, 2), generator=g).to(DEV)
        codes = {arm: models[arm].encode(goal) for arm in PLANNER_ARMS}
        step = lambda arm: E.plan_step(models[arm], state, goal, codes[arm], r, th, noise=noise)    # noqa: E731
        for arm in PLANNER_ARMS:
            event_ms(lambda: step(arm), 2)
        times = {arm: [] for arm in PLANNER_ARMS}
        for _ in range(ROUNDS):
            for arm in PLANNER_ARMS:
                times[arm].append(event_ms(lambda: step(arm), max(1, REPS // (4 if b > 1 else 1))))
        print("plan_step B = %d, R = %d, Th = %d (%d encoded images per step besides the state's):" % (b, r, th, b * r * (th - 1)))
        for arm in PLANNER_ARMS:
            print("   fm %-5s enc %-5s %s" % (arm[0], arm[1], fmt(times[arm])))
        print("   fm bf16: enc fp32 / enc bf16 = %.3fx"
              % (med_spread(times[("bf16", "fp32")])[0] / med_spread(times[("bf16", "bf16")])[0]))
        del models
        torch.cuda.empty_cache()


def bench_deviation(enc):
    ds = FME.make_dataset("synthetic:64:frames_u8", seq_length=2)
    x = torch.stack([torch.as_tensor(ds[i][0][0]) for i in range(len(ds))]).contiguous().to(DEV)
    p = Pass(enc, int(x.shape[0]))
    c32 = p.run("fp32", x).double().clone()
    d = p.run("bf16", x).double() - c32
    rms = float(c32.pow(2).mean().sqrt())
    print("deviation of the codes bf16 - fp32 on synthetic:64:frames_u8 (%d images, the encoder of encoder_case.npz): max |d| %.4g, "
          "rms %.4g; relative to the codes' rms %.4g: max %.4g, rms %.4g"
          % (x.shape[0], float(d.abs().max()), float(d.pow(2).mean().sqrt()), rms, float(d.abs().max()) / rms,
             float(d.pow(2).mean().sqrt()) / rms))


def bench_agreement(nets):
    b, r, th = 64, 32, 5
    arms = (("bf16", "fp32"), ("bf16", "bf16"))
    models = planner_models(nets, arms)
    differ = total = 0
    for s in range(STEPS):
        g = torch.Generator().manual_seed(100 + s)
        state = (torch.rand(b, 3, 128, 128, generator=g) * 2 - 1).to(DEV)
        goal = (torch.rand(b, 3, 128, 128, generator=g) * 2 - 1).to(DEV)
        noise = torch.rand(E.plan_step_noise_floats(b, r, th, 2), generator=g).to(DEV)
        picks = {}
        for arm in arms:
            _, picks[arm], _, _ = E.plan_step(models[arm], state, goal, models[arm].encode(goal), r, th, noise=noise)
        differ += int((picks[arms[0]] != picks[arms[1]]).sum())
        total += b
    print("rollout agreement (untrained weights, fm bf16, B = %d, R = %d, Th = %d, %d draws): the chosen rollout differs between "
          "the encoder precisions in %d of %d planning steps (%.1f %%)" % (b, r, th, STEPS, differ, total, 100.0 * differ / total))


def main(what):
    what = what or ["pass", "planner", "deviation", "agreement"]
    enc = golden_encoder()
    with torch.no_grad():
        if "pass" in what:
            bench_pass(enc)
        if "deviation" in what:
            bench_deviation(enc)
        if "planner" in what:
            bench_planner(modules())
        if "agreement" in what:
            bench_agreement(modules())


if __name__ == "__main__":
    main(sys.argv[1:])
