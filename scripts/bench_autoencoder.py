"""Time one autoencoder training step (train_autoencoder.py:79-90) on the GPU box: the HIP trainer (ndp_ae_train_grads +
ndp_ae_apply_adam) vs the reference loop unchanged on PyTorch-ROCm / MIOpen (module forward, mse, backward,
torch.optim.Adam).  Median ms/step over STEPS timed steps after WARMUP, fraction of the fp32 MFMA peak, per-kernel split
of the HIP step.  Usage: python scripts/bench_autoencoder.py [N ...]   (default: 240 16)

python scripts/bench_autoencoder.py --shards [N ...]   (default: 240 120 60 30, the per-rank share of the reference's 240
images at 1, 2, 4, 8 ranks): per-rank compute time of one step at each shard size, through ndp_ae_train_grads and through
ndp_ae_train_grads_dp at world 1 (no statistics callback, no collective: the bucket events recorded and the weight-gradient
slabs summed per bucket) -- what bucketing costs on the compute path.  The two are timed alternately, median of STEPS.

python scripts/bench_autoencoder.py --eval [N ...]   (default: 240 16 1): the eval-mode autoencoder
(ndivplanning_amd.autoencoder_eval: ndp_encoder_forward + ndp_ae_decode) -- `reconstruct` (codes, reconstruction,
per-image and mean error) and `decode` alone -- against the same two through PyTorch-ROCm
(`dec._forward_torch(enc._forward_torch(x))` / `dec._forward_torch(z)`, eval mode, no_grad; the reconstruct arm with the
same per-image and mean error).  The four arms alternate, median of STEPS after WARMUP; then the per-kernel split of one
HIP reconstruct.  --eval-once N: one HIP reconstruct + decode after a warm-up, for a kernel trace."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ndivplanning_amd import _capi  # noqa: E402
from ndivplanning_amd.autoencoder_trainer import AutoencoderTrainer  # noqa: E402
from ndivplanning_amd.models.image_autoencoder import Decoder, Encoder  # noqa: E402

DEV = "cuda:0"
PEAK = 157.3e12                                      # fp32 MFMA, MI355X
STEPS, WARMUP = int(os.environ.get("STEPS", 20)), int(os.environ.get("WARMUP", 5))


def macs_per_image():
    """Forward multiply-adds of Encoder + Decoder per 128 x 128 image, from the module shapes."""
    total = 0
    hw = 128
    for cin, cout in ((3, 64), (64, 128), (128, 256), (256, 512), (512, 1024)):
        hw //= 2
        total += hw * hw * cout * cin * 9
    total += 1024 * 128 * 16                        # conv6
    total += 16 * 1024 * 128                        # deconv1 (4 x 4 outputs, one tap each)
    hw = 4
    for cin, cout in ((1024, 512), (512, 256), (256, 128), (128, 64), (64, 3)):
        hw *= 2
        total += hw * hw * cout * cin * 4           # stride 2, 4 x 4 kernel: 4 taps per output pixel
    return total


def models():
    torch.manual_seed(1)
    enc, dec = Encoder(), Decoder()
    dec.weight_init(0.0, 0.02)
    enc.weight_init(0.0, 0.02)
    return enc.to(DEV).train(), dec.to(DEV).train()


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


def main(sizes):
    flop_img = 2.0 * 3 * macs_per_image()            # forward + data gradients + weight gradients
    print("forward MACs per image %.1f M; %.2f GFLOP per training image" % (macs_per_image() / 1e6, flop_img / 1e9))
    for n in sizes:
        x = torch.rand(n, 3, 128, 128, device=DEV) * 2 - 1
        enc, dec = models()
        tr = AutoencoderTrainer(enc, dec, batch=n)
        t_hip = median_ms(lambda: tr.step(x))
        enc, dec = models()
        mse = torch.nn.MSELoss()
        opt = torch.optim.Adam([{"params": dec.parameters()}, {"params": enc.parameters()}], lr=2e-4, betas=(0.5, 0.999))

        def ref_step():
            loss = mse(dec(enc._forward_torch(x)), x)
            opt.zero_grad()
            loss.backward()
            opt.step()
        t_ref = median_ms(ref_step)
        flop = flop_img * n
        print("n=%d  hip %.3f ms/step = %.1f TFLOP/s (%.1f %% of peak)   pytorch-rocm %.3f ms/step = %.1f TFLOP/s "
              "(%.1f %%)   speed-up %.2fx" % (n, t_hip, flop / t_hip / 1e9, 100 * flop / (t_hip * 1e-3) / PEAK, t_ref,
                                             flop / t_ref / 1e9, 100 * flop / (t_ref * 1e-3) / PEAK, t_ref / t_hip))
        _capi.timing_enable(True)
        tr.step(x)
        torch.cuda.synchronize()
        split = sorted(_capi.timing_collect().items(), key=lambda kv: -kv[1][0])
        _capi.timing_enable(False)
        total = sum(v[0] for _, v in split)
        for name, (ms, cnt) in split[:16]:
            print("   %-26s %8.3f ms (%2d launches) %5.1f %%" % (name, ms, cnt, 100 * ms / total))


def shards(sizes):
    lib = _capi.load()
    p = _capi.ptr
    print("per-rank step (forward + backward + Adam), median of %d after %d warm-up; dp = ndp_ae_train_grads_dp at world 1"
          % (STEPS, WARMUP))
    for n in sizes:
        x = torch.rand(n, 3, 128, 128, device=DEV) * 2 - 1
        tr = AutoencoderTrainer(*models(), batch=n)

        def dp_step():
            _capi.check(lib.ndp_ae_train_grads_dp(p(tr.params), p(tr.stats), p(x), n, p(tr.grad), p(tr.loss),
                                                  p(tr.loss_sum), None, p(tr.workspace), _capi.stream_ptr(DEV), None, None,
                                                  1), "ndp_ae_train_grads_dp")
            tr.apply()
        for _ in range(WARMUP):
            tr.step(x)
            dp_step()
        torch.cuda.synchronize()
        ts = {"plain": [], "dp": []}
        for _ in range(STEPS):
            for name, fn in (("plain", lambda: tr.step(x)), ("dp", dp_step)):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts[name].append(time.perf_counter() - t0)
        med = {k: 1e3 * sorted(v)[len(v) // 2] for k, v in ts.items()}
        print("n=%d (%d ranks of 240)  ndp_ae_train_grads %.3f ms   ndp_ae_train_grads_dp %.3f ms   bucketing %+.3f ms "
              "(%+.1f %%)" % (n, 240 // n if 240 % n == 0 else 0, med["plain"], med["dp"], med["dp"] - med["plain"],
                              100 * (med["dp"] - med["plain"]) / med["plain"]))


def eval_models():
    """Eval-mode modules with non-trivial BatchNorm statistics (what a trained checkpoint has)."""
    enc, dec = models()
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for m in [*enc.modules(), *dec.modules()]:
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(0.5 + torch.rand(m.num_features, generator=gen))
                m.running_mean.copy_(0.1 * torch.randn(m.num_features, generator=gen))
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=gen))
    return enc.eval(), dec.eval()


def eval_mode(sizes):
    from ndivplanning_amd import autoencoder_eval as AE
    enc, dec = eval_models()
    print("eval-mode autoencoder, median of %d after %d warm-up, the four arms alternating" % (STEPS, WARMUP))
    for n in sizes:
        x = torch.rand(n, 3, 128, 128, device=DEV) * 2 - 1
        with torch.no_grad():
            z = enc(x)

        def torch_reconstruct():
            with torch.no_grad():
                y = dec._forward_torch(enc._forward_torch(x))
                sq = ((y - x) ** 2).reshape(n, -1).mean(dim=1)
                return y, sq, sq.mean()

        def torch_decode():
            with torch.no_grad():
                return dec._forward_torch(z)
        arms = (("hip reconstruct", lambda: AE.reconstruct(enc, dec, x)), ("torch reconstruct", torch_reconstruct),
                ("hip decode", lambda: AE.decode(dec, z)), ("torch decode", torch_decode))
        for _ in range(WARMUP):
            for _, fn in arms:
                fn()
        torch.cuda.synchronize()
        ts = {name: [] for name, _ in arms}
        for _ in range(STEPS):
            for name, fn in arms:
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts[name].append(time.perf_counter() - t0)
        med = {k: 1e3 * sorted(v)[len(v) // 2] for k, v in ts.items()}
        print("n=%d  reconstruct: hip %.3f ms  pytorch-rocm %.3f ms  (%.2fx)   decode: hip %.3f ms  pytorch-rocm %.3f ms  "
              "(%.2fx)" % (n, med["hip reconstruct"], med["torch reconstruct"], med["torch reconstruct"] / med["hip reconstruct"],
                           med["hip decode"], med["torch decode"], med["torch decode"] / med["hip decode"]))
        _capi.timing_enable(True)
        AE.reconstruct(enc, dec, x)
        torch.cuda.synchronize()
        split = sorted(_capi.timing_collect().items(), key=lambda kv: -kv[1][0])
        _capi.timing_enable(False)
        total = sum(v[0] for _, v in split)
        for name, (ms, cnt) in split[:16]:
            print("   %-26s %8.3f ms (%2d launches) %5.1f %%" % (name, ms, cnt, 100 * ms / total))


def eval_once(n):
    from ndivplanning_amd import autoencoder_eval as AE
    enc, dec = eval_models()
    x = torch.rand(n, 3, 128, 128, device=DEV) * 2 - 1
    for _ in range(3):
        _, _, mean = AE.reconstruct(enc, dec, x)
        out = AE.decode(dec, enc(x).detach(), out="bytes")
    torch.cuda.synchronize()
    print("n=%d mean error %.6f, bytes %s" % (n, mean.item(), tuple(out.shape)))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--eval"]:
        eval_mode([int(a) for a in sys.argv[2:]] or [240, 16, 1])
    elif sys.argv[1:2] == ["--eval-once"]:
        eval_once(int(sys.argv[2]) if len(sys.argv) > 2 else 240)
    elif sys.argv[1:2] == ["--shards"]:
        shards([int(a) for a in sys.argv[2:]] or [240, 120, 60, 30])
    else:
        main([int(a) for a in sys.argv[1:]] or [240, 16])
