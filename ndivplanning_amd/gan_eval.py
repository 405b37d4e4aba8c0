"""What a trained action generator (`models.gan.Decoder`, trained with the Normalized-Diversification loss) is asked
after training, on the gfx950 kernels: how close to the true action the best of its K samples is on held-out
trajectories, how that error falls with K, how far apart the samples are, what the diversity loss is on data it has not
seen, and whether the discriminator is any use for picking a sample.

    sample(generator, codes, num_sample)                  K actions per conditioning row: action_hat [n,K,4], noise [n,K,nz]
    score(action_hat, actions, noise, fake_logits)        the per-row scores of ndp_gan_score, one launch
    evaluate(generator, dataset, encoder, discriminator)  the same over a PushDataset / SyntheticPushDataset
    python -m ndivplanning_amd.gan_eval --generator gan_decoder_N.pt --data DIR [--discriminator ...] [--encoder ...]

The samples come from `ndp_g_forward` with code_rep = K (the K-fold repeat of the codes is never materialised), the noise
from `ndp_uniform_noise` (a seed and buffers of its own: torch's generators are never touched), the logits from
`ndp_d_forward`, the scores from `ndp_gan_score` (csrc/ndp_eval.inc; include/ndp.h states every output).  The modules are
used in eval mode; there is no CPU path, and nothing here synchronises with the host per batch: every result is a device
tensor.  Argument errors are ValueErrors raised before any launch."""
from argparse import ArgumentParser

import numpy as np
import torch

from . import _capi
from . import jpeg as jpeg_frames
from ._eval_io import fp64_mean, load_module, trajectory_batches
from .utils.trajectory_loader import open_dataset

CODE_DIM, ACTION_DIM = _capi.CODE_DIM, _capi.ACTION_DIM
OUTPUTS = ("sample_err", "mean_err", "best_err", "best_k", "best_curve", "spread", "ndiv", "d_fake_prob", "d_pick_k", "d_pick_err")
_INT = ("best_k", "d_pick_k")
_PER_SAMPLE = ("sample_err", "best_curve")
_NEEDS = {"sample_err": ("actions",), "mean_err": ("actions",), "best_err": ("actions",), "best_k": ("actions",),
          "best_curve": ("actions",), "spread": (), "ndiv": ("noise",), "d_fake_prob": ("fake_logits",),
          "d_pick_k": ("fake_logits",), "d_pick_err": ("fake_logits", "actions")}


def _device_f32(t, name, shape_text, ok):
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
    if not t.is_cuda:
        raise ValueError("%s is on %s: ndivplanning_amd computes only on a ROCm GPU (no CPU fallback)" % (name, t.device))
    if t.dtype != torch.float32 or not ok(t):
        raise ValueError("%s must be float32 %s, got %s %s" % (name, shape_text, t.dtype, tuple(t.shape)))
    return t.detach().contiguous()


def _check_eval(**modules):
    for name, m in modules.items():
        if m is not None and m.training:
            raise ValueError("the %s is in training mode: call .eval() first (these are the eval-mode kernels)" % name)


def _check_devices(device, **modules):
    """The device everything must be on (None: the first module's), as a torch.device with an index."""
    first = next(m for m in modules.values() if m is not None)
    device = torch.device(device) if device is not None else next(first.parameters()).device
    if device.type != "cuda":
        raise ValueError("device %s: ndivplanning_amd computes only on a ROCm GPU (no CPU fallback)" % device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    for name, m in modules.items():
        if m is not None and next(m.parameters()).device != device:
            raise ValueError("the %s is on %s, the evaluation on %s" % (name, next(m.parameters()).device, device))
    return device


def _check_num_sample(num_sample):
    k = int(num_sample)
    if not 1 <= k <= _capi.MAX_SAMPLES:
        raise ValueError("num_sample=%d outside 1..%d" % (k, _capi.MAX_SAMPLES))
    return k


def sample(generator, codes, num_sample, noise=None, seed=0):
    """K = num_sample actions for every row of codes [n,256]: (action_hat [n,K,4], noise [n,K,nz]).  Row r * K + k of the
    network input is cat(codes[r], noise[r,k]) -- `ndp_g_forward` with code_rep = K reads it from the two parts.  noise
    None: U[0,1) from `ndp_uniform_noise(seed, offset word 0)` into a buffer of this call; torch's global generators, on
    the CPU and on the GPU, are never touched."""
    k = _check_num_sample(num_sample)
    _check_eval(generator=generator)
    nz = int(generator.noise_dim)
    if not 1 <= nz <= _capi.MAX_NOISE_DIM:
        raise ValueError("noise_dim=%d outside 1..%d" % (nz, _capi.MAX_NOISE_DIM))
    codes = _device_f32(codes, "codes", "[n,%d]" % CODE_DIM, lambda t: t.dim() == 2 and t.shape[1] == CODE_DIM and t.shape[0] >= 1)
    n, dev = int(codes.shape[0]), codes.device
    if n * k >= 1 << 30:
        raise ValueError("%d rows of %d samples are more than one call takes" % (n, k))
    if noise is not None:
        noise = _device_f32(noise, "noise", "[%d,%d,%d]" % (n, k, nz), lambda t: tuple(t.shape) == (n, k, nz))
    flat = generator.flat_parameters()
    if flat.device != dev or (noise is not None and noise.device != dev):
        raise ValueError("codes are on %s, the generator on %s%s" % (dev, flat.device, "" if noise is None else ", noise on %s" % noise.device))
    lib = _capi.load()
    p = _capi.ptr
    action_hat = torch.empty(n, k, ACTION_DIM, dtype=torch.float32, device=dev)
    with _capi.on_device(codes):
        st = _capi.stream_ptr(dev)
        if noise is None:
            noise = torch.empty(n, k, nz, dtype=torch.float32, device=dev)
            _capi.check(lib.ndp_uniform_noise(p(noise), n * k * nz, int(seed), None, st), "ndp_uniform_noise")
        _capi.check(lib.ndp_g_forward(p(flat), nz, p(codes), CODE_DIM, k, p(noise), nz, n * k, None, p(action_hat), st),
                    "ndp_g_forward")
    return action_hat, noise


def score(action_hat, actions=None, noise=None, fake_logits=None, outputs=None):
    """ndp_gan_score on device tensors: action_hat float32 [n,K,4]; actions [n,4], noise [n,K,nz], fake_logits [n,K] or
    None.  outputs: the names wanted (OUTPUTS), None: every one the given inputs allow.  Returns {name: tensor}: [n,K] for
    sample_err / best_curve, [n] otherwise (int32 for best_k / d_pick_k)."""
    x = _device_f32(action_hat, "action_hat", "[n,K,4]", lambda t: t.dim() == 3 and t.shape[2] == ACTION_DIM and t.shape[0] >= 1)
    n, k, dev = int(x.shape[0]), int(x.shape[1]), x.device
    _check_num_sample(k)
    if n * k >= 1 << 31:
        raise ValueError("%d rows of %d samples are more than one call takes" % (n, k))
    given = {"actions": actions, "noise": noise, "fake_logits": fake_logits}
    if actions is not None:
        given["actions"] = _device_f32(actions, "actions", "[%d,4]" % n, lambda t: tuple(t.shape) == (n, ACTION_DIM))
    nz = 0
    if noise is not None:
        given["noise"] = _device_f32(noise, "noise", "[%d,%d,1..16]" % (n, k),
                                     lambda t: t.dim() == 3 and tuple(t.shape[:2]) == (n, k) and 1 <= t.shape[2] <= _capi.MAX_NOISE_DIM)
        nz = int(noise.shape[2])
    if fake_logits is not None:
        given["fake_logits"] = _device_f32(fake_logits, "fake_logits", "[%d,%d]" % (n, k), lambda t: t.numel() == n * k)
    for name, t in given.items():
        if t is not None and t.device != dev:
            raise ValueError("action_hat is on %s, %s on %s" % (dev, name, t.device))
    if outputs is None:
        outputs = tuple(o for o in OUTPUTS if all(given[i] is not None for i in _NEEDS[o]))
    outputs = tuple(outputs)
    if not outputs:
        raise ValueError("score: no output requested")
    for o in outputs:
        if o not in OUTPUTS:
            raise ValueError("unknown output %r: one of %s" % (o, ", ".join(OUTPUTS)))
        missing = [i for i in _NEEDS[o] if given[i] is None]
        if missing:
            raise ValueError("output %s needs %s" % (o, " and ".join(missing)))
    out = {o: torch.empty((n, k) if o in _PER_SAMPLE else (n,), dtype=torch.int32 if o in _INT else torch.float32, device=dev)
           for o in outputs}
    lib = _capi.load()
    p = _capi.ptr
    with _capi.on_device(x):
        _capi.check(lib.ndp_gan_score(p(x), n, k, p(given["actions"]), p(given["noise"]), nz, p(given["fake_logits"]),
                                      *[p(out.get(o)) for o in OUTPUTS], _capi.stream_ptr(dev)), "ndp_gan_score")
    return out


def discriminate(discriminator, actions, codes, code_rep=1):
    """`ndp_d_forward`: the logits [m] of actions [m,4] where row r is conditioned on codes[r // code_rep]."""
    lib = _capi.load()
    actions = actions.reshape(-1, ACTION_DIM)
    m = int(actions.shape[0])
    logits = torch.empty(m, dtype=torch.float32, device=actions.device)
    flat = discriminator.flat_parameters()
    p = _capi.ptr
    with _capi.on_device(actions):
        _capi.check(lib.ndp_d_forward(p(flat), p(actions), 1, p(codes), CODE_DIM, int(code_rep), m, p(logits),
                                      _capi.stream_ptr(actions.device)), "ndp_d_forward")
    return logits


def _yields_codes(frames):
    return isinstance(frames, torch.Tensor) and frames.dim() == 2


def _batches(dataset, first, batch_size, device, jpeg_decoder):
    """trajectory_batches with the item `evaluate` has read already: (frames [b,T,...], actions [b,T,4], b)."""
    return trajectory_batches(dataset, batch_size, device, jpeg_decoder, first=first)


def evaluate(generator, dataset, encoder=None, discriminator=None, num_sample=6, batch_size=16, seed=0, device=None):
    """The generator's scores over `dataset` (PushDataset / SyntheticPushDataset yielding (frames, states, actions, goal);
    frames: cached codes [T,128], float images, byte frames or JPEG streams, which `jpeg.JpegDecoder` decodes on the
    device).  Every frame but the last of every trajectory is one conditioning row: its code and the final frame's, as
    `train_gan.encode_batch` builds them, against the action taken there (`actions[:, :-1]`); `encoder` is required unless
    the dataset yields codes.  The noise of the whole dataset, [N (T - 1), K, nz], is drawn in ONE `ndp_uniform_noise`
    call and sliced by the batches: its bits do not depend on batch_size.  Returns a dict of device tensors (no host
    synchronisation per batch):
        action_mse [1]          the mean over rows of mean_err = mse(repeat_interleave(actions, K), action_hat)
        best_action_mse [1]     the mean of best_err, best_of_k_curve [K] that of best_curve (best of the first k + 1)
        spread [1], ndiv_per_row [1]     the means of spread and of ndiv (the diversity loss per conditioning row)
        d_fake_prob [1], d_real_prob [1], d_pick_mse [1]      with a discriminator: D's mean probability on the samples
                                and on the true actions, and the mean error of the sample D likes best
        count                   N (T - 1), an int
        rows                    {name: per-row tensor} of every score, plus action_hat [rows,K,4] and noise
        index [rows,2] int32    (trajectory, t)
    The means are taken in fp64 over the fp32 per-row values."""
    k = _check_num_sample(num_sample)
    if len(dataset) == 0 or int(batch_size) < 1:
        raise ValueError("evaluate needs a non-empty dataset and batch_size >= 1 (dataset: %d trajectories, batch_size %r)"
                         % (len(dataset), batch_size))
    T = int(dataset.seq_length)
    if T < 2:
        raise ValueError("a trajectory of %d frame(s) has no action to predict: T must be >= 2" % T)
    _check_eval(generator=generator, encoder=encoder, discriminator=discriminator)
    nz = int(generator.noise_dim)
    if not 1 <= nz <= _capi.MAX_NOISE_DIM:
        raise ValueError("noise_dim=%d outside 1..%d" % (nz, _capi.MAX_NOISE_DIM))
    first = dataset[0]
    is_jpeg = jpeg_frames.is_jpeg(dataset)
    if encoder is None and (is_jpeg or not _yields_codes(first[0])):
        raise ValueError("the dataset yields %s, not codes: evaluate needs the image encoder" % ("JPEG streams" if is_jpeg else "frames"))
    device = _check_devices(device, generator=generator, encoder=encoder, discriminator=discriminator)
    from .train_gan import encode_batch
    lib = _capi.load()
    total = len(dataset) * (T - 1)
    noise_all = torch.empty(total, k, nz, dtype=torch.float32, device=device)
    with _capi.on_device(device):
        _capi.check(lib.ndp_uniform_noise(_capi.ptr(noise_all), total * k * nz, int(seed), None, _capi.stream_ptr(device)),
                    "ndp_uniform_noise")
    jpeg_decoder = jpeg_frames.JpegDecoder(device, check="deferred") if is_jpeg else None
    rows = {o: [] for o in OUTPUTS if discriminator is not None or "fake_logits" not in _NEEDS[o]}
    hats, real_probs, row0 = [], [], 0
    for frames, actions, b in _batches(dataset, first, int(batch_size), device, jpeg_decoder):
        codes = encode_batch(frames, encoder, T)
        acts = actions[:, :-1].reshape(-1, actions.size(-1)).contiguous()
        n = b * (T - 1)
        action_hat, noise = sample(generator, codes, k, noise=noise_all[row0:row0 + n])
        logits = None
        if discriminator is not None:
            logits = discriminate(discriminator, action_hat, codes, code_rep=k).view(n, k)
            real_probs.append(torch.sigmoid(discriminate(discriminator, acts, codes)))
        got = score(action_hat, acts, noise, logits)
        for o in rows:
            rows[o].append(got[o])
        hats.append(action_hat)
        row0 += n
    if jpeg_decoder is not None:
        jpeg_decoder.finish()
    rows = {o: torch.cat(v) for o, v in rows.items()}
    result = {
        "action_mse": fp64_mean(rows["mean_err"], 0), "best_action_mse": fp64_mean(rows["best_err"], 0),
        "best_of_k_curve": fp64_mean(rows["best_curve"], 0), "spread": fp64_mean(rows["spread"], 0),
        "ndiv_per_row": fp64_mean(rows["ndiv"], 0), "count": total,
        "index": torch.from_numpy(np.stack([np.repeat(np.arange(len(dataset)), T - 1), np.tile(np.arange(T - 1), len(dataset))],
                                           axis=1).astype(np.int32)).to(device),
    }
    if discriminator is not None:
        rows["d_real_prob"] = torch.cat(real_probs)
        result.update(d_fake_prob=fp64_mean(rows["d_fake_prob"], 0), d_real_prob=fp64_mean(rows["d_real_prob"], 0),
                      d_pick_mse=fp64_mean(rows["d_pick_err"], 0))
    rows["action_hat"], rows["noise"] = torch.cat(hats), noise_all
    result["rows"] = rows
    return result


def make_dataset(path, seq_length=15, seed=2, raw_jpeg=False):
    """synthetic:<N>[:codes|images|frames_u8|jpeg] (codes by default, as train_gan's), or the HDF5 directory (byte frames;
    raw_jpeg: its JPEG streams, decoded on the device)."""
    return open_dataset(path, seq_length=int(seq_length), seed=seed, default_mode="codes",
                        push=dict(seq_length=int(seq_length), raw_uint8=not raw_jpeg, raw_jpeg=raw_jpeg))


def make_parser():
    parser = ArgumentParser(description="Best-of-K action error and diversity of a trained action generator")
    parser.add_argument("--generator", required=True, help="whole-module checkpoint (gan_decoder_N.pt of train_gan.py)")
    parser.add_argument("--discriminator", default=None, help="whole-module checkpoint (gan_discriminator_N.pt), optional")
    parser.add_argument("--encoder", default=None, help="whole-module image encoder checkpoint; not needed for cached codes")
    parser.add_argument("--data", required=True, help="trajectory directory, or synthetic:<N>[:codes|images|frames_u8|jpeg]")
    parser.add_argument("--raw-jpeg", action="store_true",
                        help="read the directory's JPEG streams as they are and decode them on the GPU")
    parser.add_argument("--num-sample", type=int, default=6, help="samples per conditioning row (K)")
    parser.add_argument("--seq-length", type=int, default=15, help="frames per trajectory (T)")
    parser.add_argument("--batch-size", type=int, default=16, help="trajectories per batch")
    parser.add_argument("--seed", type=int, default=0, help="seed of the evaluation's noise")
    parser.add_argument("--device", default="cuda")
    return parser


def main(argv=None, log=print):
    args = make_parser().parse_args(argv)
    device = torch.device(args.device)
    generator = load_module(args.generator, device)
    discriminator = load_module(args.discriminator, device) if args.discriminator else None
    encoder = load_module(args.encoder, device) if args.encoder else None
    dataset = make_dataset(args.data, seq_length=args.seq_length, raw_jpeg=args.raw_jpeg)
    result = evaluate(generator, dataset, encoder=encoder, discriminator=discriminator, num_sample=args.num_sample,
                      batch_size=args.batch_size, seed=args.seed, device=device)
    best = float(result["best_action_mse"].item())
    log("val_action_loss:", float(result["action_mse"].item()), "rows:", result["count"])
    log("val_best_action_loss:", best)
    log("val_div_loss:", float(result["ndiv_per_row"].item()))
    log("val_spread:", float(result["spread"].item()))
    for k, v in enumerate(result["best_of_k_curve"].tolist(), start=1):
        log("best of %d: action_mse %.8g" % (k, v))
    if discriminator is not None:
        log("val_d_fake_prob:", float(result["d_fake_prob"].item()))
        log("val_d_real_prob:", float(result["d_real_prob"].item()))
        log("val_d_pick_loss:", float(result["d_pick_mse"].item()))
    return best


if __name__ == "__main__":
    main()
