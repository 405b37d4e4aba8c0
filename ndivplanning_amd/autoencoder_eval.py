"""What a trained image autoencoder is asked after training, on the gfx950 kernels: what a code decodes to, what the
reconstructions look like and how large the reconstruction error is on held-out trajectories.

    decode(decoder, codes)                    codes [n,128] / [n,128,1,1]  ->  images, float NCHW or bytes HWC
    reconstruct(encoder, decoder, images)     decoder(encoder(x)), the MSE of every image against x and their mean
    evaluate(encoder, decoder, dataset)       the same over a PushDataset / SyntheticPushDataset (JPEG mode included)
    python -m ndivplanning_amd.autoencoder_eval --encoder encoder_N.pt --decoder decoder_N.pt --data DIR [--save-dir DIR]

The codes come from the eval-mode `Encoder` (ndp_encoder_forward / _u8), the images from `ndp_ae_decode`
(csrc/ndp_autoencoder.inc: the eval-mode decoder with its BatchNorms folded into the weights, and an output kernel that
also writes the reference's bytes, `denorm(...).astype(np.uint8)` of train_autoencoder.py:42-43, 97-100, and the squared
error against the input).  Both modules are used in eval mode; there is no CPU path (`NdpError`), and nothing here
synchronises with the host: every result is a device tensor.  evaluate(quality=True) / --quality add SSIM and PSNR of
every reconstruction against its input (`ndp_image_quality`, image_quality.py); off by default, nothing else changes."""
import os
from argparse import ArgumentParser

import torch

from . import _capi
from . import image_quality as IQ
from . import jpeg as jpeg_frames
from ._eval_io import OUTPUTS, _check_out, _require_eval, _require_gpu, _to_bytes, fp64_mean, load_module  # noqa: F401
from ._eval_io import trajectory_batches
from .models import image_autoencoder as IA


def decode(decoder, codes, out="float"):
    """The image every code decodes to: float32 [n,3,128,128] in [-1,1] (out="float") or uint8 [n,128,128,3], the
    reference's denormalised bytes (out="bytes")."""
    _check_out(out)
    _require_gpu(codes, "codes")
    _require_eval(decoder=decoder)
    return IA.decoder_forward_hip(decoder, codes, out=out)[0]


def _encode(encoder, images):
    _require_gpu(images, "images")
    with torch.no_grad():
        return encoder(images.detach())


def reconstruct(encoder, decoder, images, out="float", errors=True):
    """(reconstruction, per-image MSE [n], mean MSE [1]) of `images`, float32 [n,3,128,128] in [-1,1] or byte frames
    uint8 [n,128,128,3] (normalised as the loader does, as the kernels read them).  The error is against the input
    itself; errors=False: (reconstruction, None, None)."""
    _check_out(out)
    _require_eval(encoder=encoder, decoder=decoder)
    codes = _encode(encoder, images)
    return IA.decoder_forward_hip(decoder, codes, out=out, target=images if errors else None, errors=errors)


def evaluate(encoder, decoder, dataset, batch_size=16, device=None, keep=0, quality=False):
    """The reconstruction error over every frame of `dataset` (PushDataset / SyntheticPushDataset: images, byte frames or
    JPEG streams, which `jpeg.JpegDecoder` decodes on the device): (mean MSE [1], per-image MSE [frames]) -- device
    tensors, no host synchronisation per batch.  keep > 0: also the first `keep` (input bytes, reconstruction bytes)
    pairs, uint8 [keep,128,128,3] each, as a third result.  quality=True: the last result is a dict of the unquantised
    reconstructions' SSIM and PSNR against their inputs, {"ssim" [frames], "psnr" [frames], "mean_ssim" [1], "mean_psnr"
    [1]} (means in fp64 over the fp32 values, none skipped); the results before it hold the same bits."""
    _require_eval(encoder=encoder, decoder=decoder)
    device = torch.device(device) if device is not None else next(decoder.parameters()).device
    if device.type != "cuda":
        raise _capi.NdpError("the modules are on %s: ndivplanning_amd computes only on a ROCm GPU (no CPU fallback)" % device)
    if len(dataset) == 0 or int(batch_size) < 1:
        raise ValueError("evaluate needs a non-empty dataset and batch_size >= 1")
    jpeg_decoder = jpeg_frames.JpegDecoder(device, check="deferred") if jpeg_frames.is_jpeg(dataset) else None
    per_image, pairs, kept, ssim, psnr = [], [], 0, [], []
    for frames, _, _ in trajectory_batches(dataset, int(batch_size), device, jpeg_decoder, actions=False):
        frames = frames.view(-1, *frames.shape[2:])                      # [b*T,...]
        recon, sq, _ = reconstruct(encoder, decoder, frames, out="float" if quality else "bytes", errors=True)
        per_image.append(sq)
        if quality:
            s, p = IQ.image_quality(recon, frames)
            ssim.append(s)
            psnr.append(p)
        if kept < keep:
            k = min(keep - kept, int(frames.shape[0]))
            if quality:                                                  # the bytes of the few that are kept
                recon = reconstruct(encoder, decoder, frames[:k].contiguous(), out="bytes", errors=False)[0]
            pairs.append((_to_bytes(frames[:k]), recon[:k]))
            kept += k
    if jpeg_decoder is not None:
        jpeg_decoder.finish()
    per_image = torch.cat(per_image)
    mean = fp64_mean(per_image)                                          # (as ndp_ae_decode's)
    result = (mean, per_image)
    if keep > 0:
        result += ((torch.cat([a for a, _ in pairs]), torch.cat([b for _, b in pairs])),)
    if quality:
        ssim, psnr = torch.cat(ssim), torch.cat(psnr)
        result += ({"ssim": ssim, "psnr": psnr, "mean_ssim": IQ.mean(ssim), "mean_psnr": IQ.mean(psnr)},)
    return result


def save_pairs(inputs, recons, save_dir):
    """input_NNN.png / recon_NNN.png from byte frames [k,128,128,3] (PIL)."""
    from PIL import Image
    os.makedirs(save_dir, exist_ok=True)
    paths = []
    for i, (a, b) in enumerate(zip(inputs.cpu().numpy(), recons.cpu().numpy())):
        for name, frame in (("input", a), ("recon", b)):
            path = os.path.join(save_dir, "%s_%03d.png" % (name, i))
            Image.fromarray(frame).save(path)
            paths.append(path)
    return paths


def make_parser():
    parser = ArgumentParser(description="Reconstruction error (and reconstructions) of a trained image autoencoder")
    parser.add_argument("--encoder", required=True, help="whole-module checkpoint (encoder_N.pt of train_autoencoder.py)")
    parser.add_argument("--decoder", required=True, help="whole-module checkpoint (decoder_N.pt)")
    parser.add_argument("--data", required=True, help="trajectory directory, or synthetic:<N>:images|jpeg")
    parser.add_argument("--raw-jpeg", action="store_true",
                        help="read the directory's JPEG streams as they are and decode them on the GPU")
    parser.add_argument("--batch-size", type=int, default=16, help="trajectories per batch")
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--save-dir", default=None, help="write the first --num-save input / reconstruction pairs here as PNG")
    parser.add_argument("--num-save", type=int, default=8)
    parser.add_argument("--quality", action="store_true", help="also print the mean SSIM and PSNR of the reconstructions")
    return parser


def main(argv=None, log=print):
    args = make_parser().parse_args(argv)
    from .train_autoencoder import make_dataset
    device = torch.device(args.device)
    encoder, decoder = load_module(args.encoder, device), load_module(args.decoder, device)
    dataset = make_dataset(args.data, raw_jpeg=args.raw_jpeg)
    keep = args.num_save if args.save_dir else 0
    result = evaluate(encoder, decoder, dataset, batch_size=args.batch_size, device=device, keep=keep, quality=args.quality)
    mean = float(result[0].item())
    log("val_recon_loss:", mean, "frames:", int(result[1].numel()))
    if args.quality:
        log("val_recon_ssim:", float(result[-1]["mean_ssim"].item()), "val_recon_psnr:", float(result[-1]["mean_psnr"].item()))
    if args.save_dir:
        save_pairs(result[2][0], result[2][1], args.save_dir)
        log("wrote %d pairs to %s" % (int(result[2][0].shape[0]), args.save_dir))
    return mean


if __name__ == "__main__":
    main()
