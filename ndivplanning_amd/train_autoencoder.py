"""Autoencoder training script -- mirror of the reference's `train_autoencoder.py` (same constants, seeds, data loader,
per-step print and checkpoint files), with the loop body (train_autoencoder.py:79-90) replaced by
`AutoencoderTrainer.step`: forward, MSE, backward and Adam as gfx950 kernels (csrc/ndp_autoencoder.inc).

What differs from the reference, on purpose:
  * the constants are `train()`'s keyword arguments and `main()`'s command-line options, with the reference's values
    as defaults (data `128_128_data`, 16 trajectories per batch, shuffled, 50 epochs, lr 2e-4, betas (0.5, 0.999));
  * `synthetic:<N>:images` as the data path gives N seeded synthetic trajectories (the HDF5 loader needs h5py, see
    utils/trajectory_loader.py);
  * visdom is optional: with it importable (and `visdom=True`) the loss is plotted every `report_freq` steps;
  * `val_data` (`--val-data`): held-out trajectories.  At the end of every `val_every`-th epoch rank 0 writes the
    trainer's vectors into the modules, evaluates them in eval mode on the kernels (`autoencoder_eval.evaluate`), logs
    `epoch, "val_recon_loss:", value`, shows the first input and reconstruction through visdom as the reference does
    every 10 steps (train_autoencoder.py:96-103, win 1 / 2) and puts the modules back into training mode.  It draws no
    random number and changes nothing the trainer reads: the training losses are bit-identical with and without it.
    `val_quality` (`--val-quality`, default off) also logs `epoch, "val_ssim:", value, "val_psnr:", value`, the mean SSIM
    and PSNR of the reconstructions (`autoencoder_eval.evaluate(quality=True)`); the same holds.
  * `device_store` (`--device-store`, default off; needs a directory of .ndpt bundles, ndivplanning_amd/bundle.py) keeps
    the whole directory in device memory and assembles every batch there (trajectory_store.py) instead of going through
    a DataLoader: the same batches in the same order, decoded by the same JPEG decoder.
The whole modules are saved as models/encoder_{epoch}.pt / models/decoder_{epoch}.pt when epoch % 10 == 1
(train_autoencoder.py:92-97), after the trainer's flat vectors are written back into them.

More than one process (torch.distributed.run) trains data-parallel: `batch_size` is the GLOBAL trajectory count, every
rank takes batch_size / world_size trajectories of each (identically shuffled) batch, one GPU per local rank
(NDP_BENCH_ONE_GPU=1: all on cuda:0).  BatchNorm normalises over all ranks' images (`sync_batchnorm`, default on) and the
gradient is averaged bucket by bucket beside the backward pass (`grad_exchange="bucketed"`; "single": one collective
between backward and Adam), so W ranks train what one process trains on the whole batch.  A final batch that does not
split evenly is skipped; the per-step loss is the mean of the ranks' losses; rank 0 prints, plots and saves."""
import os
import warnings
from argparse import ArgumentParser

import numpy as np
import torch
import torch.distributed as dist

from . import _capi, dp
from . import _train_io as T
from ._train_io import denorm, norm  # noqa: F401
from .autoencoder_trainer import AutoencoderTrainer
from .models.image_autoencoder import Decoder, Encoder
from .utils.trajectory_loader import open_dataset

LR_RATE = 2e-4
NUM_EPOCHS = 50
BATCH_SIZE = 16
REPORT_FREQ = 10


def make_dataset(path, seed=1, raw_jpeg=False):
    """synthetic:<N>:images|jpeg, or the trajectory directory (HDF5 or .ndpt bundles; raw_jpeg: its JPEG streams, decoded
    on the device)."""
    return open_dataset(path, seq_length=15, seed=seed, default_mode="images", modes=("images", "jpeg"),
                        mode_error="the autoencoder trains on images: use synthetic:<N>:images or synthetic:<N>:jpeg",
                        push={"raw_jpeg": True} if raw_jpeg else None)


def build_models(device):
    """The reference's construction and initialisation order (train_autoencoder.py:54-57), on the seeded generator."""
    encoder = Encoder().to(device)
    decoder = Decoder().to(device)
    decoder.weight_init(mean=0.0, std=0.02)
    encoder.weight_init(mean=0.0, std=0.02)
    return encoder, decoder


def train(data_path="128_128_data", batch_size=BATCH_SIZE, num_epochs=NUM_EPOCHS, lr=LR_RATE, betas=(0.5, 0.999),
          device="cuda", save_dir="models", report_freq=REPORT_FREQ, visdom=False, log=print, sync_batchnorm=True,
          grad_exchange="bucketed", raw_jpeg=False, val_data=None, val_every=1, val_quality=False, device_store=False):
    """The reference's loop; returns (encoder, decoder, per-step losses).  Under torch.distributed.run: data parallel
    (module docstring); `device` is then the local rank's GPU, every rank returns the same losses."""
    if grad_exchange not in ("bucketed", "single"):
        raise ValueError("grad_exchange must be 'bucketed' or 'single', got %r" % (grad_exchange,))
    rank, world, local_rank = dp.env_world()
    if batch_size % world != 0:                                        # (before any process group or GPU is touched)
        raise ValueError("batch_size=%d trajectories must be a multiple of the %d ranks" % (batch_size, world))
    store_dir = None
    if device_store:
        from .trajectory_store import require_bundle_dir
        store_dir = require_bundle_dir(data_path, "device_store")
    if val_data is not None and int(val_every) < 1:
        raise ValueError("val_every must be >= 1, got %r" % (val_every,))
    own_group = False
    if world > 1:                                                      # (one process: the caller's `device`, not made current)
        own_group = not dist.is_initialized()                          # a group this call creates is torn down at its end
        device = T.open_device(world, local_rank, None)
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    # seeds first, then the dataset and the modules, as the reference's module-level code runs
    torch.manual_seed(1)
    np.random.seed(1)
    dataset = make_dataset(data_path, raw_jpeg=raw_jpeg)
    # JPEG frames are decoded on the device, then normalised by ndp_eval_frames_u8 (decode_images below)
    loader, jpeg_decoder = T.open_batch_source(dataset, batch_size, device, store_dir, dataset.seq_length, rank, world)
    val_dataset = make_dataset(val_data, seed=2, raw_jpeg=raw_jpeg) if val_data is not None and rank == 0 else None
    encoder, decoder = build_models(device)
    trainer, bucket_group = None, None
    try:
        if world > 1:
            T.broadcast_initial_weights([encoder, decoder])
            if grad_exchange == "bucketed" and sync_batchnorm:
                # with cross-rank statistics the buckets get a communicator of their own: on the statistics' one they
                # would queue behind the 8 backward statistics syncs, i.e. behind nearly the whole backward pass
                bucket_group = dist.new_group(list(range(world)))
        dp_kw = T.dp_trainer_kwargs(world, grad_exchange, sync_batchnorm, group=bucket_group,
                                    bucket_ranges=_capi.ae_grad_buckets, wait="ndp_ae_bucket_wait")
        trainer = AutoencoderTrainer(encoder.train(), decoder.train(), batch=batch_size // world * 15, lr=lr, betas=betas,
                                     **dp_kw)                          # (15 frames)
        display = None
        if visdom and rank == 0:
            try:
                from .vis_tools import visualizer
                display = visualizer(port=8082)
            except Exception as e:  # pragma: no cover - visdom is optional
                log("visdom unavailable (%s): no plots" % e)
        losses, val_losses, val_quality_log = [], [], []
        step = 0
        skipped = []

        def warn_ragged(rows):                                         # rank 0, the first time
            if rank == 0 and not skipped:
                warnings.warn("train_autoencoder: a final batch of %d trajectories does not split over %d ranks; skipped"
                              % (rows, world))
            skipped.append(rows)

        for epoch in range(num_epochs):
            for images, _, _, _ in T.rank_batches(loader, batch_size, rank, world, device_store, on_ragged=warn_ragged):
                images = T.upload_frames(images, device, jpeg_decoder, "decode_images", non_blocking=False)
                state_cur = images.view(-1, *(images.size()[2:])).contiguous()
                recon_loss = trainer.step(state_cur)
                step += 1
                if world > 1:                                          # the global batch's loss: the mean of the ranks'
                    mean = dp.reduce_loss_shares([recon_loss.item() / world], device=device)[0]
                    recon_loss = torch.tensor([mean], dtype=torch.float32)
                    if step == 1:
                        dp.assert_replicas_identical([trainer.params], grad_exchange, "after the first step")
                recon_loss_np = recon_loss.cpu().data.numpy()
                losses.append(float(recon_loss_np[0]))
                if rank == 0:
                    log(epoch, step, "recon_loss_np: ", recon_loss_np)
                if display is not None and step % report_freq == 0:
                    display.plot("recon_loss", "train", "autoencoder", step, float(recon_loss_np[0]))
            if jpeg_decoder is not None:
                jpeg_decoder.finish()
            if world > 1:
                dp.assert_replicas_identical([trainer.params], grad_exchange, "end of epoch %d" % epoch)
            if val_dataset is not None and (epoch + 1) % int(val_every) == 0:
                quality = {} if val_quality else None
                val_losses.append((epoch, validate(trainer, val_dataset, batch_size, device, display, quality=quality)))
                log(epoch, "val_recon_loss:", val_losses[-1][1])
                if val_quality:
                    val_quality_log.append((epoch, quality["mean_ssim"], quality["mean_psnr"]))
                    log(epoch, "val_ssim:", quality["mean_ssim"], "val_psnr:", quality["mean_psnr"])
            if epoch % 10 == 1 and rank == 0:
                os.makedirs(save_dir, exist_ok=True)
                trainer.sync_to_modules()
                torch.save(encoder, os.path.join(save_dir, "encoder_" + str(epoch) + ".pt"))
                torch.save(decoder, os.path.join(save_dir, "decoder_" + str(epoch) + ".pt"))
        trainer.sync_to_modules()
    finally:
        if trainer is not None:
            trainer.close()
        if bucket_group is not None:
            dist.destroy_process_group(bucket_group)
        if own_group and dist.is_initialized():
            dist.destroy_process_group()
    train.last_trainer = trainer                                       # tests: the replica's flat vectors
    train.last_val_losses = val_losses                                 # [(epoch, val_recon_loss)]
    train.last_val_quality = val_quality_log                           # [(epoch, val_ssim, val_psnr)] with val_quality
    return encoder, decoder, losses


def validate(trainer, val_dataset, batch_size, device, display=None, quality=None):
    """The mean reconstruction error of the trainer's current parameters over `val_dataset`, eval mode, on the kernels
    (autoencoder_eval.evaluate); with a visdom display also the first input and reconstruction (the reference's win 1 /
    2).  The modules come back in training mode; the trainer's own vectors are only read.  quality: None, or a dict that
    receives mean_ssim and mean_psnr of the reconstructions as host floats."""
    from . import autoencoder_eval
    encoder, decoder = trainer.sync_to_modules()
    encoder.eval()
    decoder.eval()
    try:
        result = autoencoder_eval.evaluate(encoder, decoder, val_dataset, batch_size=batch_size, device=device,
                                           keep=1 if display is not None else 0, quality=quality is not None)
        if quality is not None:
            quality.update(mean_ssim=float(result[-1]["mean_ssim"].item()), mean_psnr=float(result[-1]["mean_psnr"].item()))
        if display is not None:
            display.vis.image(result[2][0][0].permute(2, 0, 1).cpu().numpy(), win=1, opts={"caption": "state_cur_vis"})
            display.vis.image(result[2][1][0].permute(2, 0, 1).cpu().numpy(), win=2, opts={"caption": "state_cur_hat_vis"})
    finally:
        for m in (encoder.train(), decoder.train()):                   # the eval kernels' scratch goes back to the allocator
            m.__dict__.pop("_ndp_packed", None)
            m.__dict__.pop("_ndp_ws", None)
    return float(result[0].item())


def make_parser():
    parser = ArgumentParser(description="Train the image autoencoder (train_autoencoder.py)")
    parser.add_argument("--data", default="128_128_data", help="trajectory directory, or synthetic:<N>:images|jpeg")
    parser.add_argument("--raw-jpeg", action="store_true",
                        help="read the directory's JPEG streams as they are and decode them on the GPU")
    parser.add_argument("--device-store", action="store_true",
                        help="keep the directory's .ndpt bundles in GPU memory and assemble every batch there "
                             "(ndivplanning_amd/trajectory_store.py) instead of through a DataLoader")
    parser.add_argument("--batch-size", type=int, default=BATCH_SIZE,
                        help="trajectories per step (under torch.distributed.run: over all ranks)")
    parser.add_argument("--epochs", type=int, default=NUM_EPOCHS)
    parser.add_argument("--lr", type=float, default=LR_RATE)
    parser.add_argument("--save-dir", default="models")
    parser.add_argument("--val-data", default=None,
                        help="held-out trajectories (as --data): their reconstruction error is logged after every "
                             "--val-every-th epoch")
    parser.add_argument("--val-every", type=int, default=1)
    parser.add_argument("--val-quality", action="store_true",
                        help="with --val-data: also log val_ssim and val_psnr, the mean SSIM and PSNR of the reconstructions")
    parser.add_argument("--visdom", action="store_true", help="plot the loss through visdom")
    parser.add_argument("--no-sync-batchnorm", dest="sync_batchnorm", action="store_false",
                        help="data parallel: BatchNorm statistics per rank instead of over all ranks' images")
    parser.add_argument("--grad-exchange", choices=("bucketed", "single"), default="bucketed",
                        help="data parallel: average the gradient per bucket beside the backward pass, or in one "
                             "collective after it")
    return parser


def main(argv=None):
    args = make_parser().parse_args(argv)
    return train(args.data, batch_size=args.batch_size, num_epochs=args.epochs, lr=args.lr, save_dir=args.save_dir,
                 visdom=args.visdom, sync_batchnorm=args.sync_batchnorm, grad_exchange=args.grad_exchange,
                 raw_jpeg=args.raw_jpeg, val_data=args.val_data, val_every=args.val_every, val_quality=args.val_quality, device_store=args.device_store)


if __name__ == "__main__":
    main()
