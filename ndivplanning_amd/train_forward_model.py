"""Forward-model training script -- mirror of the reference's `train_forward_model.py` (same CLI, same YAML keys
`training.forward.*`, same `train(config)` entry point, epoch log line and checkpoint files), with the loop body
(train_forward_model.py:98-112) replaced by `ForwardModelTrainer.step`: forward, MSE, backward and Adam as gfx950
kernels (csrc/ndp_forward_model.inc).

What differs from the reference, on purpose:
  * the per-step `loss.cpu()` read (train_forward_model.py:113-114) becomes one read per epoch of a sum kept on the
    device;
  * the StepLR scheduler the reference constructs and never steps (train_forward_model.py:86) is not constructed;
  * visdom image panels are attempted only if visdom is importable;
  * `train_data_path: synthetic:<N>` gives seeded synthetic trajectories (the HDF5 loader needs h5py, see
    utils/trajectory_loader.py);
  * more than one process (torch.distributed.run) trains data-parallel: `batch_size` is the GLOBAL batch, every rank
    takes batch_size / world_size trajectories of each (identically shuffled) batch, the flat gradient is averaged over
    RCCL between backward and Adam (ndivplanning_amd/dp.py::mean_all_reduce).  BatchNorm statistics are per rank, as with
    torch's DistributedDataParallel; a final batch that does not split evenly is dropped; rank 0 saves.
  * three optional keys, `training.forward.val_data_path` (held-out trajectories: a directory or `synthetic:<N>[:mode]`),
    `val_every` (epochs, default 1) and `val_horizon` (default 1): at the end of every `val_every`-th epoch rank 0 writes
    the trainer's flat vectors into the module (they are the source of truth and are never read back), evaluates it in
    eval mode on the kernels (`forward_model_eval.evaluate`) and logs `val_pred_loss` (the one-step error) and
    `val_persistence_loss` (the error of "the frame does not change"), then one line per further horizon.  Validation
    changes no bit of training: it reads the trajectories by index (no random number is drawn), the forward pass is in
    eval mode (the running statistics are read, never moved; the cross-rank BatchNorm hook belongs to training-mode
    calls and is not invoked), it issues no collective -- the other ranks simply meet rank 0 at the next epoch's first
    all-reduce -- and the module is back in training mode afterwards.  Without `val_data_path` nothing changes.
    `training.forward.val_quality` (default off) also logs `val_ssim` and `val_psnr` (`forward_model_eval.evaluate(
    quality=True)`), with their persistence values; the same argument holds, training stays bit-identical.
  * `training.forward.rollout_steps` (default 1: the loop above, bit for bit): with H > 1 the inner loop runs over the
    windows of H + 1 frames, `ForwardModelTrainer.step_rollout` unrolls the model H steps on its own predictions and
    takes one Adam step on the mean of the H step losses, differentiated through every path; `step` and the epoch's
    average count windows.  One process only.
The whole module is saved every `epochs_per_stage` epochs as the reference does (train_forward_model.py:151-163), after
the trainer's flat vectors are written back into it."""
import logging
import os

import numpy as np
import torch

from . import _train_io as T
from . import dp
from ._train_io import cfg_get, cfg_require, denorm, norm  # noqa: F401
from .forward_trainer import ForwardModelTrainer
from .models.forward_encoder import Decoder, Encoder, ForwardAutoencoder
from .train_gan import make_dataset, push_arguments
from .utils.trajectory_loader import open_dataset


def bind_reference_class_paths():
    """The whole-module checkpoints record `models.forward_encoder.ForwardAutoencoder` (/ Encoder / Decoder), the path
    the reference's evaluation scripts unpickle (control_evaluation.py:177-180; _train_io.bind_reference_class_paths)."""
    return T.bind_reference_class_paths({"models.forward_encoder": (ForwardAutoencoder, Encoder, Decoder)})


def train(config):
    for key in ("num_epochs", "learning_rate", "batch_size", "epochs_per_stage"):
        cfg_require(config, "training.forward." + key)
    for key in ("random_seed", "train_data_path", "forward_save_path"):
        cfg_require(config, key)
    f = config.training.forward
    random_seed = int(config.random_seed)
    lr_rate, num_epochs, batch_size = float(f.learning_rate), int(f.num_epochs), int(f.batch_size)
    epochs_per_stage = int(f.epochs_per_stage)
    store_dir = None
    if bool(cfg_get(f, "device_store", False)):                      # (before any GPU or process group is touched)
        from .trajectory_store import require_bundle_dir
        store_dir = require_bundle_dir(config.train_data_path, "training.forward.device_store")
    rank, world, local_rank = dp.env_world()
    rollout_steps = cfg_get(f, "rollout_steps", 1)                  # (checked before any GPU or process group is touched)
    if isinstance(rollout_steps, bool) or int(rollout_steps) != rollout_steps or int(rollout_steps) < 1:
        raise ValueError("training.forward.rollout_steps must be an integer >= 1, got %r" % (rollout_steps,))
    rollout_steps = int(rollout_steps)
    trajectory_length = cfg_get(config, "trajectory_length", None)
    if trajectory_length is not None and int(trajectory_length) < rollout_steps + 1:
        raise ValueError("training.forward.rollout_steps=%d needs windows of %d frames, trajectory_length is %d"
                         % (rollout_steps, rollout_steps + 1, int(trajectory_length)))
    if rollout_steps > 1 and world > 1:
        raise ValueError("training.forward.rollout_steps=%d with %d ranks: multi-step rollouts train on one process (the "
                         "bucketed gradient exchange and the cross-rank BatchNorm statistics assume one pass per iteration)"
                         % (rollout_steps, world))
    if not torch.cuda.is_available():
        from . import _capi
        raise _capi.NdpError("train_forward_model needs a ROCm GPU (gpu_id %r); there is no CPU path" % (config.gpu_id,))
    device = T.open_device(world, local_rank, config.gpu_id)
    if batch_size % world != 0:
        raise ValueError("training.forward.batch_size=%d must be a multiple of the %d ranks" % (batch_size, world))
    local_batch = batch_size // world
    bind_reference_class_paths()
    torch.manual_seed(random_seed)                                   # train_forward_model.py:60-61
    np.random.seed(random_seed)
    display = None
    try:
        from .vis_tools import visualizer                            # optional (visdom)
        display = visualizer(port=config.log_port)
    except Exception:                                                # pragma: no cover - depends on the image
        display = None

    dataset = make_dataset(config)
    if getattr(dataset, "mode", "images") not in ("images", "frames_u8", "jpeg"):
        raise ValueError("the forward model trains on images: use `synthetic:<N>:images` or an HDF5 directory")
    if dataset.seq_length < rollout_steps + 1:                       # (a config without trajectory_length)
        raise ValueError("training.forward.rollout_steps=%d needs windows of %d frames, the trajectories have %d"
                         % (rollout_steps, rollout_steps + 1, dataset.seq_length))
    loader, jpeg_decoder = T.open_batch_source(dataset, batch_size, device, store_dir, trajectory_length, rank, world)

    model = ForwardAutoencoder().to(device)                          # train_forward_model.py:67-70
    model.decoder.weight_init(mean=0.0, std=0.02)
    model.encoder.weight_init(mean=0.0, std=0.02)
    model.train()
    if world > 1:
        T.broadcast_initial_weights([model])
    # data parallel (`batch_size` is the GLOBAL batch): `training.forward.grad_exchange` bucketed (default) or single,
    # `training.forward.sync_batchnorm` (default on; off: 20 fewer small collectives per step), see dp_trainer_kwargs.
    # The buckets share the statistics' process group.
    exchange = str(cfg_get(f, "grad_exchange", "bucketed"))
    if exchange not in ("bucketed", "single"):
        raise ValueError("training.forward.grad_exchange must be 'bucketed' or 'single', got %r" % (exchange,))
    trainer = ForwardModelTrainer(model, batch=local_batch, lr=lr_rate, betas=(0.5, 0.999), rollout_steps=rollout_steps,
                                  **T.dp_trainer_kwargs(world, exchange, bool(cfg_get(f, "sync_batchnorm", True))))

    # held-out trajectories (optional): rank 0 alone reads and evaluates them
    val_path, val_every, val_horizon = cfg_get(f, "val_data_path", None), int(cfg_get(f, "val_every", 1)), int(cfg_get(f, "val_horizon", 1))
    if val_path is not None and (val_every < 1 or val_horizon < 1):
        raise ValueError("training.forward.val_every and val_horizon must be >= 1, got %r and %r" % (val_every, val_horizon))
    val_quality = bool(cfg_get(f, "val_quality", False))
    val_dataset = make_val_dataset(config, val_path) if val_path is not None and rank == 0 else None
    val_history = []

    history = []
    step = 0
    for epoch in range(num_epochs):
        trainer.loss_sum.zero_()
        pairs = 0
        for images, _, actions, _ in T.rank_batches(loader, batch_size, rank, world, presharded=store_dir is not None):
            images = T.upload_frames(images, device, jpeg_decoder)
            actions = actions.to(device, non_blocking=True).float()
            if rollout_steps > 1:
                # windows of rollout_steps + 1 frames: the model is unrolled on its own predictions and trained through them
                for image_num in range(dataset.seq_length - rollout_steps):
                    trainer.step_rollout(images[:, image_num:image_num + rollout_steps + 1],
                                         actions[:, image_num:image_num + rollout_steps])
                    step += 1
                    pairs += 1
                continue
            for image_num in range(dataset.seq_length - 1):          # train_forward_model.py:98-112
                trainer.step(images[:, image_num].contiguous(), images[:, image_num + 1].contiguous(),
                             actions[:, image_num].contiguous())
                step += 1
                pairs += 1
        if jpeg_decoder is not None:
            jpeg_decoder.finish()
        avg_loss = float(trainer.loss_sum.item()) / max(pairs, 1)    # (seq_length - 1) * len(loader) terms
        if world > 1:
            avg_loss = dp.reduce_loss_shares([avg_loss / world], device=device)[0]
        history.append(avg_loss)
        if display is not None:                                      # pragma: no cover
            display.plot("loss", "train", "Forward Model Loss", epoch, avg_loss)
        logging.info("{}, {}: reconstruction loss per epoch: {}".format(epoch, step, avg_loss))
        if val_dataset is not None and (epoch + 1) % val_every == 0:
            val_history.append((epoch, validate(trainer, val_dataset, val_horizon, local_batch, quality=val_quality)))
        if epoch % epochs_per_stage == epochs_per_stage - 1 and rank == 0:   # train_forward_model.py:151-163
            os.makedirs(config.forward_save_path, exist_ok=True)
            trainer.sync_to_module()
            torch.cuda.synchronize(device)
            torch.save(model, os.path.join(config.forward_save_path, "forward_autoencoder_{}.pt".format(str(epoch))))
    trainer.sync_to_module()
    trainer.close()
    train.last_trainer = trainer                                       # tests: the replica's flat vectors
    train.last_val = val_history                                       # [(epoch, {one_step_mse, horizon_mse, persistence_mse, counts})]
    return history


def make_val_dataset(config, path):
    """The held-out trajectories of `training.forward.val_data_path`, made as `make_dataset` makes the training set
    (same trajectory_length and frame format); a synthetic set is seeded apart from the training set."""
    return open_dataset(path, seq_length=config.trajectory_length, seed=int(config.random_seed) + 1, default_mode="images",
                        modes=("images", "frames_u8", "jpeg"), push=push_arguments(config),
                        mode_error="the forward model is validated on images: use `synthetic:<N>:images`, `:frames_u8` or `:jpeg`")


def validate(trainer, val_dataset, horizon, batch_size, quality=False):
    """The prediction error of the trainer's current parameters over `val_dataset`, in eval mode on the kernels
    (forward_model_eval.evaluate), logged; returns the means as host lists.  The trainer's flat vectors are the source of
    truth: they are written into the module first and nothing is read back, no random number is drawn, no collective
    is issued (rank 0 calls this alone), and eval mode neither moves the running statistics nor invokes the cross-rank
    BatchNorm hook, which belongs to training-mode calls.  The module returns to training mode.  quality: also SSIM and
    PSNR per horizon (horizon_ssim, horizon_psnr, persistence_ssim, persistence_psnr), logged as val_ssim / val_psnr."""
    from . import forward_model_eval
    model = trainer.sync_to_module()
    model.eval()
    try:
        result = forward_model_eval.evaluate(model, val_dataset, horizon=horizon, batch_size=batch_size, device=trainer.device,
                                             quality=quality)
        keys = ("one_step_mse", "horizon_mse", "persistence_mse", "counts")
        if quality:
            keys += ("horizon_ssim", "horizon_psnr", "persistence_ssim", "persistence_psnr")
        means = {k: result[k].tolist() for k in keys}
    finally:
        model.train()
        model.invalidate_cache()                                       # the eval pass's scratch goes back to the allocator
    logging.info("val_pred_loss: {} val_persistence_loss: {}".format(means["one_step_mse"][0], means["persistence_mse"][0]))
    for h in range(1, len(means["horizon_mse"])):
        logging.info("val horizon {}: model_mse {} persistence_mse {} count {}".format(
            h + 1, means["horizon_mse"][h], means["persistence_mse"][h], means["counts"][h]))
    if quality:
        for h in range(len(means["horizon_ssim"])):
            logging.info("val horizon {}: val_ssim: {} val_psnr: {} persistence_ssim {} persistence_psnr {}".format(
                h + 1, means["horizon_ssim"][h], means["horizon_psnr"][h], means["persistence_ssim"][h],
                means["persistence_psnr"][h]))
    return means


def main(argv=None):
    return T.config_main(train, argv)


if __name__ == "__main__":
    main()
