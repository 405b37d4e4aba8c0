"""Autoencoder training script -- mirror of the reference's `train_autoencoder.py` (same constants, seeds, data loader,
per-step print and checkpoint files), with the loop body (train_autoencoder.py:79-90) replaced by
`AutoencoderTrainer.step`: forward, MSE, backward and Adam as gfx950 kernels (csrc/ndp_autoencoder.inc).

What differs from the reference, on purpose:
  * the constants are `train()`'s keyword arguments and `main()`'s command-line options, with the reference's values
    as defaults (data `128_128_data`, 16 trajectories per batch, shuffled, 50 epochs, lr 2e-4, betas (0.5, 0.999));
  * `synthetic:<N>:images` as the data path gives N seeded synthetic trajectories (the HDF5 loader needs h5py, see
    utils/trajectory_loader.py);
  * visdom is optional: with it importable (and `visdom=True`) the loss is plotted every `report_freq` steps.
The whole modules are saved as models/encoder_{epoch}.pt / models/decoder_{epoch}.pt when epoch % 10 == 1
(train_autoencoder.py:92-97), after the trainer's flat vectors are written back into them."""
import os
from argparse import ArgumentParser

import numpy as np
import torch
from torch.utils import data

from .autoencoder_trainer import AutoencoderTrainer
from .models.image_autoencoder import Decoder, Encoder
from .utils.trajectory_loader import PushDataset, SyntheticPushDataset

LR_RATE = 2e-4
NUM_EPOCHS = 50
BATCH_SIZE = 16
REPORT_FREQ = 10


def denorm(tensor):
    return ((tensor + 1.0) / 2.0) * 255.0


def norm(image):
    return (image / 255.0 - 0.5) * 2.0


def make_dataset(path, seed=1):
    path = str(path)
    if path.startswith("synthetic:"):
        spec = path.split(":")
        mode = spec[2] if len(spec) > 2 else "images"
        if mode != "images":
            raise ValueError("the autoencoder trains on images: use synthetic:<N>:images")
        return SyntheticPushDataset(int(spec[1]), seq_length=15, mode="images", seed=seed)
    return PushDataset(path)


def build_models(device):
    """The reference's construction and initialisation order (train_autoencoder.py:54-57), on the seeded generator."""
    encoder = Encoder().to(device)
    decoder = Decoder().to(device)
    decoder.weight_init(mean=0.0, std=0.02)
    encoder.weight_init(mean=0.0, std=0.02)
    return encoder, decoder


def train(data_path="128_128_data", batch_size=BATCH_SIZE, num_epochs=NUM_EPOCHS, lr=LR_RATE, betas=(0.5, 0.999),
          device="cuda", save_dir="models", report_freq=REPORT_FREQ, visdom=False, log=print):
    """The reference's loop; returns (encoder, decoder, per-step losses)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    # seeds first, then the dataset and the modules, as the reference's module-level code runs
    torch.manual_seed(1)
    np.random.seed(1)
    dataset = make_dataset(data_path)
    loader = data.DataLoader(dataset, batch_size=batch_size, shuffle=True)
    encoder, decoder = build_models(device)
    trainer = AutoencoderTrainer(encoder.train(), decoder.train(), batch=batch_size * 15, lr=lr, betas=betas)   # (15 frames)
    display = None
    if visdom:
        try:
            from .vis_tools import visualizer
            display = visualizer(port=8082)
        except Exception as e:  # pragma: no cover - visdom is optional
            log("visdom unavailable (%s): no plots" % e)
    losses = []
    step = 0
    for epoch in range(num_epochs):
        for i, inputs in enumerate(loader):
            images, _, _, _ = inputs
            images = images.to(device)
            state_cur = images.view(-1, *(images.size()[2:])).contiguous()
            recon_loss = trainer.step(state_cur)
            step += 1
            recon_loss_np = recon_loss.cpu().data.numpy()
            losses.append(float(recon_loss_np[0]))
            log(epoch, step, "recon_loss_np: ", recon_loss_np)
            if display is not None and step % report_freq == 0:
                display.plot("recon_loss", "train", "autoencoder", step, float(recon_loss_np[0]))
        if epoch % 10 == 1:
            os.makedirs(save_dir, exist_ok=True)
            trainer.sync_to_modules()
            torch.save(encoder, os.path.join(save_dir, "encoder_" + str(epoch) + ".pt"))
            torch.save(decoder, os.path.join(save_dir, "decoder_" + str(epoch) + ".pt"))
    trainer.sync_to_modules()
    return encoder, decoder, losses


def main(argv=None):
    parser = ArgumentParser(description="Train the image autoencoder (train_autoencoder.py)")
    parser.add_argument("--data", default="128_128_data", help="trajectory directory, or synthetic:<N>:images")
    parser.add_argument("--batch-size", type=int, default=BATCH_SIZE, help="trajectories per step")
    parser.add_argument("--epochs", type=int, default=NUM_EPOCHS)
    parser.add_argument("--lr", type=float, default=LR_RATE)
    parser.add_argument("--save-dir", default="models")
    parser.add_argument("--visdom", action="store_true", help="plot the loss through visdom")
    args = parser.parse_args(argv)
    return train(args.data, batch_size=args.batch_size, num_epochs=args.epochs, lr=args.lr, save_dir=args.save_dir,
                 visdom=args.visdom)


if __name__ == "__main__":
    main()
