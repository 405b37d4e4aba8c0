"""GAN training script -- mirror of the reference's `train_gan.py` (same CLI, same YAML keys,
same `train(config)` entry point, same epoch log line and checkpoint files), with the loop
body (train_gan.py:115-207) replaced by `GanTrainer.step`: a few fused gfx950 kernels per
iteration, replayed from a HIP graph, with no host synchronisation inside an epoch.

What differs from the reference, on purpose:
  * the three `.cpu()` loss reads per step (train_gan.py:205-207) become one read per epoch
    of sums accumulated on the device;
  * dead work is gone: the K-fold image repeats that are never read (144-149), the back-prop
    through G inside the D step and the D weight gradients inside the G step (183, 202);
  * a ragged final batch is dropped (the reference hard-codes batch_size and crashes on it,
    train_gan.py:168-194);
  * noise comes from a counter-based generator on the device unless `training.gan.noise_source`
    is "cpu" (the reference's torch.FloatTensor(...).uniform_() stream);
  * more than one process (torch.distributed.run) trains data-parallel: `batch_size` is the
    GLOBAL batch, every rank takes batch_size / world_size trajectories of each batch
    (ndivplanning_amd/dp.py);
  * the forward-model checkpoints the reference loads and never uses (train_gan.py:79-86) are
    not loaded; visdom plotting is attempted only if visdom is importable.

Extra YAML keys (all optional): `train_data_path: synthetic:<N>[:codes|images|frames_u8|jpeg]` for seeded
synthetic trajectories, `training.gan.noise_source`, `training.gan.use_graph`,
`training.gan.steps_per_launch` (iterations per HIP-graph launch, default 16; the batches of one
launch are staged into separate input slots, the arithmetic is unchanged),
`training.gan.cache_codes` (default true: encode every trajectory once, the encoder being frozen).
In data-parallel runs each rank caches only the trajectories of its own shard positions, so the
cache fills over several epochs there.

Validation (optional): `training.gan.val_data_path` (held-out trajectories, the forms of `train_data_path`),
`val_every` (epochs, default 1) and `val_num_sample` (default `num_sample`).  At the end of every `val_every`-th
epoch rank 0 evaluates the live decoder and discriminator -- their parameters are views into the trainer's flat
buffers, nothing is copied -- with `gan_eval.evaluate` and logs `val_action_loss`, `val_best_action_loss`,
`val_div_loss` and `val_spread` on one line after the epoch line.  It changes no bit of training: the trajectories
are read by index, the noise comes from `ndp_uniform_noise` with a seed and buffers of its own (no generator that
training reads is drawn from, the trainer's noise counter and captured graph are not touched), and the modules go
back into training mode.  In a data-parallel run rank 0 evaluates alone and issues no collective while doing so;
the in-kernel gradient exchange waits with a 10 s time-out (dp.py), so after a validation epoch all ranks meet at
one barrier of the process group before any of them launches the next step.  Without the key nothing is added.
"""
import logging
import os

# HSA reads this when the runtime initialises (the first torch.cuda call below): dmabuf IPC is the only
# mode this platform's driver supports, and the peer-to-peer gradient exchange / RCCL need it
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils import data  # noqa: E402

from . import dp  # noqa: E402
from . import jpeg as jpeg_frames  # noqa: E402
from ._train_io import cfg_get, config_main, denorm, norm, open_device, upload_frames  # noqa: E402,F401
from ._train_io import bind_reference_class_paths as _bind  # noqa: E402
from .models.gan import Decoder, Discriminator  # noqa: E402
from .models.image_autoencoder import Encoder  # noqa: E402
from .trainer import GanTrainer  # noqa: E402
from .utils.trajectory_loader import open_dataset  # noqa: E402


def bind_reference_class_paths():
    """The whole-module checkpoints (train_gan.py:254-266) record `models.gan.Decoder` / `models.gan.Discriminator`, and
    the encoder `models.image_autoencoder.Encoder` (_train_io.bind_reference_class_paths)."""
    return _bind({"models.gan": (Decoder, Discriminator), "models.image_autoencoder": (Encoder,)})


def push_arguments(config):
    """PushDataset's keyword arguments as the trainers' configuration states them.  Decoded frames stay bytes until the
    first convolution reads them (ndp_encoder_forward_u8 / ndp_fm_*_u8): `raw_uint8: false` restores the reference's
    host-side float tensors; `raw_jpeg: true` yields the stored JPEG streams, decoded on the device (ndivplanning_amd.jpeg)."""
    return dict(seq_length=config.trajectory_length, raw_uint8=bool(cfg_get(config, "raw_uint8", True)),
                raw_jpeg=bool(cfg_get(config, "raw_jpeg", False)))


def make_dataset(config):
    return open_dataset(config.train_data_path, seq_length=config.trajectory_length, seed=int(config.random_seed),
                        default_mode="codes", push=push_arguments(config))


def load_encoder(config, device):
    """torch.load of the pretrained whole-module encoder pickle (train_gan.py:75-76).  A local,
    trusted file written by train_autoencoder.py: weights_only=False is required for module
    pickles.  Without a file (synthetic image runs) a seeded Encoder stands in."""
    path = cfg_get(config, "image_encoder_model_path", None)
    if path and os.path.isfile(path):
        enc = torch.load(path, map_location=device, weights_only=False)
    else:
        logging.warning("no image encoder checkpoint at %s: using a seeded random Encoder", path)
        torch.manual_seed(int(config.random_seed))
        enc = Encoder()
    return enc.to(device).eval()


def encode_batch(frames, encoder, seq_length):
    """codes [B*(T-1), 256] = cat(code(current frame), code(final frame)) (train_gan.py:127-155).
    `frames` is [B,T,3,H,W] images or [B,T,128] cached codes; the target frame is encoded once
    per trajectory instead of T-1 times."""
    b, t = frames.shape[0], frames.shape[1]
    if frames.dim() == 5:
        with torch.no_grad():
            per_frame = encoder(frames.reshape((b * t,) + tuple(frames.shape[2:]))).reshape(b, t, -1)
    else:
        per_frame = frames
    cur = per_frame[:, :-1]
    tgt = per_frame[:, -1:].expand(-1, t - 1, -1)
    return torch.cat([cur, tgt], dim=2).reshape(b * (t - 1), -1).contiguous()


# the validation noise's Philox key: apart from every trainer's (random_seed * 1000 + rank)
VAL_NOISE_SEED = 1 << 40


def make_val_dataset(config, path):
    """The held-out trajectories of `training.gan.val_data_path`, made as `make_dataset` makes the training set (same
    trajectory_length); a synthetic set is seeded apart from the training set."""
    return open_dataset(path, seq_length=config.trajectory_length, seed=int(config.random_seed) + 1, default_mode="codes",
                        push=push_arguments(config))


def validate(decoder, discriminator, encoder, val_dataset, num_sample, batch_size, seed, device):
    """gan_eval.evaluate on the live modules, logged; returns the means as host floats.  Rank 0 calls this alone: no
    collective is issued, no generator that training reads is drawn from, and the modules return to training mode."""
    from . import gan_eval
    decoder.eval()
    discriminator.eval()
    try:
        result = gan_eval.evaluate(decoder, val_dataset, encoder=encoder, discriminator=discriminator, num_sample=num_sample,
                                   batch_size=batch_size, seed=seed, device=device)
        means = {k: float(result[k].item()) for k in ("action_mse", "best_action_mse", "ndiv_per_row", "spread", "d_fake_prob",
                                                      "d_real_prob", "d_pick_mse")}
        means["best_of_k_curve"] = result["best_of_k_curve"].tolist()
    finally:
        decoder.train()
        discriminator.train()
    logging.info("val_action_loss: {} val_best_action_loss: {} val_div_loss: {} val_spread: {}".format(
        means["action_mse"], means["best_action_mse"], means["ndiv_per_row"], means["spread"]))
    return means


def epoch_batches(n_items, batch_size, generator):
    """Shuffled index batches of one epoch (ragged tail dropped): what DataLoader(shuffle=True,
    drop_last=True) does, as an explicit list so that cached epochs can follow the same order."""
    perm = torch.randperm(n_items, generator=generator)
    return [perm[i:i + batch_size] for i in range(0, n_items - batch_size + 1, batch_size)]


def train(config):
    g = config.training.gan
    random_seed = int(config.random_seed)
    num_epochs, num_sample, noise_dim = int(g.num_epochs), int(g.num_sample), int(g.noise_dim)
    batch_size, dsteps, epochs_per_stage = int(g.batch_size), int(g.discrim_steps_per_gen), int(g.epochs_per_stage)
    lr_rate = float(g.learning_rate)
    div_factor = cfg_get(g, "pairwise_div_factor", None)
    if div_factor is None or isinstance(div_factor, dict):
        raise KeyError("training.gan.pairwise_div_factor is missing from the config "
                       "(the reference fails at train_gan.py:199 for such a file)")
    noise_source = cfg_get(g, "noise_source", "device")
    use_graph = bool(cfg_get(g, "use_graph", True))
    steps_per_launch = int(cfg_get(g, "steps_per_launch", 16))
    cache_codes = bool(cfg_get(g, "cache_codes", True))
    val_path, val_every = cfg_get(g, "val_data_path", None), int(cfg_get(g, "val_every", 1))
    val_num_sample = int(cfg_get(g, "val_num_sample", num_sample))
    if val_path is not None and (val_every < 1 or not 1 <= val_num_sample <= 256):
        raise ValueError("training.gan.val_every must be >= 1 and val_num_sample in 1..256, got %r and %r"
                         % (val_every, val_num_sample))

    rank, world, local_rank = dp.env_world()
    if not torch.cuda.is_available():
        raise RuntimeError("train_gan needs a ROCm GPU: the HIP path has no CPU fallback")
    # (gpu_id wraps round the cards present; NDP_BENCH_ONE_GPU is not read here: LOCAL_RANK alone places the ranks)
    device = open_device(world, local_rank, int(cfg_get(config, "gpu_id", 0)) % max(torch.cuda.device_count(), 1),
                         one_gpu_rehearsal=False)
    if batch_size % world != 0:
        raise ValueError("training.gan.batch_size=%d must be a multiple of the %d ranks" % (batch_size, world))
    local_batch = batch_size // world

    torch.manual_seed(random_seed)          # train_gan.py:65-66: Decoder, then Discriminator, then shuffling
    np.random.seed(random_seed)
    bind_reference_class_paths()

    display = None
    if rank == 0 and cfg_get(config, "log_port", None):
        try:                                  # train_gan.py:68; needs a live visdom server
            from visdom import Visdom        # noqa: F401
            from .vis_tools import visualizer
            display = visualizer(port=config.log_port)
        except Exception as e:                # noqa: BLE001 - observability is optional
            logging.info("visdom plotting disabled (%s)", e)

    dataset = make_dataset(config)
    order_gen = torch.Generator().manual_seed(random_seed)
    n_batches = len(dataset) // batch_size
    if n_batches == 0:
        raise ValueError("dataset of %d trajectories is smaller than one batch of %d" % (len(dataset), batch_size))
    seq_length = int(dataset.seq_length)
    image_mode = getattr(dataset, "mode", "images") in ("images", "frames_u8", "jpeg")
    # JPEG frames (`synthetic:<N>:jpeg`, `raw_jpeg: true`) are decoded on the device; failures raise one batch later
    jpeg_decoder = jpeg_frames.JpegDecoder(device, check="deferred") if jpeg_frames.is_jpeg(dataset) else None
    encoder = load_encoder(config, device) if image_mode else None

    decoder = Decoder(noise_dim=noise_dim)
    discriminator = Discriminator()
    decoder.weight_init(mean=0.0, std=0.02)            # no-op on Linear layers, as in the reference
    discriminator.weight_init(mean=0.0, std=0.02)
    decoder, discriminator = decoder.to(device), discriminator.to(device)

    flat_local = local_batch * (seq_length - 1)
    # gradient exchange of a data-parallel run: summed inside the slab-reduce kernels over hipIpc-mapped
    # peer memory when that passes its self-check on this node (the step stays one graph), RCCL
    # all-reduce between the phases otherwise
    p2p, reduce_fn, exchange = dp.make_exchange(device, world, log=logging.info)
    if world > 1 and rank == 0:
        logging.info("data parallel over %d ranks, gradient exchange: %s", world, exchange)
    trainer = GanTrainer(decoder, discriminator, flat=flat_local, num_sample=num_sample, lr=lr_rate,
                         betas=(0.5, 0.999), pairwise_div_factor=float(div_factor), discrim_steps=dsteps,
                         flat_global=flat_local * world, reduce_fn=reduce_fn, p2p=p2p,
                         use_graph=use_graph, noise_seed=random_seed * 1000 + rank,
                         steps_per_launch=steps_per_launch if (reduce_fn is None and use_graph) else 1)
    group = trainer.nslots
    # The encoder is frozen (train_gan.py:75-76, .detach() at 152-153), so a frame's code never
    # changes: with `cache_codes` every trajectory is encoded (and its actions uploaded) once, in
    # the first epoch that meets it; later epochs gather codes and actions on the device and touch
    # neither the images nor the host.
    code_cache = action_cache = cached = None
    if cache_codes:
        code_cache = torch.zeros(len(dataset), seq_length, 128, device=device)
        action_cache = torch.zeros(len(dataset), seq_length, 4, device=device)
        cached = torch.zeros(len(dataset), dtype=torch.bool)
    # held-out trajectories (optional): rank 0 alone reads and evaluates them
    val_dataset = make_val_dataset(config, val_path) if val_path is not None and rank == 0 else None
    val_encoder = encoder
    if val_dataset is not None and encoder is None and getattr(val_dataset, "mode", "images") != "codes":
        rng_state = torch.get_rng_state()            # a seeded stand-in encoder draws from torch's generator: put it back
        val_encoder = load_encoder(config, device)
        torch.set_rng_state(rng_state)
    val_history = []
    history = []
    # Replicas apply the same Adam update to the same summed gradients, so their parameters must stay bit-identical.
    # The in-kernel exchange has its own time-out word, but a sum that arrived WRONG (a flag overtaking its data on a
    # transport it has not met) would train on silently: compare parameter checksums across ranks after the first
    # launch and at the end of every epoch (two 16-byte all-reduces); a mismatch raises on every rank.
    lockstep = {"checked_first_launch": world == 1}

    def check_lockstep(where):
        if world > 1:
            if p2p is not None:
                p2p.check()                  # a timed-out wait is an error, not a silent wrong sum
            dp.assert_replicas_identical([trainer.g_flat, trainer.d_flat], exchange, where)

    for epoch in range(num_epochs):
        discriminator.train()
        decoder.train()
        pending = []                         # up to `group` prepared batches -> one graph launch
        batches = epoch_batches(len(dataset), batch_size, order_gen)
        lo, hi = dp.shard_bounds(batch_size, rank, world)

        def flush():
            if len(pending) == group and group > 1:
                trainer.step_many(torch.stack([p[0] for p in pending]), torch.stack([p[1] for p in pending]),
                                  None if pending[0][2] is None else torch.stack([p[2] for p in pending]))
            else:
                for c_, a_, n_ in pending:
                    trainer.step(c_, a_, n_)
            del pending[:]
            if not lockstep["checked_first_launch"]:
                lockstep["checked_first_launch"] = True
                check_lockstep("after the first launch")

        all_cached = cached is not None and bool(cached.all())
        loader = None if all_cached else iter(data.DataLoader(dataset, batch_sampler=[b.tolist() for b in batches],
                                                              **jpeg_frames.loader_kwargs(dataset)))
        for idx in batches:
            if all_cached:
                mine = idx[lo:hi].to(device)
                per_frame, actions = code_cache[mine], action_cache[mine]
            else:
                frames, _states, actions, _goal = next(loader)
                frames = upload_frames(frames[lo:hi], device, jpeg_decoder)
                actions = actions[lo:hi].float().to(device, non_blocking=True)
                if frames.dim() == 5:
                    with torch.no_grad():
                        b_, t_ = frames.shape[0], frames.shape[1]
                        per_frame = encoder(frames.reshape((b_ * t_,) + tuple(frames.shape[2:]))).reshape(b_, t_, -1)
                else:
                    per_frame = frames
                if cached is not None:
                    mine = idx[lo:hi]
                    code_cache[mine.to(device)] = per_frame
                    action_cache[mine.to(device)] = actions
                    cached[mine] = True
            codes = encode_batch(per_frame, None, seq_length)
            acts = actions[:, :-1].reshape(-1, actions.size(-1))                # train_gan.py:137
            noise = None
            if noise_source == "cpu":                                           # train_gan.py:44
                # every rank has the same CPU generator state: draw the GLOBAL batch's noise, the single-process
                # stream, and keep this rank's rows (identical draws per rank would duplicate noise W-fold)
                noise = torch.FloatTensor(flat_local * world, num_sample, noise_dim).uniform_()
                noise = noise[rank * flat_local:(rank + 1) * flat_local].to(device)
            pending.append((codes, acts, noise))
            if len(pending) == group:
                flush()
        flush()
        if jpeg_decoder is not None:
            jpeg_decoder.finish()
        check_lockstep("end of epoch %d" % epoch)
        sums = dp.reduce_loss_shares(trainer.pop_loss_sums(), device=device)
        d_avg, g_avg, div_avg = (v / n_batches for v in sums)                   # train_gan.py:209-211
        history.append((d_avg, g_avg, div_avg))
        if rank == 0:
            logging.info("{}, D: {:4f}, G: {:4f}, div: {:4f}".format(epoch, d_avg, g_avg, div_avg))
            if display is not None:
                display.plot("gan", "discriminator", "GAN Loss", epoch, d_avg)
                display.plot("gan", "generator", "GAN Loss", epoch, g_avg)
                display.plot("pairwise_div", "loss", "Pairwise Divergence Loss", epoch, div_avg)
        if val_path is not None and (epoch + 1) % val_every == 0:
            if val_dataset is not None:
                means = validate(decoder, discriminator, val_encoder, val_dataset, val_num_sample, local_batch,
                                 VAL_NOISE_SEED + random_seed, device)
                val_history.append((epoch, means))
                if display is not None:
                    display.plot("val_action", "mean", "Validation Action Loss", epoch, means["action_mse"])
                    display.plot("val_action", "best", "Validation Action Loss", epoch, means["best_action_mse"])
                    display.plot("val_div", "loss", "Validation Pairwise Divergence Loss", epoch, means["ndiv_per_row"])
                    display.plot("val_div", "spread", "Validation Pairwise Divergence Loss", epoch, means["spread"])
            if world > 1:                    # rank 0 evaluated alone: meet before any rank launches the next step
                dp.dist.barrier()
        if rank == 0 and epoch % epochs_per_stage == epochs_per_stage - 1:      # train_gan.py:249-266
            os.makedirs(config.gan_save_path, exist_ok=True)
            torch.cuda.synchronize(device)
            torch.save(discriminator, os.path.join(config.gan_save_path, "gan_discriminator_{}.pt".format(epoch)))
            torch.save(decoder, os.path.join(config.gan_save_path, "gan_decoder_{}.pt".format(epoch)))
    train.last_params = (trainer.g_flat, trainer.d_flat)               # tests: the replica's flat vectors
    train.last_val = val_history                                       # [(epoch, {action_mse, best_action_mse, ...})]
    if p2p is not None:
        del trainer
        p2p.close()
    return history


def main(argv=None):
    return config_main(train, argv)


if __name__ == "__main__":
    main()
