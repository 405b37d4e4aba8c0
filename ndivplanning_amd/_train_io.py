"""What the training scripts share around their trainers (train_gan, train_forward_model, train_autoencoder): configuration
reads, the reference's class paths, the --config-file command line, the way from (world, local rank) to a device and a
process group, the way from a dataset to this rank's device batches, and a trainer's data-parallel arguments.  The
training sibling of _eval_io.py: nothing here launches a kernel, and nothing imports a training script."""
import importlib
import logging
import os

import torch
import torch.distributed as dist
from torch.utils import data

from . import dp
from . import jpeg as jpeg_frames
from ._eval_io import denorm, norm  # noqa: F401  (the scripts' `denorm` / `norm`)


def cfg_get(node, key, default):
    """node[key] of a DotMap / dict node, `default` where the key is absent.  A DotMap reads a missing key as an empty
    map, so None and {} are absences; False, 0 and "" are values."""
    value = node.get(key, None) if hasattr(node, "get") else None
    return default if value is None or (isinstance(value, dict) and not value) else value


def cfg_require(config, dotted):
    """The value at `a.b.c`, or a KeyError that names the key (float() / int() of the empty map a missing key reads as
    is a TypeError about the wrong thing)."""
    node = config
    for part in dotted.split("."):
        node = cfg_get(node, part, None)
    if node is None:
        raise KeyError("%s is missing from the config (the reference's config/default.yaml has it)" % dotted)
    return node


def bind_reference_class_paths(table):
    """table: {reference module name: classes}.  Whole-module checkpoints must record the classes under the paths the
    reference's evaluation scripts unpickle (control_evaluation.py:175-180), e.g. `models.gan.Decoder`.  The root-level
    shims with those names rename the classes when imported; do that here, so that every way into train() -- the CLI
    entry, the package, a test -- writes the same pickles.  Returns the names that could not be bound."""
    missing = []
    for name, classes in table.items():
        try:
            mod = importlib.import_module(name)
        except ImportError:
            mod = None
        for cls in classes:
            if mod is not None and getattr(mod, cls.__name__, None) is cls:
                cls.__module__ = name
            else:
                missing.append("%s.%s" % (name, cls.__name__))
    if missing:
        logging.warning("checkpoints will record ndivplanning_amd.* class paths: %s do(es) not resolve to this "
                        "implementation (is the repository root, with its models/ shims, on sys.path?)", ", ".join(missing))
    return missing


def config_main(train, argv=None):
    """main() of a script with the reference's --config-file command line: train(configuration with the command line's
    overrides and absolute paths).  (Not _eval_io.config_cli: the GPU check, and its message, are train()'s.)"""
    from argparse import ArgumentParser

    from .utils.argparse_util import override_dotmap
    from .utils.cli_arguments.common_arguments import add_common_arguments
    from .utils.file import make_paths_absolute
    args = add_common_arguments(ArgumentParser(description="Interact with your training script")).parse_args(argv)
    return train(make_paths_absolute(os.getcwd(), override_dotmap(args, "config_file"), log_not_exist=True))


def open_device(world, local_rank, single_device, one_gpu_rehearsal=True):
    """The device of this process, made current, with the process group of a data-parallel run on it: the local rank's
    GPU under torch.distributed.run (all ranks on cuda:0 with NDP_BENCH_ONE_GPU=1, where the script honours that
    rehearsal switch), else `single_device`, the script's own choice (an index or anything torch.device takes)."""
    if world > 1:
        single_device = 0 if one_gpu_rehearsal and os.environ.get("NDP_BENCH_ONE_GPU") == "1" else local_rank
    device = torch.device("cuda", single_device) if isinstance(single_device, int) else torch.device(single_device)
    torch.cuda.set_device(device)
    dp.init_process_group(device)
    return device


def open_batch_source(dataset, batch_size, device, device_store_dir, seq_length, rank, world):
    """(loader, jpeg_decoder) of an image trainer: a shuffling DataLoader over `dataset`, with a decoder if it yields JPEG
    streams (`synthetic:<N>:jpeg`, `raw_jpeg: true`: decoded on the device; failures raise one batch later, or at
    finish()).  device_store_dir: the directory's bundles stay in device memory and every batch is assembled there
    (trajectory_store.py) -- the same batches in the same order as the DataLoader's, this rank's rows only, decoded by
    the same kind of decoder."""
    if device_store_dir is not None:
        from .trajectory_store import DeviceTrajectoryStore, StoreLoader
        loader = StoreLoader(DeviceTrajectoryStore(device_store_dir, device), batch_size, 0, int(seq_length), shuffle=True,
                             rank=rank, world=world)
        return loader, jpeg_frames.JpegDecoder(device, check="deferred")
    loader = data.DataLoader(dataset, batch_size=batch_size, shuffle=True, **jpeg_frames.loader_kwargs(dataset))
    return loader, jpeg_frames.JpegDecoder(device, check="deferred") if jpeg_frames.is_jpeg(dataset) else None


def rank_batches(loader, batch_size, rank, world, presharded, on_ragged=None):
    """The loader's batches (tuples whose members have one row per trajectory) as this rank trains on them: its
    dp.shard_bounds rows of every batch of `batch_size`; a ragged final batch does not split evenly and is skipped on
    every rank (on_ragged(rows), if given).  One process, or presharded (a StoreLoader yields this rank's rows
    already): every batch as it comes."""
    if world == 1 or presharded:
        yield from loader
        return
    lo, hi = dp.shard_bounds(batch_size, rank, world)
    for batch in loader:
        if batch[0].shape[0] != batch_size:
            if on_ragged is not None:
                on_ragged(batch[0].shape[0])
            continue
        yield tuple(member[lo:hi] for member in batch)


def upload_frames(frames, device, jpeg_decoder=None, decode="decode_frames", non_blocking=True):
    """A batch's frames on the device as the kernels take them: JPEG streams decoded there (`decode`: the decoder's
    method), byte frames [B,T,128,128,3] uploaded as they are (the kernels normalise them as they read them), anything
    else as float32."""
    if jpeg_decoder is not None:
        frames = getattr(jpeg_decoder, decode)(frames)
    if frames.dtype != torch.uint8:
        frames = frames.float()
    return frames.to(device, non_blocking=non_blocking)


def broadcast_initial_weights(modules):
    """One set of initial weights in a data-parallel run: rank 0's parameters and buffers."""
    for module in modules:
        for t in [*module.parameters(), *module.buffers()]:
            dist.broadcast(t.data, src=0)


def dp_trainer_kwargs(world, grad_exchange, sync_batchnorm, **bucket_kwargs):
    """The data-parallel arguments of a FlatTrainer for one of `world` ranks ({} for one process).  The mean of the
    ranks' gradients is taken per gradient bucket on a communication stream while the backward pass is still running
    (grad_exchange "bucketed"; bucket_kwargs go to dp.BucketedMeanAllReduce) or as ONE collective between backward and
    Adam ("single"); two ranks give bit-identical parameters either way.  sync_batchnorm: BatchNorm normalises over all
    ranks' images (exact integer all-reduce of the statistics accumulators), so W ranks train the single-process step
    on the GLOBAL batch; off keeps the statistics per rank (torch DistributedDataParallel without SyncBatchNorm)."""
    if world == 1:
        return {}
    if grad_exchange == "single":
        return {"sync_batchnorm_world": world if sync_batchnorm else 1, "reduce_fn": dp.mean_all_reduce(world)}
    return {"sync_batchnorm_world": world if sync_batchnorm else 1,
            "bucket_reduce": dp.BucketedMeanAllReduce(world, **bucket_kwargs)}
