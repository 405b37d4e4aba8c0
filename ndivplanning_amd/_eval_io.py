"""What the evaluation entry points share in front of and behind their kernels (evaluation.py and its scripts,
gan_eval, forward_model_eval, autoencoder_eval, image_quality, push_world's `mpc`): the command line with a
--config-file, the whole-module checkpoints, the way from a dataset to device batches, the fp64 mean of fp32 values, and
the argument checks of the two image evaluations.  Nothing here launches a kernel, and nothing imports `evaluation`."""
import importlib
import os

import torch

from . import _capi
from . import jpeg as jpeg_frames

OUTPUTS = ("float", "bytes")
FM_PRECISIONS = ("fp32", "bf16")    # NDP_FM_FP32, NDP_FM_BF16 (include/ndp.h): the operand precision of an eval-mode pass


def fm_precision_code(name):
    """'fp32' / 'bf16' -> NDP_FM_FP32 / NDP_FM_BF16; anything else is a ValueError that lists the two names."""
    if not isinstance(name, str) or name not in FM_PRECISIONS:
        raise ValueError("fm_precision must be 'fp32' or 'bf16', got %r" % (name,))
    return FM_PRECISIONS.index(name)


def fm_precision_of(config):
    """The forward model's operand precision for an evaluation script: --fm-precision (a top-level key, as every command
    line argument becomes one), else the config's `evaluation.fm_precision`, else 'fp32'.  Checked."""
    name = config.get("fm_precision") if hasattr(config, "get") else None
    if name is None:
        ev = config.get("evaluation") if hasattr(config, "get") else None
        name = ev.get("fm_precision") if ev is not None and hasattr(ev, "get") else None
    name = "fp32" if name is None else name
    fm_precision_code(name)
    return name


ENC_PRECISIONS = ("fp32", "bf16")   # NDP_ENC_FP32, NDP_ENC_BF16 (include/ndp.h): the image encoder's pass in EvalModels.encode


def enc_precision_code(name):
    """'fp32' / 'bf16' -> NDP_ENC_FP32 / NDP_ENC_BF16; anything else is a ValueError that lists the two names."""
    if not isinstance(name, str) or name not in ENC_PRECISIONS:
        raise ValueError("enc_precision must be 'fp32' or 'bf16', got %r" % (name,))
    return ENC_PRECISIONS.index(name)


def enc_precision_of(config):
    """The image encoder's precision for an evaluation script: --enc-precision (a top-level key), else the config's
    `evaluation.enc_precision`, else 'fp32'.  Checked."""
    name = config.get("enc_precision") if hasattr(config, "get") else None
    if name is None:
        ev = config.get("evaluation") if hasattr(config, "get") else None
        name = ev.get("enc_precision") if ev is not None and hasattr(ev, "get") else None
    name = "fp32" if name is None else name
    enc_precision_code(name)
    return name


def _check_out(out):
    if out not in OUTPUTS:
        raise ValueError("out must be 'float' or 'bytes', got %r" % (out,))


def _require_gpu(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise _capi.NdpError("%s is on %s: ndivplanning_amd computes only on a ROCm GPU (no CPU fallback)" % (name, t.device))
    return t


def _require_eval(**modules):
    for name, m in modules.items():
        if m.training:
            raise _capi.NdpError("the %s is in training mode: call .eval() first (these are the eval-mode kernels)" % name)


def denorm(tensor):
    """[-1, 1] -> [0, 255]: the reference's helper, which its training and evaluation scripts each define."""
    return ((tensor + 1.0) / 2.0) * 255.0


def norm(image):
    return (image / 255.0 - 0.5) * 2.0


def _to_bytes(frames):
    """Input frames as displayable bytes HWC: byte frames as they are, floats denormalised as the reference does."""
    if frames.dtype == torch.uint8:
        return frames
    return denorm(frames).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def fp64_mean(values, dim=None):
    """float32 [1] (dim None), or one value per column ([K] for dim=0 of [n,K]): the mean of the fp32 values, taken in
    fp64.  No value is skipped: an infinite PSNR gives an infinite mean."""
    values = values.double()
    return (values.mean() if dim is None else values.mean(dim=dim)).float().reshape(-1)


def _load(path, map_location):
    # a local, trusted whole-module pickle written by the training scripts: weights_only=False is required
    return torch.load(path, map_location=map_location, weights_only=False)


def load_module(path, device):
    """torch.load of a whole-module checkpoint of train_gan.py, train_autoencoder.py or train_forward_model.py, in eval
    mode on `device`.  The checkpoints name their classes `models.gan.*`, `models.image_autoencoder.*` and
    `models.forward_encoder.ForwardAutoencoder`: the root-level shims of those names are imported first where they are
    on sys.path."""
    for name in ("models.gan", "models.image_autoencoder", "models.forward_encoder"):
        try:
            importlib.import_module(name)
        except ImportError:
            pass
    return _load(path, "cpu").to(device).eval()


def device_of(config):
    gpu = config.gpu_id
    return torch.device("cuda", gpu) if isinstance(gpu, int) else torch.device(gpu)


def load_eval_models(config):
    """(image_encoder, generator, fwd_model_autoencoder, device): the three whole-module pickles the configuration names,
    loaded onto its gpu_id, in the mode they were saved in."""
    device = device_of(config)
    return (_load(config.image_encoder_model_path, device), _load(config.gan_decoder_model_path, device),
            _load(config.forward_model_autoencoder_path, device), device)


def config_cli(parser, argv, what, prepare=None):
    """The front of a command line with a --config-file (`parser` has the common arguments): parse, then
    prepare(namespace) (after parsing, before anything is read or loaded), the configuration with the command line's
    overrides and absolute paths, and the GPU check (`what` needs one).  Returns (namespace, config, what prepare
    returned)."""
    from .utils.argparse_util import override_dotmap
    from .utils.file import make_paths_absolute
    namespace = parser.parse_args(argv)
    prepared = prepare(namespace) if prepare is not None else None
    config = make_paths_absolute(os.getcwd(), override_dotmap(namespace, "config_file"), log_not_exist=True)
    if not torch.cuda.is_available():
        raise _capi.NdpError("%s needs a ROCm GPU; there is no CPU path" % what)
    return namespace, config, prepared


def trajectory_batches(dataset, batch_size, device, jpeg_decoder, first=None, actions=True):
    """(frames [b,T,...], actions [b,T,4] float32 or None, b) for `batch_size` trajectories at a time, as the kernels take
    them: cached codes [b,T,128], float images NCHW, or byte frames HWC for a dataset that yields bytes or JPEG streams
    (`jpeg_decoder`: the dataset's deferred `JpegDecoder`, None for any other dataset); bytes are never converted.
    `first`: dataset[0] where the caller has read it already.  The trajectories are read by index in order -- no
    DataLoader, so no random number of the process is drawn (validation inside a training run must not move its
    shuffling)."""
    for lo in range(0, len(dataset), batch_size):
        items = [first if i == 0 and first is not None else dataset[i] for i in range(lo, min(lo + batch_size, len(dataset)))]
        acts = torch.stack([torch.as_tensor(it[2]) for it in items]).to(device, non_blocking=True).float() if actions else None
        if jpeg_decoder is not None:
            buffer, offsets = jpeg_frames.pack_jpegs([s for it in items for s in it[0]])
            frames = jpeg_decoder.decode(buffer, offsets)
            frames = frames.view(len(items), -1, *frames.shape[1:])
        else:
            frames = torch.stack([it[0] for it in items]).to(device, non_blocking=True)
            if frames.dtype != torch.uint8:
                frames = frames.float()
        yield frames, acts, len(items)
