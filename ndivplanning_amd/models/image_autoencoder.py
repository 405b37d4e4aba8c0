"""Image autoencoder -- mirror of the reference's `models/image_autoencoder.py` (image_autoencoder.py:14-87).

`Encoder`: 5 x conv3x3 stride 2 (BatchNorm only after the first three; conv4_bn / conv5_bn exist as attributes but are
not applied) + a 4x4 conv to 128 channels; 3x128x128 -> 128x1x1.  `Decoder`: deconv1 (128 -> 1024, 4x4 on the 1x1 code),
deconv2..5 (ConvTranspose2d(c, c/2, 4, 2, 1)), each + BatchNorm + ReLU, deconv6 (64 -> 3) + tanh.  Same attribute names,
state_dict keys and `weight_init` as the reference, so that its whole-module pickles load.

On the GAN path the encoder runs in eval mode ahead of the step and its output is detached (train_gan.py:75-76,
152-153): that case -- CUDA input, eval mode, input without grad -- goes through the gfx950 kernels of
`csrc/ndp_encoder.inc` (`ndp_encoder_forward`: implicit-GEMM convolutions on the fp32 matrix pipe, BatchNorm folded into
the weights).  Training both modules (train_autoencoder.py) goes through `ndivplanning_amd.autoencoder_trainer`
(`ndp_ae_train_grads` / `ndp_ae_apply_adam`, csrc/ndp_autoencoder.inc), which owns the flat vectors `pack_autoencoder`
builds.  The eval-mode `Decoder` -- eval mode, CUDA float32 codes [n,128,1,1], nothing for autograd to record -- runs on
`ndp_ae_decode`: the five BatchNorms folded into the transposed convolutions on the host (`fold_decoder_params`), the
chain of csrc/ndp_autoencoder.inc, no BatchNorm launch (`ndivplanning_amd.autoencoder_eval` adds the byte output and the
reconstruction error).  A forward in training mode, with gradients, on the CPU or on another shape or dtype keeps
PyTorch's operators (`_forward_torch`), so that the classes still behave like nn.Modules there."""
from functools import partial
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import flat_params


def normal_init(m, mean, std):
    if isinstance(m, (nn.ConvTranspose2d, nn.Conv2d)):
        m.weight.data.normal_(mean, std)
        m.bias.data.zero_()


class Encoder(nn.Module):
    _CHANNELS = (3, 64, 128, 256, 512, 1024)

    def __init__(self, d=16):
        super().__init__()
        ch = self._CHANNELS
        for i in range(5):
            setattr(self, "conv%d" % (i + 1), nn.Conv2d(ch[i], ch[i + 1], 3, 2, 1))
            setattr(self, "conv%d_bn" % (i + 1), nn.BatchNorm2d(ch[i + 1]))
        self.conv6 = nn.Conv2d(ch[5], 128, 4, 1, 0)

    def weight_init(self, mean, std):
        for name in self._modules:
            normal_init(self._modules[name], mean, std)

    def forward(self, x):
        # Every caller in the reference detaches the codes at once (train_gan.py:152-153, control_evaluation.py:110-111,
        # mpc_eval.py:139-140) with grad mode on and the loaded parameters still requiring grad: an eval-mode forward
        # is therefore NOT differentiable with respect to the encoder's parameters here; only an input that itself
        # requires grad (or training mode) selects the PyTorch operators.
        if x.dtype == torch.uint8:
            # decoded camera frames [n,128,128,3] (bytes, HWC): the first convolution normalises them as it gathers
            # (utils/hdf5_load.py:9-11's formula) -- eval mode only, the GAN path's case
            if self.training:
                raise RuntimeError("byte frames are accepted by the eval-mode Encoder only (normalise them for training: "
                                   "(x / 255 - 0.5) * 2, NCHW)")
            if not x.is_cuda:
                from .. import _capi
                raise _capi.NdpError("frames are on %s: the eval-mode Encoder computes only on a ROCm GPU (no CPU fallback)"
                                     % x.device)
            return _encoder_forward_hip(self, x)
        if not self.training and not (torch.is_grad_enabled() and x.requires_grad):
            if not x.is_cuda:
                # the GAN path's case has no CPU or eager fallback, like Decoder / Discriminator
                from .. import _capi
                raise _capi.NdpError("images are on %s: the eval-mode Encoder computes only on a ROCm GPU "
                                     "(no CPU fallback)" % x.device)
            return _encoder_forward_hip(self, x)
        return self._forward_torch(x)

    def __getstate__(self):
        state = self.__dict__.copy()                 # whole-module pickles carry no kernel scratch
        state.pop("_ndp_packed", None)
        state.pop("_ndp_ws", None)
        return state

    def _forward_torch(self, x):
        for i in (1, 2, 3):
            x = F.relu(getattr(self, "conv%d_bn" % i)(getattr(self, "conv%d" % i)(x)))
        x = F.relu(self.conv4(x))
        x = F.relu(self.conv5(x))
        return self.conv6(x)


class Decoder(nn.Module):
    _CHANNELS = (1024, 512, 256, 128, 64)

    def __init__(self, d=128):
        super().__init__()
        ch = self._CHANNELS
        self.deconv1 = nn.ConvTranspose2d(128, ch[0], 4, 1, 0)
        self.deconv1_bn = nn.BatchNorm2d(ch[0])
        for i in range(1, 5):
            setattr(self, "deconv%d" % (i + 1), nn.ConvTranspose2d(ch[i - 1], ch[i], 4, 2, 1))
            setattr(self, "deconv%d_bn" % (i + 1), nn.BatchNorm2d(ch[i]))
        self.deconv6 = nn.ConvTranspose2d(ch[4], 3, 4, 2, 1)

    def weight_init(self, mean, std):
        for name in self._modules:
            normal_init(self._modules[name], mean, std)

    def forward(self, z):
        # the kernels only where PyTorch would record nothing: eval mode, CUDA float32 codes [n,128,1,1], and autograd
        # off or with nothing to differentiate; every other case is the PyTorch forward, unchanged
        if (not self.training and isinstance(z, torch.Tensor) and z.is_cuda and z.dtype == torch.float32 and z.dim() == 4
                and tuple(z.shape[1:]) == (128, 1, 1)
                and not (torch.is_grad_enabled() and (z.requires_grad or any(p.requires_grad for p in self.parameters())))):
            return decoder_forward_hip(self, z)[0]
        return self._forward_torch(z)

    def __getstate__(self):
        state = self.__dict__.copy()                 # whole-module pickles carry no kernel scratch
        state.pop("_ndp_packed", None)
        state.pop("_ndp_ws", None)
        return state

    def _forward_torch(self, z):
        for i in range(1, 6):
            z = F.relu(getattr(self, "deconv%d_bn" % i)(getattr(self, "deconv%d" % i)(z)))
        return torch.tanh(self.deconv6(z))


# ---------------------------------------------------------------- flat vectors of ndp_ae_* <-> modules
AE_LAYERS = (("encoder", "conv1"), ("encoder", "conv2"), ("encoder", "conv3"), ("encoder", "conv4"), ("encoder", "conv5"),
             ("encoder", "conv6"), ("decoder", "deconv1"), ("decoder", "deconv2"), ("decoder", "deconv3"),
             ("decoder", "deconv4"), ("decoder", "deconv5"), ("decoder", "deconv6"))
AE_BNS = (("encoder", "conv1_bn"), ("encoder", "conv2_bn"), ("encoder", "conv3_bn"), ("decoder", "deconv1_bn"),
          ("decoder", "deconv2_bn"), ("decoder", "deconv3_bn"), ("decoder", "deconv4_bn"), ("decoder", "deconv5_bn"))


_FLAT = flat_params.FlatParams("ndp_ae_layout", "ndp_ae_param_floats", "ndp_ae_stat_floats",
                               [".".join(x) for x in AE_LAYERS], [".".join(x) for x in AE_BNS])


def _resolve(encoder, decoder):
    return partial(flat_params.module_at, SimpleNamespace(encoder=encoder, decoder=decoder))


def ae_layout(lib, what, index):
    return _FLAT.layout(what, index)


def pack_autoencoder(encoder, decoder, device=None):
    """(params, running_stats): the flat vectors ndp_ae_train_grads reads, from an Encoder and a Decoder (layout:
    include/ndp.h, image autoencoder).  conv4_bn / conv5_bn are not part of them."""
    return _FLAT.pack(_resolve(encoder, decoder), device if device is not None else next(encoder.parameters()).device)


def unpack_autoencoder_vector(vec, encoder=None, decoder=None):
    """'encoder.conv1.weight' ... -> tensor in the modules' own shapes, from a flat vector in the parameters' layout
    (parameters, gradients or Adam moments)."""
    return _FLAT.unpack_vector(vec, _resolve(encoder if encoder is not None else Encoder(),
                                             decoder if decoder is not None else Decoder()))


def unpack_into_autoencoder(encoder, decoder, params, stats=None, batches_tracked=None):
    """Write the flat vectors back into the modules (after HIP training).  conv4_bn / conv5_bn -- no gradient, as torch's
    Adam leaves a parameter whose .grad is None -- keep their parameters, running statistics and counters."""
    _FLAT.unpack_into(_resolve(encoder, decoder), params, stats, batches_tracked)


def pack_encoder_params(enc):
    """The flat parameter buffer `ndp_encoder_forward` reads (layout: include/ndp.h): eval-mode BatchNorm of
    conv1..conv3 folded into weights and biases, conv1 as [27][64], conv2..6 as [Cout][KH][KW][Cin]."""
    parts = []
    with torch.no_grad():
        for i in range(1, 7):
            conv = getattr(enc, "conv%d" % i)
            w, b = conv.weight.detach().float(), conv.bias.detach().float()
            if i <= 3:
                bn = getattr(enc, "conv%d_bn" % i)
                scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
                w = w * scale.view(-1, 1, 1, 1)
                b = (b - bn.running_mean.detach().float()) * scale + bn.bias.detach().float()
            if i == 1:
                w = w.permute(1, 2, 3, 0).reshape(27, 64)            # [ci][kh][kw][co]
            else:
                w = w.permute(0, 2, 3, 1)                            # [co][kh][kw][ci]
            parts += [w.reshape(-1), b.reshape(-1)]
        return torch.cat(parts).contiguous()


def _encoder_state_key(enc):
    ts = list(enc.parameters()) + list(enc.buffers())
    return tuple((t.data_ptr(), t._version) for t in ts)


def _encoder_forward_hip(enc, x):
    from .. import _capi
    lib = _capi.load()
    u8 = x.dtype == torch.uint8
    if u8:
        if x.dim() != 4 or tuple(x.shape[1:]) != (128, 128, 3):
            raise _capi.NdpError("Encoder expects byte frames [n,128,128,3], got %s" % (tuple(x.shape),))
    else:
        _capi.require_gpu_f32(x, "images")
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, 128, 128):
            raise _capi.NdpError("Encoder expects images [n,3,128,128], got %s" % (tuple(x.shape),))
    key = _encoder_state_key(enc)
    cache = enc.__dict__.get("_ndp_packed")
    if cache is None or cache[0] != key or cache[1].device != x.device:
        packed = pack_encoder_params(enc).to(x.device)
        if packed.numel() != lib.ndp_encoder_param_floats():
            raise _capi.NdpError("encoder parameter count %d != %d" % (packed.numel(), lib.ndp_encoder_param_floats()))
        cache = (key, packed)
        enc.__dict__["_ndp_packed"] = cache
    x = x.contiguous()
    n = x.shape[0]
    codes = torch.empty(n, 128, device=x.device, dtype=torch.float32)
    if n == 0:
        return codes.view(0, 128, 1, 1)
    ws = enc.__dict__.get("_ndp_ws")
    need = lib.ndp_encoder_workspace_floats(n)
    if ws is None or ws.numel() < need or ws.device != x.device:
        ws = torch.empty(need, device=x.device, dtype=torch.float32)
        enc.__dict__["_ndp_ws"] = ws
    with torch.cuda.device(x.device):
        fn = lib.ndp_encoder_forward_u8 if u8 else lib.ndp_encoder_forward
        _capi.check(fn(_capi.ptr(cache[1]), _capi.ptr(x), n, _capi.ptr(codes), _capi.ptr(ws), _capi.stream_ptr()),
                    "ndp_encoder_forward_u8" if u8 else "ndp_encoder_forward")
    return codes.view(n, 128, 1, 1)


# ---------------------------------------------------------------- eval-mode Decoder on ndp_ae_decode
def fold_decoder_layers(dec, dtype=torch.float32):
    """[(w', b')] of deconv1..6 in the module's own shapes, eval-mode BatchNorm of deconv1..5 folded in, computed in
    `dtype` in this order: scale = gamma / sqrt(running_var + eps); w' = w * scale[cout]; b' = (b - running_mean) * scale
    + beta.  relu(bn(deconv(x))) == relu(conv_transpose2d(x, w', b')) in eval mode."""
    out = []
    with torch.no_grad():
        for i in range(1, 7):
            deconv = getattr(dec, "deconv%d" % i)
            w, b = deconv.weight.detach().to(dtype), deconv.bias.detach().to(dtype)
            if i <= 5:
                bn = getattr(dec, "deconv%d_bn" % i)
                scale = bn.weight.detach().to(dtype) / torch.sqrt(bn.running_var.detach().to(dtype) + bn.eps)
                w = w * scale.view(1, -1, 1, 1)                          # ConvTranspose2d: [cin][cout][kh][kw]
                b = (b - bn.running_mean.detach().to(dtype)) * scale + bn.bias.detach().to(dtype)
            out.append((w, b))
    return out


_DEC_FLAT = flat_params.FlatParams("ndp_ae_decoder_layout", "ndp_ae_decoder_param_floats", None,
                                   ["deconv%d" % i for i in range(1, 7)], [])


def fold_decoder_params(dec):
    """The flat parameter vector `ndp_ae_decode` reads (layout: include/ndp.h, eval-mode Decoder), on the module's
    device: `fold_decoder_layers` in fp32, per layer the weight as [cin_pad][kh][kw][cout_pad], then the bias."""
    from .. import _capi
    lib = _capi.load()
    device = dec.deconv1.weight.device
    params = torch.zeros(lib.ndp_ae_decoder_param_floats(), dtype=torch.float32, device=device)
    for i, (w, b) in enumerate(fold_decoder_layers(dec, torch.float32)):
        off, d = _DEC_FLAT.layout(0, i)
        params[off:off + d[0] * d[1] * d[2]] = flat_params.to_kernel_layout(w, d[0], d[2]).reshape(-1)
        boff, _ = _DEC_FLAT.layout(1, i)
        params[boff:boff + b.numel()] = b
    return params


def _decoder_state_key(dec):
    ts = list(dec.parameters()) + list(dec.buffers())
    return tuple((t.data_ptr(), t._version) for t in ts)


def _decoder_packed(dec, device, n):
    """(folded parameters, workspace with their second weight order in its head) for n images on `device`, cached on the
    module by the versions of its parameters and buffers and by the device."""
    from .. import _capi
    lib = _capi.load()
    key = _decoder_state_key(dec)
    cache = dec.__dict__.get("_ndp_packed")
    fresh = cache is None or cache[0] != key or cache[1].device != device
    if fresh:
        cache = (key, fold_decoder_params(dec).to(device))
        dec.__dict__["_ndp_packed"] = cache
    ws = dec.__dict__.get("_ndp_ws")
    need = lib.ndp_ae_decode_workspace_floats(n)
    if ws is None or ws.numel() < need or ws.device != device:
        ws = torch.empty(need, device=device, dtype=torch.float32)
        dec.__dict__["_ndp_ws"] = ws
        fresh = True
    if fresh:
        with torch.cuda.device(device):
            _capi.check(lib.ndp_ae_decode_pack(_capi.ptr(cache[1]), _capi.ptr(ws), _capi.stream_ptr()), "ndp_ae_decode_pack")
    return cache[1], ws


def decoder_forward_hip(dec, codes, out="float", target=None, errors=False):
    """ndp_ae_decode on codes [n,128,1,1] / [n,128] (CUDA float32): (reconstruction, per-image MSE, mean MSE).
    out: "float" -> [n,3,128,128] float32, "bytes" -> [n,128,128,3] uint8, None -> no reconstruction; target (float NCHW
    or byte frames HWC) with errors=True -> the MSE of every image against it [n] and their mean [1], else None."""
    from .. import _capi
    lib = _capi.load()
    if out not in ("float", "bytes", None):
        raise ValueError("out must be 'float', 'bytes' or None, got %r" % (out,))
    _capi.require_gpu_f32(codes, "codes")
    if codes.dim() not in (2, 4) or codes.shape[1] != 128 or codes.numel() != codes.shape[0] * 128:
        raise _capi.NdpError("Decoder expects codes [n,128,1,1], got %s" % (tuple(codes.shape),))
    if dec.training:
        raise _capi.NdpError("ndp_ae_decode is the eval-mode Decoder: call decoder.eval() first")
    n = int(codes.shape[0])
    dev = codes.device
    codes = codes.detach().contiguous()
    recon = None
    if out == "float":
        recon = torch.empty(n, 3, 128, 128, device=dev, dtype=torch.float32)
    elif out == "bytes":
        recon = torch.empty(n, 128, 128, 3, device=dev, dtype=torch.uint8)
    sq = mean = tf = tu = None
    if errors:
        if target is None:
            raise _capi.NdpError("errors=True needs a target")
        if not isinstance(target, torch.Tensor) or not target.is_cuda or target.device != dev:
            raise _capi.NdpError("the target must be on %s (no CPU fallback)" % dev)
        if target.dtype == torch.uint8 and tuple(target.shape) == (n, 128, 128, 3):
            tu = target.contiguous()
        elif target.dtype == torch.float32 and tuple(target.shape) == (n, 3, 128, 128):
            tf = target.detach().contiguous()
        else:
            raise _capi.NdpError("the target must be float32 [%d,3,128,128] or uint8 [%d,128,128,3], got %s %s"
                                 % (n, n, target.dtype, tuple(target.shape)))
        sq = torch.empty(n, device=dev, dtype=torch.float32)
        mean = torch.empty(1, device=dev, dtype=torch.float32)
    if n == 0:
        if mean is not None:
            mean.fill_(float("nan"))
        return recon, sq, mean
    if recon is None and not errors:
        raise _capi.NdpError("nothing to compute: no reconstruction and no errors requested")
    params, ws = _decoder_packed(dec, dev, n)
    p = _capi.ptr
    with torch.cuda.device(dev):
        _capi.check(lib.ndp_ae_decode(p(params), p(codes), n, p(recon) if out == "float" else None,
                                      p(recon) if out == "bytes" else None, p(tf), p(tu), p(sq), p(mean), p(ws),
                                      _capi.stream_ptr()), "ndp_ae_decode")
    return recon, sq, mean
