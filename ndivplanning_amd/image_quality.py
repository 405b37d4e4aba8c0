"""SSIM and PSNR of image pairs on the device, for the evaluations of the networks that draw pictures (the forward model
and the image autoencoder): the mean squared error they report rewards blur, these two do not.

    image_quality(a, b, a_idx=None, b_idx=None, ssim=True, psnr=True)      ->  (ssim [n] or None, psnr [n] or None)

One call of `ndp_image_quality` (csrc/ndp_eval.inc): a workgroup per (pair, channel, band of output rows)
filters the five moment maps through LDS and leaves one fp64 sum per row, a second small kernel folds them.  Images are
3 x 128 x 128: float32 NCHW in the networks' [-1, 1] scale or byte frames HWC (normalised through the loader's table: the
bits of the floats of the same bytes).  Values are brought to [0, 1] and clamped there; SSIM is scikit-image's
structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range=1) in fp32, PSNR is
10 log10(1 / mse).  An image against itself gives exactly 1 and +Inf; a NaN value, or an index outside its array, gives
NaN for both results of that pair.  There is no CPU path (`NdpError`), no host synchronisation, and two calls give the
same bits."""
import torch

from . import _capi
from ._eval_io import fp64_mean

IMAGE = (3, 128, 128)
FRAME = (128, 128, 3)


def _images(t, name):
    """`t` as the kernel takes it, flattened to [m, ...]: float32 NCHW or byte frames HWC (shapes first, devices after:
    a wrong shape is reported as such on any device)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.dtype == torch.uint8:
        if t.dim() < 3 or tuple(t.shape[-3:]) != FRAME:
            raise _capi.NdpError("%s: byte frames must be [...,128,128,3], got %s" % (name, tuple(t.shape)))
        t = t.detach().reshape(-1, *FRAME)
    elif not t.is_floating_point() or t.dim() < 3 or tuple(t.shape[-3:]) != IMAGE:
        raise _capi.NdpError("%s: float images must be [...,3,128,128], got %s %s" % (name, t.dtype, tuple(t.shape)))
    else:
        t = t.detach().reshape(-1, *IMAGE).float()
    return t


def _index(idx, device, name):
    if idx is None:
        return None
    if not isinstance(idx, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor or None" % name)
    return idx.to(device=device, dtype=torch.int32).reshape(-1).contiguous()


def image_quality(a, b, a_idx=None, b_idx=None, ssim=True, psnr=True):
    """(ssim [n] or None, psnr [n] or None), float32 device tensors: pair p compares a[a_idx[p]] with b[b_idx[p]] (an
    index map of None: row p).  a, b: float32 [m,3,128,128] in [-1, 1] or byte frames uint8 [m,128,128,3], on one GPU;
    a_idx, b_idx: integer tensors [n].  n is the index maps' length, without them the number of images (which the two
    operands must then share)."""
    if not (ssim or psnr):
        raise _capi.NdpError("image_quality: nothing to compute (ssim and psnr are both off)")
    a, b = _images(a, "a"), _images(b, "b")
    for name, t in (("a", a), ("b", b)):
        if not t.is_cuda:
            raise _capi.NdpError("%s is on %s: ndivplanning_amd computes only on a ROCm GPU (no CPU fallback)" % (name, t.device))
    dev = a.device
    if b.device != dev:
        raise _capi.NdpError("a is on %s, b on %s" % (dev, b.device))
    a, b = a.contiguous(), b.contiguous()
    a_idx, b_idx = _index(a_idx, dev, "a_idx"), _index(b_idx, dev, "b_idx")
    n_a, n_b = int(a.shape[0]), int(b.shape[0])
    counts = {int(i.numel()) for i in (a_idx, b_idx) if i is not None}
    if a_idx is None:
        counts.add(n_a)
    if b_idx is None:
        counts.add(n_b)
    if len(counts) != 1:
        raise _capi.NdpError("image_quality: the operands do not agree on the number of pairs (a %d images%s, b %d images%s)"
                             % (n_a, "" if a_idx is None else " through %d indices" % a_idx.numel(),
                                n_b, "" if b_idx is None else " through %d indices" % b_idx.numel()))
    n = counts.pop()
    if n < 1 or n_a < 1 or n_b < 1:
        raise _capi.NdpError("image_quality: no pairs (a %d images, b %d images, %d pairs)" % (n_a, n_b, n))
    lib = _capi.load()
    ws_bytes = int(lib.ndp_image_quality_ws_bytes(n))
    if ws_bytes <= 0:
        raise _capi.NdpError("image_quality: %d pairs are more than one call takes" % n)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    out_ssim = torch.empty(n, dtype=torch.float32, device=dev) if ssim else None
    out_psnr = torch.empty(n, dtype=torch.float32, device=dev) if psnr else None
    f32 = lambda t: t if t.dtype == torch.float32 else None     # noqa: E731
    u8 = lambda t: t if t.dtype == torch.uint8 else None        # noqa: E731
    p = _capi.ptr
    with _capi.on_device(a):
        _capi.check(lib.ndp_image_quality(p(f32(a)), p(u8(a)), n_a, p(a_idx), p(f32(b)), p(u8(b)), n_b, p(b_idx), n,
                                          p(out_ssim), p(out_psnr), p(ws), ws_bytes, _capi.stream_ptr(dev)),
                    "ndp_image_quality")
    return out_ssim, out_psnr


mean = fp64_mean          # [1] float32: the mean of the fp32 per-pair values, taken in fp64; no value is skipped
