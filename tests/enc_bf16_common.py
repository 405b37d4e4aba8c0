"""Shared by tests/test_enc_bf16.py (CPU) and tests/test_gpu_enc_bf16.py (GPU): what precision NDP_ENC_BF16 of the image
encoder's pass (include/ndp.h) means, restated apart from the kernels, on the PACKED parameter buffer (whose layout
tests/test_encoder_oracle.py pins to the oracle):

  conv1        F.conv2d of the image with the packed fp32 weight in the given dtype, + bias, ReLU;
  conv2..6     the input and the packed weight rounded through fm_bf16_common.round_tensor (fp32 -> bf16, to nearest even),
               convolved in the given dtype, + the fp32 bias, ReLU (not behind conv6).

The input of layer l + 1 is the ROUNDED output of layer l: that is the stored bf16 map.  With fp64 tensors the products are
exact and the sum (almost) is: the definition.  rounded=False switches every rounding off: the plain network.
"""
import numpy as np
import torch
import torch.nn.functional as F

from fm_bf16_common import rel_norm, round_tensor  # noqa: F401  (rel_norm: for the tests)
from oracle import encoder_oracle as EO

# (Cin, Cout, kernel, stride, padding), conv1..conv6
LAYERS = ((3, 64, 3, 2, 1), (64, 128, 3, 2, 1), (128, 256, 3, 2, 1), (256, 512, 3, 2, 1), (512, 1024, 3, 2, 1), (1024, 128, 4, 1, 0))
SIDES = (64, 32, 16, 8, 4)                        # of the maps behind conv1..conv5
LP_WEIGHT_VALUES = sum(co * k * k * ci for ci, co, k, _, _ in LAYERS[1:])
assert LP_WEIGHT_VALUES == 8364032


def packed_layer(packed, l):
    """(weight [Cout,Cin,k,k], bias [Cout]) of conv l + 1 from the packed buffer, fp32 views made contiguous."""
    o = 0
    for i, (cin, cout, k, _, _) in enumerate(LAYERS):
        nw = cout * k * k * cin
        if i == l:
            w, b = packed[o:o + nw], packed[o + nw:o + nw + cout]
            w = w.reshape(cin, k, k, cout).permute(3, 0, 1, 2) if i == 0 else w.reshape(cout, k, k, cin).permute(0, 3, 1, 2)
            return w.contiguous(), b.contiguous()
        o += nw + cout
    raise IndexError(l)


def layer_forward(packed, l, x, dtype, rounded=True):
    """Layer l (0..5) alone on the input x [n,Cin,H,W] (for l >= 1: the stored map, NCHW): act(bias + conv(x, w)) in `dtype`;
    rounded: both operands of l >= 1 go through round_tensor first."""
    w, b = packed_layer(packed, l)
    _, _, _, stride, pad = LAYERS[l]
    x, w = x.to(dtype), w.to(dtype)
    if rounded and l >= 1:
        x, w = round_tensor(x), round_tensor(w)
    with torch.no_grad():
        y = F.conv2d(x, w, b.to(dtype), stride=stride, padding=pad)
        return F.relu(y) if l < 5 else y


def fp32_sum_error_bound(packed, l, x):
    """Per output element of layer l on the input x, the most by which ANY fp32 evaluation of the definition's sum can
    lie from the exact value (fp64 tensor, shaped like the layer's output): the sum has K products and the bias, so by
    the standard bound of floating-point summation in any order, |fl(sum) - sum| <= (K + 2) u (sum |x_i w_i| + |bias|) with
    u = 2^-24 (K + 1 terms; one more rounding per product for conv1, whose fp32 operands do not multiply exactly).  The
    operands are the ones the layer multiplies: rounded for l >= 1."""
    w, b = packed_layer(packed, l)
    cin, _, k, stride, pad = LAYERS[l]
    x, w = x.double(), w.double()
    if l >= 1:
        x, w = round_tensor(x), round_tensor(w)
    with torch.no_grad():
        s = F.conv2d(x.abs(), w.abs(), b.double().abs(), stride=stride, padding=pad)
    return (cin * k * k + 2) * 2.0 ** -24 * s


def restatement(packed, images, dtype=torch.float64, rounded=True):
    """The whole pass: (the five maps behind conv1..conv5 as STORED -- rounded when `rounded` -- NCHW, in `dtype`; the codes
    [n,128] in `dtype`)."""
    maps, x = [], images
    for l in range(5):
        x = layer_forward(packed, l, x, dtype, rounded)
        if rounded:
            x = round_tensor(x)
        maps.append(x)
    return maps, layer_forward(packed, 5, x, dtype, rounded).reshape(-1, 128)


def pack_state(state, dtype):
    """pack_encoder_params' buffer from an oracle state with the BatchNorm folding done in `dtype` (fp64: a packed buffer
    without the fp32 roundings of the folded weights, for the comparison with the fp64 oracle; fp32: pack_encoder_params)."""
    parts = []
    for i in range(1, 7):
        w, b = state["conv%d.weight" % i].to(dtype), state["conv%d.bias" % i].to(dtype)
        if i <= 3:
            bn = "conv%d_bn." % i
            scale = state[bn + "weight"].to(dtype) / torch.sqrt(state[bn + "running_var"].to(dtype) + 1e-5)
            w = w * scale.view(-1, 1, 1, 1)
            b = (b - state[bn + "running_mean"].to(dtype)) * scale + state[bn + "bias"].to(dtype)
        w = w.permute(1, 2, 3, 0).reshape(27, 64) if i == 1 else w.permute(0, 2, 3, 1)
        parts += [w.reshape(-1), b.reshape(-1)]
    return torch.cat(parts).contiguous()


# ------------------------------------------------------------------------------------------------ the model, the images
def model_case(n):
    """(oracle state, packed fp32 parameters on the CPU, images float32 [n,3,128,128]): EO.init_encoder_state(11, bn_seed=12)
    and EO.synthetic_images(13, n)."""
    from ndivplanning_amd.models.image_autoencoder import Encoder, pack_encoder_params
    state = EO.init_encoder_state(11, bn_seed=12)
    enc = Encoder()
    enc.load_state_dict(state, strict=False)
    enc.eval()
    return state, pack_encoder_params(enc).detach().cpu().contiguous(), EO.synthetic_images(13, n)


def byte_frames():
    """(bytes [2,128,128,3], the float tensor [2,3,128,128] the reference's loader builds from them): tests/golden/frames_case.npz."""
    from conftest import load_golden
    g = load_golden("frames_case")
    frames = torch.from_numpy(np.ascontiguousarray(g["frames_u8"]))
    return frames, torch.from_numpy(g["lut"][g["frames_u8"]].transpose(0, 3, 1, 2).copy())


def bf16_ulp(ref):
    """One bf16 ulp at |ref| (fp64 tensor): 2^(floor(log2 |ref|) - 7), the smallest normal's for anything below it."""
    a = ref.abs().double().clamp_min(2.0 ** -126)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), torch.floor(torch.log2(a)) - 7)
