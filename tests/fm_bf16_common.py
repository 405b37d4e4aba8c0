"""Shared by tests/test_fm_bf16.py (CPU) and tests/test_gpu_fm_bf16.py (GPU): what precision NDP_FM_BF16 of the eval-mode
forward model (include/ndp.h) means, restated apart from the kernels.

  to_bf16 / to_bf16_bits   fp32 -> bf16, round to nearest even, by integer arithmetic on the bits (numpy);
  rounded_layers()         a context manager under which oracle.forward_model_oracle.forward (imported, not edited) rounds
                           the input and the weight of exactly the nine stride-2 layers -- conv2..conv5, deconv2..deconv6 --
                           and of no other: it wraps torch.nn.functional.conv2d / conv_transpose2d and tells the layers apart
                           by call order (one forward = 8 conv2d calls: conv1..6, refine 1, 2; 6 conv_transpose2d calls:
                           deconv1..6).  Everything else of the oracle -- bias, BatchNorm, ReLU, the concatenations, tanh --
                           runs in the dtype it is given: with fp64 tensors the restatement is the definition with exact
                           products and an (almost) exact sum;
  golden_case(n)           the seeded model of tests/golden/fm_eval_case.npz with n images and actions.
"""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

import fm_eval_common as C

# the layers precision bf16 touches, by call index within one forward of the oracle
ROUNDED_CONV2D = (1, 2, 3, 4)                  # of conv1..conv6, conv_refine_1, conv_refine_2
ROUNDED_CONV_TRANSPOSE2D = (1, 2, 3, 4, 5)     # of deconv1..deconv6
CALLS_PER_FORWARD = {"conv2d": 8, "conv_transpose2d": 6}
LAYER_NAMES = {("conv2d", i): "conv%d" % (i + 1) for i in range(6)}
LAYER_NAMES.update({("conv2d", 6): "refine1", ("conv2d", 7): "refine2"})
LAYER_NAMES.update({("conv_transpose2d", i): "deconv%d" % (i + 1) for i in range(6)})
NINE = ("conv2", "conv3", "conv4", "conv5", "deconv2", "deconv3", "deconv4", "deconv5", "deconv6")


def to_bf16_bits(x):
    """uint16 bits of bf16(x), x float32: round to nearest, ties to even, on the integer bits; +-Inf stay, a finite value
    beyond the largest bf16 rounds to +-Inf, a NaN stays a NaN: its upper 16 bits with the quiet bit set (which NaN a
    conversion writes is its own affair -- torch's CPU paths write 0x7FC0 or 0xFFFF -- only that it is one is defined)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    rounded = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    nan = (u & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    return np.where(nan, (u >> np.uint64(16)) | np.uint64(0x0040), rounded).astype(np.uint16)


def to_bf16(x):
    """float32 array of the values bf16(x)."""
    return (to_bf16_bits(x).astype(np.uint32) << np.uint32(16)).view(np.float32).reshape(np.shape(x))


def round_tensor(t):
    """bf16(t) in t's dtype (fp32 or fp64; an fp64 value goes through fp32 first, as a stored map is fp32).  torch's own
    conversion, which tests/test_fm_bf16.py holds to to_bf16 bit for bit."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


@contextlib.contextmanager
def rounded_layers(log=None):
    """See the module docstring.  log: a list that receives (function name, call index in its forward, layer name, rounded)
    per call."""
    real = {"conv2d": F.conv2d, "conv_transpose2d": F.conv_transpose2d}
    counts = {"conv2d": 0, "conv_transpose2d": 0}
    which = {"conv2d": ROUNDED_CONV2D, "conv_transpose2d": ROUNDED_CONV_TRANSPOSE2D}

    def wrap(name):
        def call(x, w, *args, **kw):
            idx = counts[name] % CALLS_PER_FORWARD[name]
            counts[name] += 1
            rounded = idx in which[name]
            if log is not None:
                log.append((name, idx, LAYER_NAMES[(name, idx)], rounded))
            if rounded:
                x, w = round_tensor(x), round_tensor(w)
            return real[name](x, w, *args, **kw)
        return call

    F.conv2d, F.conv_transpose2d = wrap("conv2d"), wrap("conv_transpose2d")
    try:
        yield
    finally:
        F.conv2d, F.conv_transpose2d = real["conv2d"], real["conv_transpose2d"]


# ------------------------------------------------------------------------------------------------ the golden model
def golden_case(n):
    """(cpu module in eval mode, byte frames uint8 [n,128,128,3], the same frames as float32 [n,3,128,128], actions
    float32 [n,4]) from the recipe of tests/golden/fm_eval_case.npz: its 8 frames and their actions; images beyond the 8th
    are earlier ones mirrored left to right with the negated action."""
    from ndivplanning_amd.models.forward_encoder import ForwardAutoencoder
    R = C.recipe()
    model = R.build_module(ForwardAutoencoder)
    frames_u8, actions = R.inputs()
    frames_u8, actions = frames_u8.reshape(-1, 128, 128, 3), actions.reshape(-1, 4)
    rows = [i % len(frames_u8) for i in range(n)]
    f = torch.stack([frames_u8[r] if i < len(frames_u8) else frames_u8[r].flip(1) for i, r in enumerate(rows)])
    a = torch.stack([actions[r] if i < len(actions) else -actions[r] for i, r in enumerate(rows)])
    return model, f.contiguous(), R.norm_frames(f), a.contiguous()


def oracle_state(model, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in model.state_dict().items()}


def oracle_forward(model, images, actions, dtype=torch.float64, rounded=False, log=None):
    """The oracle's eval-mode prediction [n,3,128,128] in `dtype`; rounded: under rounded_layers()."""
    from oracle import forward_model_oracle as FO
    s = oracle_state(model, dtype)
    with torch.no_grad():
        if not rounded:
            return FO.forward(s, images.to(dtype), actions.to(dtype), training=False)
        with rounded_layers(log):
            return FO.forward(s, images.to(dtype), actions.to(dtype), training=False)


def rel_norm(a, b):
    """||a - b|| / ||b|| in fp64."""
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())
