"""What the multi-step rollout tests share: the definition restated on the oracle's forward pass,
the gradient recursion the device implements, the plain numpy restatement of the link kernels' arithmetic and
schedule, and the run of the sanitized CPU driver (tests/host_drivers/fm_rollout.inc, through tests/host_driver.py).  No
GPU is touched here."""
import struct
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import host_driver
from oracle import forward_model_oracle as FO

PLANE, VALUES, THREADS = 128 * 128, 3 * 128 * 128, 256
F32 = np.float32

# Biases of the layers a BatchNorm follows (tests/test_gpu_forward_model.py): the batch mean is subtracted right after
# them, so their gradient is zero but for rounding and is compared with the weight gradient's scale, not with itself.
NOISE_BIASES = tuple("%s.bias" % n for n in ("encoder.conv1", "encoder.conv2", "encoder.conv3", "decoder.deconv1",
                                             "decoder.deconv2", "decoder.deconv3", "decoder.deconv4", "decoder.deconv5",
                                             "decoder.deconv6", "decoder.conv_refine_1"))


# ------------------------------------------------------------------------------------------ the stated definition
def rollout(state, frames, actions, relu_masks=None):
    """s_0 = x_0; r_k = model(s_k, a_k) in training mode (batch statistics of this call, running statistics moved by it);
    s_{k+1} = s_k + r_k, not detached; loss_k = mean((s_{k+1} - x_{k+1})^2), written as the reference's
    mse(r_k, x_{k+1} - s_k) -- the same difference, and for H = 1 the oracle trainer's expression to the bit;
    L = (loss_0 + .. + loss_{H-1}) / H.  frames [n,H+1,3,128,128], actions [n,H,4]; relu_masks: per pass, or None.
    Returns (L, [loss_k], [s_0 .. s_H])."""
    H = actions.shape[1]
    assert frames.shape[1] == H + 1
    s, losses, states = frames[:, 0], [], [frames[:, 0]]
    for k in range(H):
        r = FO.forward(state, s, actions[:, k], training=True, relu_masks=None if relu_masks is None else relu_masks[k])
        losses.append(F.mse_loss(r, frames[:, k + 1] - s))
        s = s + r
        states.append(s)
    return sum(losses) / H, losses, states


def rollout_grads(state, frames, actions, relu_masks=None):
    """End-to-end autograd of the definition: {loss, losses, grads (name -> tensor or None)}."""
    names = FO.trainable(state)
    for n in names:
        state[n].requires_grad_(True)
    L, losses, _ = rollout(state, frames, actions, relu_masks)
    g = torch.autograd.grad(L, [state[n] for n in names], allow_unused=True)
    return {"loss": L.detach(), "losses": [l.detach() for l in losses], "grads": OrderedDict(zip(names, g))}


def recursion_grads(state, frames, actions):
    """The recursion the device runs, with one torch.autograd.grad call per pass:
        local_j = (2 / (H N)) (s_j - x_j);  G_H = local_H;  for k = H-1 .. 0: backward of pass k with d_resid = G_{k+1}
        -> grad_k, dcur_k;  G_k = (local_k + G_{k+1}) + dcur_k;  grad = ((grad_0 + grad_1) + ..) + grad_{H-1}."""
    names = FO.trainable(state)
    for n in names:
        state[n].requires_grad_(True)
    H = actions.shape[1]
    N = frames[:, 0].numel()
    s, ins, resids, local = frames[:, 0], [], [], [None]
    for k in range(H):
        s_in = s.detach().clone().requires_grad_(True)
        r = FO.forward(state, s_in, actions[:, k], training=True)
        s = s_in.detach() + r.detach()
        ins.append(s_in)
        resids.append(r)
        local.append((2.0 / (H * N)) * (s - frames[:, k + 1]))
    G, per_pass = local[H], [None] * H
    for k in range(H - 1, -1, -1):
        out = torch.autograd.grad(resids[k], [state[n] for n in names] + [ins[k]], grad_outputs=G, allow_unused=True)
        per_pass[k] = out[:-1]
        if k >= 1:
            G = (local[k] + G) + out[-1]
    grads = OrderedDict()
    for i, n in enumerate(names):
        if per_pass[0][i] is None:
            grads[n] = None
            continue
        total = per_pass[0][i]
        for k in range(1, H):
            total = total + per_pass[k][i]
        grads[n] = total
    return grads


# ------------------------------------------------------------------------------------------ the kernels' arithmetic, in numpy
def norm_table():
    """utils/hdf5_load.py:9-11 in fp32: what u8_norm_table holds."""
    return ((np.arange(256).astype(F32) / F32(255.0)) - F32(0.5)) * F32(2.0)


def as_float_frames(frames):
    """uint8 [n,128,128,3] -> the floats the loader would upload, [n,3,128,128]; floats pass through."""
    if frames.dtype != np.uint8:
        return frames
    return np.ascontiguousarray(norm_table()[frames].transpose(0, 3, 1, 2))


def loss_scale(n, steps):
    return F32(2.0 / (float(steps) * float(n * VALUES)))


def want_advance(state, resid, target, step, steps, loss, loss_sum):
    """(state_next, local_next, the blocks' sums, loss_step, loss, loss_sum) by the kernels' fixed order."""
    n = state.shape[0]
    x = as_float_frames(target)
    sn = (state + resid).astype(F32)
    d = (sn - x).astype(F32)
    local = (loss_scale(n, steps) * d).astype(F32)
    # a thread: image, four neighbouring pixels; its twelve squares in the order channel, pixel
    sq = (d.astype(np.float64) ** 2).reshape(n, 3, PLANE // 4, 4).transpose(0, 2, 1, 3).reshape(n * PLANE // 4, 12)
    thread = np.zeros(sq.shape[0])
    for i in range(12):
        thread = thread + sq[:, i]
    red = thread.reshape(-1, THREADS).copy()                         # a block: the fixed tree 128, 64 .. 1
    w = THREADS // 2
    while w > 0:
        red[:, :w] = red[:, :w] + red[:, w:2 * w]
        w //= 2
    partial = red[:, 0].copy()
    share = np.zeros(THREADS)                                        # the final pass: thread t adds blocks t, t + 256 ..
    for i in range(len(partial)):
        share[i % THREADS] = share[i % THREADS] + partial[i]
    total = 0.0
    for t in range(THREADS):
        total = total + share[t]
    lk = total / float(n * VALUES)
    new_loss = F32((F32(0.0) if step == 0 else F32(loss)) + F32(lk / float(steps)))
    new_sum = F32(F32(loss_sum) + new_loss) if step == steps - 1 else F32(loss_sum)
    return sn, local, partial, F32(lk), new_loss, new_sum


# ------------------------------------------------------------------------------------------ the CPU driver
def build_driver(out_dir=None, sanitize=True):
    return host_driver.build(sanitize)


def _strided(images, stride):
    """images [n, ...] -> one flat buffer with image i at i * stride elements (the gaps hold a pattern nobody may read)."""
    n = images.shape[0]
    per = images[0].size
    fill = 0xA5 if images.dtype == np.uint8 else np.nan
    buf = np.full((n - 1) * stride + per, fill, images.dtype)
    for i in range(n):
        buf[i * stride:i * stride + per] = images[i].reshape(-1)
    return buf


def run_driver(exe, cases, work_dir, timeout=900):
    """cases: dicts with kind 'begin' (frames, stride), 'advance' (state, resid, target, stride, step, steps, loss, loss_sum),
    'chain' (local, g_next, d_cur) or 'sum' (grads [count, floats], stride).  Asserts that the child exits 0 with no
    sanitizer report.  Returns per case the outputs the driver's header lists."""
    kinds = {"begin": 0, "advance": 1, "chain": 2, "sum": 3}
    parts = [struct.pack("<i", len(cases))]
    for c in cases:
        k = kinds[c["kind"]]
        if k in (0, 1):
            tgt = c["frames"] if k == 0 else c["target"]
            n = tgt.shape[0]
            parts.append(struct.pack("<8i", k, n, c.get("steps", 1), c.get("step", 0), int(tgt.dtype == np.uint8), c["stride"], 0, 0))
            if k == 1:
                parts += [np.ascontiguousarray(c["state"], F32).tobytes(), np.ascontiguousarray(c["resid"], F32).tobytes()]
            parts.append(_strided(tgt, c["stride"]).tobytes())
            if k == 1:
                parts.append(np.array([c["loss"], c["loss_sum"]], F32).tobytes())
        elif k == 2:
            parts.append(struct.pack("<8i", k, c["local"].shape[0], 0, 0, 0, 0, 0, 0))
            parts += [np.ascontiguousarray(c[name], F32).tobytes() for name in ("local", "g_next", "d_cur")]
        else:
            count, floats = c["grads"].shape
            parts += [struct.pack("<8i", k, 1, 0, 0, 0, c["stride"], count, floats),
                      _strided(np.ascontiguousarray(c["grads"], F32), c["stride"]).tobytes()]
    raw = np.frombuffer(host_driver.run("fm_rollout", b"".join(parts), work_dir, timeout=timeout, exe=exe), np.uint8)
    out, pos = [], 0

    def take(count, dtype):
        nonlocal pos
        size = count * np.dtype(dtype).itemsize
        a = raw[pos:pos + size].copy().view(dtype)
        pos += size
        return a
    for c in cases:
        k = kinds[c["kind"]]
        if k == 0:
            n = c["frames"].shape[0]
            out.append(take(n * VALUES, F32).reshape(n, 3, 128, 128))
        elif k == 1:
            n = c["state"].shape[0]
            out.append((take(n * VALUES, F32).reshape(n, 3, 128, 128), take(n * VALUES, F32).reshape(n, 3, 128, 128),
                        take(n * 16, np.float64), take(c["steps"], F32), take(1, F32)[0], take(1, F32)[0]))
        elif k == 2:
            out.append(take(c["local"].size, F32).reshape(c["local"].shape))
        else:
            out.append(take(c["grads"].shape[1], F32))
    assert pos == raw.size, (pos, raw.size)
    return out
