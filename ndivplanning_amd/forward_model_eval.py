"""What a trained forward (next-frame) model is asked after training, on the gfx950 kernels: how large its prediction
error is on held-out trajectories when it is fed its own predictions for 1, 2, ... H steps -- what `mpc_plan`, `plan_step`
and `MpcController` rely on -- and whether it beats the trivial predictor "the frame does not change".

    predict(fwd_model, state, actions, target)        one step: next state, its MSE per image, the persistence MSE, the mean
    rollout(fwd_model, state0, actions, targets)      H steps on the model's own fp32 predictions: [B,H,...], err / persistence [B,H]
    rollout_schedule(T, horizon)                      which start frames are alive at step h, their action and target frame
    evaluate(fwd_model, dataset, horizon)             the same over a PushDataset / SyntheticPushDataset, from EVERY start frame
    python -m ndivplanning_amd.forward_model_eval --model forward_autoencoder_N.pt --data DIR [--horizon H] [--save-dir DIR]

The predictions come from the eval-mode `ForwardAutoencoder` (ndp_fm_forward / _u8 with training = 0: state + residual),
the scoring from `ndp_fm_score` (csrc/ndp_eval.inc: one launch gives every prediction's MSE against its target frame,
the MSE of the start frame against the same target and the reference's display bytes, `denorm(...).astype(np.uint8)` of
train_forward_model.py:116-145; targets and start frames are addressed through index maps, no gathered copy).  The
module is used in eval mode; there is no CPU path (`NdpError`), and nothing here synchronises with the host per batch:
every result is a device tensor.  quality=True (predict, rollout, evaluate; --quality) adds SSIM and PSNR of the
same pairs -- prediction against target, start frame against target -- from `ndp_image_quality` (image_quality.py): the MSE
rewards a blurred prediction, these do not.  Off by default, and nothing else changes with it."""
import os
from argparse import ArgumentParser

import numpy as np
import torch

from . import _capi
from . import image_quality as IQ
from . import jpeg as jpeg_frames
from ._eval_io import (FM_PRECISIONS, _check_out, _require_eval, _require_gpu, _to_bytes, fm_precision_code, fp64_mean,
                       load_module, trajectory_batches)
from .utils.trajectory_loader import open_dataset

IMAGE = (3, 128, 128)
FRAME = (128, 128, 3)


def _images(t, name):
    """`t` as the kernels take it, flattened to [m, ...]: float32 NCHW or byte frames HWC, contiguous."""
    _require_gpu(t, name)
    if t.dtype == torch.uint8:
        if tuple(t.shape[-3:]) != FRAME:
            raise _capi.NdpError("%s: byte frames must be [...,128,128,3], got %s" % (name, tuple(t.shape)))
        return t.detach().reshape(-1, *FRAME).contiguous()
    if tuple(t.shape[-3:]) != IMAGE:
        raise _capi.NdpError("%s: float images must be [...,3,128,128], got %s" % (name, tuple(t.shape)))
    return t.detach().reshape(-1, *IMAGE).contiguous().float()


def _index(idx, n, device, name):
    if idx is None:
        return None
    idx = idx.to(device=device, dtype=torch.int32).contiguous()
    if idx.numel() != n:
        raise _capi.NdpError("%s has %d entries for %d predictions" % (name, idx.numel(), n))
    return idx


def score(pred, target=None, target_idx=None, base=None, base_idx=None, errors=True, out_bytes=False):
    """ndp_fm_score on device tensors: pred float32 [n,3,128,128]; target / base float NCHW or byte frames HWC
    [m,...]; target_idx / base_idx int32 [n] or None (prediction i uses row i).  Returns (pred_err [n] or None, base_err
    [n] or None, bytes [n,128,128,3] or None).  An index outside its array gives NaN for that prediction's error."""
    lib = _capi.load()
    pred = _images(pred, "pred")
    if pred.dtype != torch.float32:
        raise _capi.NdpError("pred must be float32 [n,3,128,128]")
    n, dev = int(pred.shape[0]), pred.device
    if target is None:                                              # bytes alone: the entry wants a target, reads none
        target, errors, base = pred, False, None
    target = _images(target, "target")
    base = _images(base, "base") if base is not None else None
    for name, t in (("target", target), ("base", base)):
        if t is not None and t.device != dev:
            raise _capi.NdpError("pred is on %s, %s on %s" % (dev, name, t.device))
    target_idx, base_idx = _index(target_idx, n, dev, "target_idx"), _index(base_idx if base is not None else None, n, dev, "base_idx")
    pred_err = torch.empty(n, dtype=torch.float32, device=dev) if errors else None
    base_err = torch.empty(n, dtype=torch.float32, device=dev) if base is not None else None
    pred_u8 = torch.empty(n, *FRAME, dtype=torch.uint8, device=dev) if out_bytes else None
    f32 = lambda t: t if t is not None and t.dtype == torch.float32 else None     # noqa: E731
    u8 = lambda t: t if t is not None and t.dtype == torch.uint8 else None        # noqa: E731
    p = _capi.ptr
    with _capi.on_device(pred):
        _capi.check(lib.ndp_fm_score(p(pred), n, p(f32(target)), p(u8(target)), int(target.shape[0]), p(target_idx),
                                     p(f32(base)), p(u8(base)), int(base.shape[0]) if base is not None else 0, p(base_idx),
                                     p(pred_err), p(base_err), p(pred_u8), _capi.stream_ptr(dev)), "ndp_fm_score")
    return pred_err, base_err, pred_u8


def _forward_bf16(fwd_model, state, actions):
    """One eval-mode pass with bf16 operands (NDP_FM_BF16, include/ndp.h) on the module's packed parameters: a workspace
    and the bf16 weights of their own beside the module's cache, rebuilt when the cache is (a parameter changed)."""
    lib = _capi.load()
    dev, n = state.device, int(state.shape[0])
    cache = fwd_model._cache_for(dev)
    lp = cache.get("lp")
    if lp is None or lp["n"] < n:
        lp = cache["lp"] = {"ws": torch.empty(lib.ndp_fm_workspace_floats(n), dtype=torch.float32, device=dev), "n": n,
                            "weights": torch.empty(lib.ndp_fm_lp_weight_bytes(), dtype=torch.uint8, device=dev),
                            "packed": False}
    u8 = state.dtype == torch.uint8
    if u8 and tuple(state.shape[1:]) != (128, 128, 3):
        raise _capi.NdpError("byte frames must be [n,128,128,3], got %s" % (tuple(state.shape),))
    x = state.detach().contiguous() if u8 else state.detach().contiguous().float()
    a = actions.detach().contiguous().float()
    out = torch.empty(n, 3, 128, 128, dtype=torch.float32, device=dev)
    with _capi.on_device(x):
        st = _capi.stream_ptr(dev)
        if not lp["packed"]:
            _capi.check(lib.ndp_fm_pack_params(_capi.ptr(cache["params"]), _capi.ptr(lp["ws"]), st), "ndp_fm_pack_params")
            _capi.check(lib.ndp_fm_pack_params_lp(_capi.ptr(cache["params"]), _capi.ptr(lp["ws"]), _capi.ptr(lp["weights"]), st),
                        "ndp_fm_pack_params_lp")
            lp["packed"] = True
        _capi.check(lib.ndp_fm_forward_lp(_capi.ptr(cache["params"]), _capi.ptr(cache["stats"]), None if u8 else _capi.ptr(x),
                                          _capi.ptr(x) if u8 else None, _capi.ptr(a), n, 1, _capi.ptr(lp["weights"]),
                                          _capi.ptr(out), _capi.ptr(lp["ws"]), st), "ndp_fm_forward_lp")
    return out


def _forward(fwd_model, state, actions, precision="fp32"):
    if precision == "bf16":
        return _forward_bf16(fwd_model, state, actions)
    with torch.no_grad():
        return fwd_model(state, actions.detach().float())


def _quality(pred, base, target, base_idx=None, target_idx=None):
    """(ssim, psnr, persistence_ssim, persistence_psnr): two ndp_image_quality launches, the predictions against their
    targets, then the base frames against the same targets."""
    ssim, psnr = IQ.image_quality(pred, target, b_idx=target_idx)
    base_ssim, base_psnr = IQ.image_quality(base, target, a_idx=base_idx, b_idx=target_idx)
    return ssim, psnr, base_ssim, base_psnr


def predict(fwd_model, state, actions, target=None, out="float", quality=False, precision="fp32"):
    """(next_state, per-image MSE [n], persistence MSE [n], mean MSE [1]) of one eval-mode step from `state`, float32
    [n,3,128,128] in [-1,1] or byte frames uint8 [n,128,128,3] (normalised as the loader does, as the kernels read them).
    next_state: float32 NCHW (out="float") or the reference's bytes HWC (out="bytes": below 0 / above 255 saturate).  The
    errors are against `target` (float or byte frames); the persistence MSE is that of `state` itself against the target.
    Without a target the three error results are None.  quality=True: four more results follow, SSIM and PSNR per image of
    the prediction and of `state` itself against the target (ssim, psnr, persistence_ssim, persistence_psnr [n]; None
    without a target).  precision: 'fp32', or 'bf16' -- the pass with bf16 operands (NDP_FM_BF16, include/ndp.h)."""
    _check_out(out)
    fm_precision_code(precision)
    _require_eval(fwd_model=fwd_model)
    _require_gpu(state, "state")
    pred = _forward(fwd_model, state, actions, precision)
    if target is None:
        return ((score(pred, out_bytes=True)[2] if out == "bytes" else pred), None, None, None) + ((None,) * 4 if quality else ())
    err, base_err, pred_u8 = score(pred, target, base=state, out_bytes=out == "bytes")
    extra = _quality(pred, state, target) if quality else ()
    return ((pred_u8 if out == "bytes" else pred), err, base_err, fp64_mean(err)) + extra


def rollout(fwd_model, state0, actions, targets=None, out="float", quality=False, precision="fp32"):
    """H eval-mode steps from state0 [B,...] (float NCHW or byte frames) with actions [B,H,4], every step on the model's
    own fp32 prediction of the step before, as `mpc_plan` does (bytes are never fed back).  Returns (predictions
    [B,H,3,128,128] float32 or [B,H,128,128,3] bytes, err [B,H], persistence [B,H]); targets [B,H,...] float or byte
    frames, None: the two errors are None.  persistence[b,h] is the error of state0[b] against target h.  quality=True:
    (ssim, psnr, persistence_ssim, persistence_psnr), [B,H] each, follow (None without targets).  precision: as predict's."""
    _check_out(out)
    fm_precision_code(precision)
    _require_eval(fwd_model=fwd_model)
    _require_gpu(state0, "state0")
    _require_gpu(actions, "actions")
    if actions.dim() != 3 or actions.shape[-1] != 4 or actions.shape[0] != state0.shape[0]:
        raise _capi.NdpError("actions must be [B,H,4] with state0's B, got %s" % (tuple(actions.shape),))
    bsz, steps, dev = int(actions.shape[0]), int(actions.shape[1]), state0.device
    flat_targets = None
    if targets is not None:
        if tuple(targets.shape[:2]) != (bsz, steps):
            raise _capi.NdpError("targets must be [B,H,...] = [%d,%d,...], got %s" % (bsz, steps, tuple(targets.shape)))
        flat_targets = _images(targets, "targets")                  # row b * H + h
    rows = torch.arange(bsz, device=dev, dtype=torch.int32) * steps
    preds, errs, bases, state = [], [], [], state0
    quals = [[], [], [], []]
    for h in range(steps):
        state = _forward(fwd_model, state, actions[:, h].contiguous(), precision)
        want_bytes = out == "bytes"
        if flat_targets is not None:
            err, base_err, pred_u8 = score(state, flat_targets, rows + h, base=state0, out_bytes=want_bytes)
            errs.append(err)
            bases.append(base_err)
            if quality:
                for q, v in zip(quals, _quality(state, state0, flat_targets, target_idx=rows + h)):
                    q.append(v)
        elif want_bytes:
            pred_u8 = score(state, out_bytes=True)[2]
        preds.append(pred_u8 if want_bytes else state)
    preds = torch.stack(preds, dim=1)
    if flat_targets is None:
        return (preds, None, None) + ((None,) * 4 if quality else ())
    extra = tuple(torch.stack(q, dim=1) for q in quals) if quality else ()
    return (preds, torch.stack(errs, dim=1), torch.stack(bases, dim=1)) + extra


def rollout_schedule(T, horizon=None):
    """Pure host function: for each rollout step h = 1 .. H the tuple (starts, action_frames, target_frames) -- the start
    frames still alive at step h (0 .. T-1-h: those with a target frame left), the frame whose action each takes
    (start + h - 1) and the frame each is scored against (start + h).  horizon None: T - 1."""
    T = int(T)
    if T < 2:
        raise ValueError("a trajectory of %d frame(s) has no frame to predict: T must be >= 2" % T)
    H = T - 1 if horizon is None else int(horizon)
    if not 1 <= H <= T - 1:
        raise ValueError("horizon %d is outside 1 .. T - 1 = %d: a trajectory of %d frames has no target beyond that"
                         % (H, T - 1, T))
    steps = []
    for h in range(1, H + 1):
        starts = tuple(range(0, T - h))
        steps.append((starts, tuple(t + h - 1 for t in starts), tuple(t + h for t in starts)))
    return steps


def _maps(sched, T, b, device):
    """Per step the int32 device index maps of a batch of b trajectories whose frames are rows traj * T + frame:
    (start rows, action rows, target rows), trajectory-major."""
    traj = np.arange(b, dtype=np.int64)[:, None] * T
    return [tuple(torch.from_numpy((traj + np.asarray(col, np.int64)[None, :]).reshape(-1).astype(np.int32)).to(device)
                  for col in step) for step in sched]


QUALITY_KEYS = ("ssim", "psnr", "persistence_ssim", "persistence_psnr")


def evaluate(fwd_model, dataset, horizon=None, batch_size=16, device=None, keep=0, quality=False, precision="fp32"):
    """The multi-step prediction error over `dataset` (PushDataset / SyntheticPushDataset: images, byte frames or JPEG
    streams, which `jpeg.JpegDecoder` decodes on the device), from EVERY start frame: pass h of a batch of B trajectories
    runs the B * (T - h) starts still alive (rollout_schedule) in ONE forward call, on their own predictions of pass
    h - 1 (at h = 1 on the frames themselves), and scores them in one ndp_fm_score launch.  horizon None: T - 1.
    Returns a dict of device tensors (no host synchronisation per batch):
        one_step_mse [1]      the mean error at h = 1 (= horizon_mse[0])
        horizon_mse [H]       the mean error at h = 1 .. H, persistence_mse [H] that of "the frame does not change" (the
                              start frame against the same target), counts [H] int64 = N * (T - h)
        errors [P], persistence [P], index [P,3] int32 (trajectory, start, h)      every prediction's own values
      keep > 0: also `strips`, the first `keep` starts that live for all H steps (trajectory-major), as bytes:
        {"start" [k,128,128,3], "targets" [k,H,128,128,3], "predictions" [k,H,128,128,3]}
      quality=True: also horizon_ssim, horizon_psnr, persistence_ssim, persistence_psnr [H] (of the start frame against the
        same target) and `quality`, a dict of every prediction's own ssim, psnr, persistence_ssim, persistence_psnr [P] in
        `errors`' order: two ndp_image_quality launches per pass, the predictions against `frames` through the target
        rows, then `frames` through the start rows against the same targets.  Every other key holds the same bits.
    The means are taken in fp64 over the fp32 per-prediction values; a PSNR mean skips no value (an infinite value gives an
    infinite mean).  precision: 'fp32', or 'bf16' -- every pass with bf16 operands (NDP_FM_BF16, include/ndp.h)."""
    fm_precision_code(precision)
    _require_eval(fwd_model=fwd_model)
    if len(dataset) == 0 or int(batch_size) < 1:
        raise ValueError("evaluate needs a non-empty dataset and batch_size >= 1 (dataset: %d trajectories, batch_size %r)"
                         % (len(dataset), batch_size))
    T = int(dataset.seq_length)
    sched = rollout_schedule(T, horizon)
    H = len(sched)
    device = torch.device(device) if device is not None else next(fwd_model.parameters()).device
    model_device = next(fwd_model.parameters()).device
    if device.type != "cuda" or model_device.type != "cuda":
        raise _capi.NdpError("the forward model is on %s (device %s): ndivplanning_amd computes only on a ROCm GPU "
                             "(no CPU fallback)" % (model_device, device))
    jpeg_decoder = jpeg_frames.JpegDecoder(device, check="deferred") if jpeg_frames.is_jpeg(dataset) else None
    errs, bases = [[] for _ in range(H)], [[] for _ in range(H)]     # per step, for the means
    all_err, all_base, index = [], [], []                             # in the order computed: batch, h, trajectory, start
    quals = {k: [[] for _ in range(H)] for k in QUALITY_KEYS} if quality else {}
    all_qual = {k: [] for k in quals}
    strips = {"start": [], "targets": [], "predictions": []}
    maps, kept, first_traj = {}, 0, 0
    full = T - H                                                      # starts per trajectory that live for all H steps
    for frames, actions, b in trajectory_batches(dataset, int(batch_size), device, jpeg_decoder):
        frames = frames.view(-1, *frames.shape[2:])                  # [b*T,...]
        if b not in maps:
            maps[b] = _maps(sched, T, b, device)
        flat_actions = actions.reshape(b * T, 4)
        want = min(keep - kept, b * full) if keep > kept else 0      # strips still to take from this batch
        state, strip_preds = None, []
        for h, (starts, _, _) in enumerate(sched, start=1):
            start_rows, action_rows, target_rows = maps[b][h - 1]
            alive = len(starts)
            if h == 1:
                state = frames.index_select(0, start_rows.long())
            else:                                                     # the survivors' own predictions: drop each last start
                state = state.view(b, alive + 1, *IMAGE)[:, :alive].reshape(b * alive, *IMAGE)
            state = _forward(fwd_model, state, flat_actions.index_select(0, action_rows.long()), precision)
            err, base_err, pred_u8 = score(state, frames, target_rows, base=frames, base_idx=start_rows, out_bytes=want > 0)
            errs[h - 1].append(err)
            bases[h - 1].append(base_err)
            all_err.append(err)
            all_base.append(base_err)
            if quality:
                for k, v in zip(QUALITY_KEYS, _quality(state, frames, frames, base_idx=start_rows, target_idx=target_rows)):
                    quals[k][h - 1].append(v)
                    all_qual[k].append(v)
            index.append(np.stack([np.repeat(np.arange(first_traj, first_traj + b), alive), np.tile(np.asarray(starts), b),
                                   np.full(b * alive, h)], axis=1))
            if want > 0:
                strip_preds.append(pred_u8.view(b, alive, *FRAME)[:, :full].reshape(b * full, *FRAME)[:want])
        if want > 0:
            byte_frames = _to_bytes(frames).view(b, T, *FRAME)
            strips["start"].append(byte_frames[:, :full].reshape(b * full, *FRAME)[:want])
            strips["targets"].append(torch.stack([byte_frames[:, h:h + full].reshape(b * full, *FRAME)[:want]
                                                  for h in range(1, H + 1)], dim=1))
            strips["predictions"].append(torch.stack(strip_preds, dim=1))
            kept += want
        first_traj += b
    if jpeg_decoder is not None:
        jpeg_decoder.finish()
    per_h = [torch.cat(errs[h]) for h in range(H)]
    per_h_base = [torch.cat(bases[h]) for h in range(H)]
    result = {
        "horizon_mse": torch.cat([fp64_mean(e) for e in per_h]),
        "persistence_mse": torch.cat([fp64_mean(e) for e in per_h_base]),
        "counts": torch.tensor([int(e.numel()) for e in per_h], dtype=torch.int64, device=device),
        "errors": torch.cat(all_err), "persistence": torch.cat(all_base),
        "index": torch.from_numpy(np.concatenate(index).astype(np.int32)).to(device),
    }
    result["one_step_mse"] = result["horizon_mse"][:1].clone()
    if quality:
        for k in QUALITY_KEYS:
            name = k if k.startswith("persistence_") else "horizon_" + k
            result[name] = torch.cat([IQ.mean(torch.cat(quals[k][h])) for h in range(H)])
        result["quality"] = {k: torch.cat(v) for k, v in all_qual.items()}
    if keep > 0:
        result["strips"] = {k: torch.cat(v) for k, v in strips.items()}
    return result


def save_strips(strips, save_dir):
    """strip_NNN.png per kept start (PIL): the top row is the start frame and its targets 1 .. H, the bottom row the start
    frame and the predictions 1 .. H."""
    from PIL import Image
    os.makedirs(save_dir, exist_ok=True)
    start, targets, preds = (strips[k].cpu().numpy() for k in ("start", "targets", "predictions"))
    paths = []
    for i in range(start.shape[0]):
        top = np.concatenate([start[i]] + list(targets[i]), axis=1)
        bottom = np.concatenate([start[i]] + list(preds[i]), axis=1)
        path = os.path.join(save_dir, "strip_%03d.png" % i)
        Image.fromarray(np.concatenate([top, bottom], axis=0)).save(path)
        paths.append(path)
    return paths


def make_dataset(path, seq_length=15, seed=2, raw_jpeg=False):
    """synthetic:<N>:images|frames_u8|jpeg, or the HDF5 directory (byte frames; raw_jpeg: its JPEG streams, decoded on
    the device)."""
    return open_dataset(path, seq_length=int(seq_length), seed=seed, default_mode="images", modes=("images", "frames_u8", "jpeg"),
                        mode_error="the forward model predicts images: use synthetic:<N>:images, :frames_u8 or :jpeg, got %(mode)r",
                        push=dict(seq_length=int(seq_length), raw_uint8=not raw_jpeg, raw_jpeg=raw_jpeg))


def make_parser():
    parser = ArgumentParser(description="Multi-step prediction error (and prediction strips) of a trained forward model")
    parser.add_argument("--model", required=True, help="whole-module checkpoint (forward_autoencoder_N.pt of train_forward_model.py)")
    parser.add_argument("--data", required=True, help="trajectory directory, or synthetic:<N>:images|frames_u8|jpeg")
    parser.add_argument("--raw-jpeg", action="store_true",
                        help="read the directory's JPEG streams as they are and decode them on the GPU")
    parser.add_argument("--seq-length", type=int, default=15, help="frames per trajectory (T)")
    parser.add_argument("--horizon", type=int, default=None, help="rollout steps H (default T - 1)")
    parser.add_argument("--batch-size", type=int, default=16, help="trajectories per batch")
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--save-dir", default=None, help="write the first --num-save prediction strips here as PNG")
    parser.add_argument("--num-save", type=int, default=8)
    parser.add_argument("--quality", action="store_true",
                        help="also print SSIM and PSNR per horizon, of the model and of the persistence baseline")
    parser.add_argument("--fm-precision", choices=FM_PRECISIONS, default="fp32",
                        help="operand precision of the forward model's passes: fp32, or bf16 operands with fp32 accumulation")
    return parser


def main(argv=None, log=print):
    args = make_parser().parse_args(argv)
    device = torch.device(args.device)
    model = load_module(args.model, device)
    dataset = make_dataset(args.data, seq_length=args.seq_length, raw_jpeg=args.raw_jpeg)
    keep = args.num_save if args.save_dir else 0
    result = evaluate(model, dataset, horizon=args.horizon, batch_size=args.batch_size, device=device, keep=keep,
                      quality=args.quality, precision=args.fm_precision)
    one_step = float(result["one_step_mse"].item())
    log("val_pred_loss:", one_step, "trajectories:", len(dataset))
    rows = zip(result["horizon_mse"].tolist(), result["persistence_mse"].tolist(), result["counts"].tolist())
    for h, (model_mse, base_mse, count) in enumerate(rows, start=1):
        log("horizon %d: model_mse %.8g persistence_mse %.8g count %d" % (h, model_mse, base_mse, count))
    if args.quality:
        rows = zip(*(result[k].tolist() for k in ("horizon_ssim", "persistence_ssim", "horizon_psnr", "persistence_psnr")))
        for h, (model_ssim, base_ssim, model_psnr, base_psnr) in enumerate(rows, start=1):
            log("horizon %d: model_ssim %.8g persistence_ssim %.8g model_psnr %.8g persistence_psnr %.8g"
                % (h, model_ssim, base_ssim, model_psnr, base_psnr))
    if args.save_dir:
        paths = save_strips(result["strips"], args.save_dir)
        log("wrote %d strips to %s" % (len(paths), args.save_dir))
    return one_step


if __name__ == "__main__":
    main()
