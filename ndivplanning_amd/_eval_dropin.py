"""The body the three drop-in evaluation scripts share: `fetch_push_control_evaluation` of control_evaluation.py (open
loop), complete_eval.py (closed loop) and mpc_eval.py (model-predictive control), on `ndivplanning_amd.evaluation`.

Kept from the reference, each on purpose: the signature and the returned (avg_action_error, avg_image_loss); the seeds
(`torch.manual_seed(random_seed)`, `np.random.seed(random_seed)`, :74-75) and the CPU noise stream, drawn in the
reference's shapes and order (one upload per trajectory batch); the loader (`batch_size=evaluation.batch_size`,
unshuffled); the stdout lines; `image_error_sum` reset for every batch while the divisor is `(T-1) * len(loader)`, so
that avg_image_loss covers only the last batch (:120, :153-154)."""
import logging

import numpy as np
import torch
from torch.utils import data

from . import evaluation as E


def fetch(kind, image_encoder, fwd_model_autoencoder, generator, dataset, config):
    image_encoder.eval()
    fwd_model_autoencoder.eval()
    generator.eval()
    seed, k, nz, bs, r, th = E.eval_settings(kind, config, dataset, generator)
    gpu_id = E.device_of(config)
    models = E.EvalModels(image_encoder, fwd_model_autoencoder, generator, gpu_id, fm_precision=E.fm_precision_of(config),
                          enc_precision=E.enc_precision_of(config))
    t1 = int(dataset.seq_length) - 1
    torch.manual_seed(seed)
    np.random.seed(seed)
    loader = data.DataLoader(dataset, batch_size=bs, shuffle=False, **E.jpeg.loader_kwargs(dataset))
    shapes = E.noise_piece_shapes(kind, bs, dataset.seq_length, k, nz, r, th)
    # the optional `mpc.cem` mapping turns the cross-entropy planner on (evaluation.CemSettings; absent: off)
    cem = E.cem_from_config(config) if kind == "mpc" else None
    # the optional `mpc.grad` mapping turns the gradient stage on (evaluation.GradSettings; absent: off)
    grad = E.grad_from_config(config) if kind == "mpc" else None
    action_error_sum = torch.zeros(1, dtype=torch.float32, device=models.device)
    image_error_sum = None
    for i, inputs in enumerate(loader):
        images, _, actions, _ = inputs
        if kind == "mpc":
            logging.info("trajectory: %d", i)
        else:
            print("trajectory: ", i)
        noise = E.draw_noise(shapes, pin=True)
        actions = actions.to(models.device).float()
        if kind == "open":
            res = E.open_loop(models, images, actions, k, noise, action_error_acc=action_error_sum)
        elif kind == "closed":
            res = E.closed_loop(models, images, actions, k, noise, action_error_acc=action_error_sum, on_step=print)
        else:
            # seed: with `cem`, the device's normal draws, one stream per trajectory (unread without it: the noise is given)
            res = E.mpc_plan(models, images, actions, r, th, noise=noise, on_step=print, cem=cem, seed=seed + i, grad=grad)
            models.mse(actions[:, :t1].contiguous(), res["actions"], 1, t1 * 4, acc=action_error_sum)
        image_error_sum = res["image_error_sum"][0]
        if kind != "open":
            print(action_error_sum[0])                     # one host sync per batch, as the reference's print
    if image_error_sum is None:
        raise ValueError("the evaluation dataset is empty")
    models.finish_jpeg()
    avg_action_error = action_error_sum[0] / (t1 * len(loader))
    avg_image_loss = image_error_sum / (t1 * len(loader))
    return avg_action_error.item(), avg_image_loss.item()
