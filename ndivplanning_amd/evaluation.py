"""Evaluation of the trained models -- the engine under the reference's three evaluation scripts
(control_evaluation.py: open loop, complete_eval.py: closed loop, mpc_eval.py: model-predictive control).

`EvalModels` packs the image encoder, the forward model and the generator once into the flat vectors their kernels read
(the modules' own pack helpers) and calls the kernels directly: `ndp_encoder_forward_lp`, `ndp_g_forward`, `ndp_fm_forward_lp`
(eval mode, in the precisions `enc_precision` / `fm_precision` name; 'fp32' is `ndp_encoder_forward` / `ndp_fm_forward`), and the evaluation glue of csrc/ndp_eval.inc (`ndp_eval_*`: pair MSEs, rollout selection, the generator's
code input, byte-frame normalisation).  Every result is a device tensor.  `mpc_plan` on frames and actions that are
already on the device makes no host synchronisation until its results are read; inputs on the host are uploaded with
ordinary (blocking) copies, and open_loop / closed_loop upload small index tensors at every step.

What the loops deduplicate against the reference, with the same arithmetic per image:
  * the goal image is encoded once per trajectory (the reference encodes it once per generator call: R x Th times per
    planning step in mpc_eval.py:131-136, T-1 times in control_evaluation.py:104-106 and complete_eval.py:120-121);
  * at ts = 0 of a planning step one image per trajectory is encoded and its code broadcast to the R rollouts
    (mpc_eval.py:125-139 encodes R identical copies);
  * the rollouts are scored and chosen on the device (mpc_eval.py:159-165: one host sync per rollout), and the chosen
    rollout's ts = 0 prediction becomes the next state (mpc_eval.py:167-169 recomputes it with one more forward call);
  * `mpc_plan` runs B trajectories at once: every launch serves B * R images.

The planner is one planning step, `_plan_once`, under every entry point (mpc_plan per frame of a recorded trajectory,
plan_step / MpcController per live observation), on two rollouts: `_rollout_generator`, the closed loop encode ->
generator -> forward model that leaves its actions in seq [steps,B,R,4], and `_rollout_open`, the forward model alone on
a given seq.  Population 0 is the first; the last ndp_eval_score_select chooses.

Beyond the reference: `cem=CemSettings(...)` on mpc_plan / plan_step / MpcController refines the rollouts' action
sequences by the cross-entropy method before the choice (csrc/ndp_plan.inc: ndp_plan_cem_update, ndp_normal_noise): rounds
of select -> update -> open-loop rollout between population 0 and the choice.  Off by default: no rounds, and then
nothing here launches anything else than the reference's planner needs.
Two further opt-in fields of CemSettings: `weighting="mppi"` weighs the elites by exp(-(e - e_best) / temperature)
(ndp_plan_update), and `warm_start=True` starts a planning step from the previous step's fit shifted by one action
(ndp_plan_warm; plan_step's `prior`, carried by mpc_plan and MpcController).
`grad=GradSettings(...)` on the same entry points adds a gradient stage before the choice (_grad_stage; ndp_plan_goal_grad,
ndp_plan_grad_gather, ndp_plan_grad_step and the forward model's ndp_fm_input_grads): the best rows of the population are
refined by gradient descent on the planner's score and replace the worst ones.  Off by default, with or without `cem`.
"""
import torch

from . import _capi, jpeg
from ._eval_io import (ENC_PRECISIONS, FM_PRECISIONS, config_cli, device_of, enc_precision_code,  # noqa: F401 (device_of,
                       enc_precision_of, fm_precision_code, fm_precision_of, load_eval_models)   # *_precision_of: for the scripts)
from .models.forward_encoder import pack_module
from .models.image_autoencoder import pack_encoder_params

IMAGE_VALUES = 3 * 128 * 128
MIN_ERROR = 10000000000          # mpc_eval.py:129: the rollout rule's sentinel (exact in fp32)


def _ptr(t):
    return _capi.ptr(t)


class EvalModels:
    """The three trained modules, packed once for the kernels (eval mode: BatchNorm with running statistics)."""

    def __init__(self, image_encoder, fwd_model_autoencoder, generator, device=None, fm_precision="fp32", enc_precision="fp32"):
        """fm_precision: 'fp32', or 'bf16' -- `forward` (every pass of the planner's rollouts) runs the nine stride-2 layers
        with bf16 operands and fp32 accumulation (NDP_FM_BF16, include/ndp.h); forward_keep / input_grads stay fp32.
        enc_precision: 'fp32', or 'bf16' -- `encode` (the state codes and the goal code alike) runs conv2..conv6 with bf16
        operands and bf16 maps (NDP_ENC_BF16, include/ndp.h); the weights are rounded once, here.  The two combine freely,
        and with cem= and grad= (the gradient stage never passes through the encoder)."""
        self._fm_precision_code = fm_precision_code(fm_precision)
        self.fm_precision = fm_precision
        self._enc_precision_code = enc_precision_code(enc_precision)
        self.enc_precision = enc_precision
        if device is None:
            device = next(fwd_model_autoencoder.parameters()).device
        device = torch.device(device)
        if device.type != "cuda":
            raise _capi.NdpError("evaluation runs only on a ROCm GPU (got %s): there is no CPU path" % device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.lib = _capi.load()
        self.device = device
        for m in (image_encoder, fwd_model_autoencoder, generator):
            m.eval()
        self.enc_params = pack_encoder_params(image_encoder).to(device).contiguous()
        if self.enc_params.numel() != self.lib.ndp_encoder_param_floats():
            raise _capi.NdpError("encoder parameter count %d != %d" % (self.enc_params.numel(),
                                                                     self.lib.ndp_encoder_param_floats()))
        self.fm_params, self.fm_stats = pack_module(fwd_model_autoencoder, device)
        self.noise_dim = int(generator.noise_dim)
        if not 1 <= self.noise_dim <= _capi.MAX_NOISE_DIM:
            raise _capi.NdpError("generator noise_dim=%d outside 1..%d" % (self.noise_dim, _capi.MAX_NOISE_DIM))
        with torch.no_grad():
            self.g_params = generator.flat_parameters().detach().to(device).clone()
        self._enc_ws = None
        self._enc_lp = None              # the bf16 weights of conv2..conv6 (ndp_encoder_pack_params_lp)
        if self._enc_precision_code:
            self._enc_lp = torch.empty(self.lib.ndp_encoder_lp_weight_bytes(), dtype=torch.uint8, device=device)
            with _capi.on_device(device):
                _capi.check(self.lib.ndp_encoder_pack_params_lp(_ptr(self.enc_params), _ptr(self._enc_lp), self._stream()),
                            "ndp_encoder_pack_params_lp")
        self._fm_ws, self._fm_n = None, 0
        self._fm_lp = None               # the bf16 weights (ndp_fm_pack_params_lp), rebuilt with every ndp_fm_pack_params
        self._mse_ws = None

    # ------------------------------------------------------------------ one launch (or a few) each
    def _stream(self):
        return _capi.stream_ptr(self.device)

    def encode(self, images):
        """images [n,3,128,128] fp32 -> codes [n,128] (Encoder.forward in eval mode)."""
        n = int(images.shape[0])
        need = self.lib.ndp_encoder_workspace_floats(n)
        if self._enc_ws is None or self._enc_ws.numel() < need:
            self._enc_ws = torch.empty(need, dtype=torch.float32, device=self.device)
        codes = torch.empty(n, 128, dtype=torch.float32, device=self.device)
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_encoder_forward_lp(_ptr(self.enc_params), _ptr(images), None, n, self._enc_precision_code,
                                                        _ptr(self._enc_lp), _ptr(codes), _ptr(self._enc_ws), self._stream()),
                        "ndp_encoder_forward_lp")
        return codes

    def generate(self, code, noise, code_rep=1, out=None):
        """code [rows,256], noise [rows*code_rep, nz] -> actions [rows*code_rep, 4] (Decoder.forward of the generator),
        written to `out` (contiguous, rows*code_rep*4 floats in any shape) when given.  Returns `out`."""
        m = int(code.shape[0]) * int(code_rep)
        if out is None:
            out = torch.empty(m, 4, dtype=torch.float32, device=self.device)
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_g_forward(_ptr(self.g_params), self.noise_dim, _ptr(code), 256, int(code_rep), _ptr(noise),
                                               self.noise_dim, m, None, _ptr(out), self._stream()), "ndp_g_forward")
        return out

    def forward(self, state, actions):
        """state [n,3,128,128], actions [n,4] -> state + residual (ForwardAutoencoder.forward in eval mode)."""
        n = int(state.shape[0])
        if n > 8192:
            raise _capi.NdpError("the forward model takes at most 8192 images per call, got %d" % n)
        if self._fm_ws is None or self._fm_n < n:
            self._fm_ws = torch.empty(self.lib.ndp_fm_workspace_floats(n), dtype=torch.float32, device=self.device)
            self._fm_n = n
            with _capi.on_device(self.device):
                _capi.check(self.lib.ndp_fm_pack_params(_ptr(self.fm_params), _ptr(self._fm_ws), self._stream()),
                            "ndp_fm_pack_params")
                if self._fm_precision_code:
                    if self._fm_lp is None:
                        self._fm_lp = torch.empty(self.lib.ndp_fm_lp_weight_bytes(), dtype=torch.uint8, device=self.device)
                    _capi.check(self.lib.ndp_fm_pack_params_lp(_ptr(self.fm_params), _ptr(self._fm_ws), _ptr(self._fm_lp),
                                                               self._stream()), "ndp_fm_pack_params_lp")
        out = torch.empty(n, 3, 128, 128, dtype=torch.float32, device=self.device)
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_fm_forward_lp(_ptr(self.fm_params), _ptr(self.fm_stats), _ptr(state), None, _ptr(actions), n,
                                                   self._fm_precision_code, _ptr(self._fm_lp), _ptr(out), _ptr(self._fm_ws),
                                                   self._stream()), "ndp_fm_forward_lp")
        return out

    def g_input(self, state_code, state_rep, goal_code, goal_rep, rows):
        """[rows,256]: row r = cat(state_code[r // state_rep], goal_code[r // goal_rep])."""
        out = torch.empty(int(rows), 256, dtype=torch.float32, device=self.device)
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_eval_g_input(_ptr(state_code), int(state_code.shape[0]), int(state_rep), _ptr(goal_code),
                                                  int(goal_code.shape[0]), int(goal_rep), int(rows), _ptr(out),
                                                  self._stream()), "ndp_eval_g_input")
        return out

    def jpeg_decoder(self):
        """The device's JPEG decoder (made on first use): failed frames raise at the next batch's decode or at
        finish_jpeg()."""
        if getattr(self, "_jpeg", None) is None:
            self._jpeg = jpeg.JpegDecoder(self.device, check="deferred")
        return self._jpeg

    def finish_jpeg(self):
        """Raise for JPEG frames of the last batch that did not decode (nothing to do without a decoder)."""
        if getattr(self, "_jpeg", None) is not None:
            self._jpeg.finish()

    def images(self, frames):
        """[n,3,128,128] fp32 from float NCHW images or byte frames [n,128,128,3] (normalised as the loader would)."""
        if frames.dtype == torch.uint8:
            if tuple(frames.shape[1:]) != (128, 128, 3):
                raise _capi.NdpError("byte frames must be [n,128,128,3], got %s" % (tuple(frames.shape),))
            x = frames.to(self.device).contiguous()
            n = int(x.shape[0])
            out = torch.empty(n, 3, 128, 128, dtype=torch.float32, device=self.device)
            with _capi.on_device(self.device):
                _capi.check(self.lib.ndp_eval_frames_u8(_ptr(x), n, _ptr(out), self._stream()), "ndp_eval_frames_u8")
            return out
        if tuple(frames.shape[1:]) != (3, 128, 128):
            raise _capi.NdpError("images must be [n,3,128,128], got %s" % (tuple(frames.shape),))
        return frames.to(self.device).float().contiguous()

    def mse(self, a, b, n_pairs, values, group=1, a_idx=None, b_idx=None, out=None, acc=None):
        """ndp_eval_mse: MSE of every `group` consecutive pairs (a[a_idx[p]], b[b_idx[p]]), written to `out` and/or added
        to `acc` in fp32.  Returns `out` (allocated when not given)."""
        n_pairs = int(n_pairs)
        if out is None:
            out = torch.empty(n_pairs // int(group), dtype=torch.float32, device=self.device)
        need = self.lib.ndp_eval_mse_ws_floats(n_pairs)
        if self._mse_ws is None or self._mse_ws.numel() < need:
            self._mse_ws = torch.empty(max(need, 64), dtype=torch.float32, device=self.device)
        n_a = a.numel() // int(values)
        n_b = b.numel() // int(values)
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_eval_mse(_ptr(a), n_a, _ptr(b), n_b, _ptr(a_idx), _ptr(b_idx), n_pairs, int(values),
                                              int(group), _ptr(out), _ptr(acc), _ptr(self._mse_ws), self._stream()),
                        "ndp_eval_mse")
        return out

    def score_select(self, pred, n_traj, rollouts, target, actions0, pred0, forced, err, choice, action_out, pred_out):
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_eval_score_select(_ptr(pred), int(n_traj), int(rollouts), _ptr(target),
                                                       int(target.shape[0]), None, IMAGE_VALUES, _ptr(actions0), _ptr(pred0),
                                                       _ptr(forced), _ptr(err), _ptr(choice), _ptr(action_out),
                                                       _ptr(pred_out), self._stream()), "ndp_eval_score_select")

    def uniform(self, n, seed):
        """n floats of U[0,1) on the device (ndp_uniform_noise, counter offset 0)."""
        out = torch.empty(max(int(n), 1), dtype=torch.float32, device=self.device)
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_uniform_noise(_ptr(out), int(n), int(seed) & 0xFFFFFFFFFFFFFFFF, None, self._stream()),
                        "ndp_uniform_noise")
        return out

    def normal(self, n, seed):
        """n standard normal floats on the device (ndp_normal_noise).  They come from counter offset 1 of `seed`'s
        stream, so they are independent of uniform(n, seed), which reads offset 0."""
        if getattr(self, "_normal_offset", None) is None:
            self._normal_offset = torch.ones(1, dtype=torch.int32, device=self.device)
        out = torch.empty(max(int(n), 1), dtype=torch.float32, device=self.device)
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_normal_noise(_ptr(out), max(int(n), 1), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                  _ptr(self._normal_offset), self._stream()), "ndp_normal_noise")
        return out

    def cem_update(self, err, seq_in, normal, settings, first, mean, std, seq_out, best_err, elite_idx=None):
        """ndp_plan_cem_update on the population seq_in [Th,B,R,4] with the scores err [B,R]: refits mean / std
        [B,Th,4] (in/out unless `first`), writes the next population to seq_out and the running minimum to best_err."""
        th, b, r = int(seq_in.shape[0]), int(seq_in.shape[1]), int(seq_in.shape[2])
        low, high = (_capi.c_float * 4)(*settings.low), (_capi.c_float * 4)(*settings.high)
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_plan_cem_update(_ptr(err), _ptr(seq_in), _ptr(normal), b, r, th, settings.elite_count(r),
                                                     1 if first else 0, settings.momentum, settings.min_std, low, high,
                                                     _ptr(mean), _ptr(std), _ptr(seq_out), _ptr(best_err), _ptr(elite_idx),
                                                     self._stream()), "ndp_plan_cem_update")

    def plan_update(self, err, seq_in, normal, settings, smooth, first, mean, std, seq_out, best_err, elite_idx=None):
        """ndp_plan_update: cem_update with settings.weighting / settings.temperature and the two flags apart: `smooth`
        (the refit is smoothed against the mean / std given) and `first` (best_err is only written)."""
        th, b, r = int(seq_in.shape[0]), int(seq_in.shape[1]), int(seq_in.shape[2])
        low, high = (_capi.c_float * 4)(*settings.low), (_capi.c_float * 4)(*settings.high)
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_plan_update(_ptr(err), _ptr(seq_in), _ptr(normal), b, r, th, settings.elite_count(r),
                                                 WEIGHTINGS.index(settings.weighting), settings.temperature or 0.0,
                                                 1 if smooth else 0, 1 if first else 0, settings.momentum, settings.min_std,
                                                 low, high, _ptr(mean), _ptr(std), _ptr(seq_out), _ptr(best_err),
                                                 _ptr(elite_idx), self._stream()), "ndp_plan_update")

    def plan_warm(self, mean_prev, std_prev, normal, settings, mean, std, warm):
        """ndp_plan_warm: the previous planning step's fit mean_prev / std_prev [B,steps_prev,4] shifted by one action into
        mean / std [B,steps,4], and the rows warm [steps,B,W,4] the next population receives (row 0: the clamped mean)."""
        th, b, w = int(warm.shape[0]), int(warm.shape[1]), int(warm.shape[2])
        low, high = (_capi.c_float * 4)(*settings.low), (_capi.c_float * 4)(*settings.high)
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_plan_warm(_ptr(mean_prev), _ptr(std_prev), _ptr(normal), b, w, int(mean_prev.shape[1]),
                                               th, settings.carried_floor(), low, high, _ptr(mean), _ptr(std), _ptr(warm),
                                               self._stream()), "ndp_plan_warm")

    # ------------------------------------------------------------------ the gradient stage (`grad`)
    def forward_keep(self, state, actions, slot):
        """forward() on the workspace of horizon step `slot`, which keeps the pass's activations for input_grads(slot).
        Every slot has a workspace of its own (made and packed on first use, kept), so Th passes can wait for one
        backward chain."""
        n = int(state.shape[0])
        if n > 8192:
            raise _capi.NdpError("the forward model takes at most 8192 images per call, got %d" % n)
        keep = self.__dict__.setdefault("_fm_keep", [])
        while len(keep) <= slot:
            keep.append({"ws": None, "n": 0})
        entry = keep[slot]
        if entry["ws"] is None or entry["n"] < n:
            entry["ws"] = torch.empty(self.lib.ndp_fm_workspace_floats(n), dtype=torch.float32, device=self.device)
            entry["n"] = n
            with _capi.on_device(self.device):
                _capi.check(self.lib.ndp_fm_pack_params(_ptr(self.fm_params), _ptr(entry["ws"]), self._stream()),
                            "ndp_fm_pack_params")
        out = torch.empty(n, 3, 128, 128, dtype=torch.float32, device=self.device)
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_fm_forward(_ptr(self.fm_params), _ptr(self.fm_stats), _ptr(state), _ptr(actions), n, 0,
                                                _ptr(out), _ptr(entry["ws"]), self._stream()), "ndp_fm_forward")
        return out

    def input_grads(self, d_out, slot, d_state, d_actions):
        """ndp_fm_input_grads through the pass forward_keep(..., slot) ran last: d_out [n,3,128,128] -> d_state (or None)
        and d_actions [n,4] (or None).  One call per forward_keep."""
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_fm_input_grads(_ptr(self.fm_params), _ptr(d_out), int(d_out.shape[0]), _ptr(d_state),
                                                    _ptr(d_actions), _ptr(self._fm_keep[slot]["ws"]), self._stream()),
                        "ndp_fm_input_grads")

    def goal_grad(self, pred, goal, rows_per_goal, err, d_pred):
        """ndp_plan_goal_grad: err [n] = the MSE of pred row i against goal row i // rows_per_goal (score_select's bits),
        d_pred = its gradient (may be `pred` itself)."""
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_plan_goal_grad(_ptr(pred), int(pred.shape[0]), _ptr(goal), int(goal.shape[0]),
                                                    int(rows_per_goal), _ptr(err), _ptr(d_pred), self._stream()),
                        "ndp_plan_goal_grad")

    def grad_gather(self, err, seq, src, dst, seq_g, m, v):
        """ndp_plan_grad_gather: the G = seq_g.shape[2] best rows of seq [Th,B,R,4] by err [B,R] into seq_g [Th,B,G,4], their
        indices into src [B,G], the G worst rows' into dst [B,G]; m, v zeroed."""
        th, b, r = int(seq.shape[0]), int(seq.shape[1]), int(seq.shape[2])
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_plan_grad_gather(_ptr(err), _ptr(seq), b, r, th, int(seq_g.shape[2]), _ptr(src), _ptr(dst),
                                                      _ptr(seq_g), _ptr(m), _ptr(v), self._stream()), "ndp_plan_grad_gather")

    def grad_step(self, grad, seq_g, m, v, err_g, t, settings, curve_out=None, dst=None, seq_full=None):
        """ndp_plan_grad_step: update number t (from 1) of seq_g [Th,B,G,4] along grad, by settings.optimizer; curve_out
        [B,G] receives err_g; with dst and seq_full the result also goes to rows dst of the population seq_full."""
        th, b, g = int(seq_g.shape[0]), int(seq_g.shape[1]), int(seq_g.shape[2])
        low, high = (_capi.c_float * 4)(*settings.low), (_capi.c_float * 4)(*settings.high)
        with _capi.on_device(self.device):
            _capi.check(self.lib.ndp_plan_grad_step(_ptr(grad), _ptr(seq_g), _ptr(m), _ptr(v), _ptr(err_g), b, g, th, int(t),
                                                    OPTIMIZERS.index(settings.optimizer), settings.lr, settings.beta1,
                                                    settings.beta2, settings.eps, low, high, _ptr(curve_out), _ptr(dst),
                                                    _ptr(seq_full), 0 if seq_full is None else int(seq_full.shape[2]),
                                                    self._stream()), "ndp_plan_grad_step")


# ---------------------------------------------------------------------- the reference's noise stream (CPU)
def noise_piece_shapes(kind, batch, seq_length, num_sample, noise_dim, rollouts=None, horizon=None):
    """The shapes of the `torch.FloatTensor(N, num_sample, noise_dim).uniform_()` draws of diverse_sampling for ONE
    loader batch, in the reference's order:
      open    control_evaluation.py:112: N = batch * (T-1), once
      closed  complete_eval.py:126: N = batch, once per step
      mpc     mpc_eval.py:141: N = rollouts, once per horizon step of every planning step (batch 1)
      mpc_gym MPC_gym_eval.py:141,188: N = rollouts, `horizon` times per planning step -- the horizon does not shrink
              towards the end of the trajectory (batch 1, num_sample 1: the `.squeeze(1)` of :215 needs it)."""
    t1 = int(seq_length) - 1
    if kind == "mpc_gym":
        if int(num_sample) != 1:
            raise ValueError("MPC_gym_eval needs evaluation.num_sample == 1 (MPC_gym_eval.py:215 squeezes the sample axis "
                             "of the [R,K,4] actions)")
        return [(rollouts, num_sample, noise_dim)] * (t1 * int(horizon))
    if kind == "open":
        return [(batch * t1, num_sample, noise_dim)]
    if kind == "closed":
        return [(batch, num_sample, noise_dim)] * t1
    if kind == "mpc":
        shapes = []
        for image_num in range(t1):
            shapes += [(rollouts, num_sample, noise_dim)] * min(int(horizon), t1 - image_num)   # mpc_eval.py:131
        return shapes
    raise ValueError("kind must be 'open', 'closed', 'mpc' or 'mpc_gym'")


def draw_noise(shapes, pin=False):
    """Draw the pieces from torch's global CPU generator in order, as the reference does, into one flat (optionally
    pinned) buffer: one upload per loader batch instead of one per piece."""
    total = sum(a * b * c for a, b, c in shapes)
    out = torch.empty(total, dtype=torch.float32, pin_memory=bool(pin) and torch.cuda.is_available())
    off = 0
    for s in shapes:
        n = s[0] * s[1] * s[2]
        out[off:off + n].copy_(torch.FloatTensor(*s).uniform_().reshape(-1))
        off += n
    return out


def reference_noise_schedule(kind, random_seed, num_batches, batch, seq_length, num_sample, noise_dim, rollouts=None,
                             horizon=None):
    """The complete CPU noise stream of a reference evaluation run, without a GPU: `torch.manual_seed(random_seed)`
    (:74), the one draw a DataLoader iterator takes from the global generator for its base seed, then every loader
    batch's pieces.  Returns one flat tensor per loader batch (what the drop-ins upload)."""
    torch.manual_seed(int(random_seed))
    loader = torch.utils.data.DataLoader(range(int(num_batches) * int(batch)), batch_size=int(batch), shuffle=False)
    shapes = noise_piece_shapes(kind, batch, seq_length, num_sample, noise_dim, rollouts, horizon)
    return [draw_noise(shapes) for _ in loader]


# ---------------------------------------------------------------------- the three loops
def _frames(models, frames):
    """[B,T,...] float NCHW, bytes HWC or JPEG streams (jpeg.JpegFrames) -> fp32 [B*T,3,128,128] on the device, once per
    trajectory batch."""
    b, t = int(frames.shape[0]), int(frames.shape[1])
    if isinstance(frames, jpeg.JpegFrames):
        frames = models.jpeg_decoder().decode_frames(frames)
    return models.images(frames.reshape(b * t, *frames.shape[2:])), b, t


def _idx(values, device):
    return torch.tensor(values, dtype=torch.int32).to(device, non_blocking=True)


def _step_targets(models, pred, imgs, b, t, image_num, out, acc):
    """image_error = mse(state_fut_hat, state_fut) of the open and closed loops (control_evaluation.py:122-132,
    complete_eval.py:108-141): against frame image_num + 1, and at the last step against state_target [B,1,...], which
    broadcasts against the [B,...] prediction (B^2 pairs; the mean over all of them)."""
    if image_num != t - 2:
        tgt = _idx([bb * t + image_num + 1 for bb in range(b)], models.device)
        models.mse(pred, imgs, b, IMAGE_VALUES, group=b, b_idx=tgt, out=out, acc=acc)
    else:
        a_idx = _idx([j for i in range(b) for j in range(b)], models.device)
        b_idx = _idx([i * t + t - 1 for i in range(b) for j in range(b)], models.device)
        models.mse(pred, imgs, b * b, IMAGE_VALUES, group=b * b, a_idx=a_idx, b_idx=b_idx, out=out, acc=acc)


def open_loop(models, frames, actions, num_sample, noise, action_error_acc=None):
    """control_evaluation.py:91-147 for one loader batch.  frames [B,T,...], actions [B,T,4], noise: the flat
    [B*(T-1), K, nz] draw.  Returns a dict of device tensors: action_hat [B,(T-1)K,4], image_errors [T-1],
    image_error_sum [1] (reset per batch, control_evaluation.py:120), action_error [1]."""
    imgs, b, t = _frames(models, frames)
    k, t1 = int(num_sample), t - 1
    codes = models.encode(imgs).view(b, t, 128)            # the T-1 states and the goal, each once
    code_in = torch.cat([codes[:, :t1], codes[:, t1:].expand(b, t1, 128)], dim=2).reshape(b * t1, 256)
    action_hat = models.generate(code_in, noise.to(models.device, non_blocking=True), code_rep=k).view(b, t1 * k, 4)
    state = imgs.view(b, t, -1)[:, 0].contiguous()
    image_errors = torch.empty(t1, dtype=torch.float32, device=models.device)
    image_error_sum = torch.zeros(1, dtype=torch.float32, device=models.device)
    for image_num in range(t1):
        # row image_num of the (T-1)*K generated rows, also when K > 1 (control_evaluation.py:128)
        pred = models.forward(state, action_hat[:, image_num].contiguous())
        _step_targets(models, pred, imgs, b, t, image_num, image_errors[image_num:image_num + 1], image_error_sum)
        state = pred
    want = torch.repeat_interleave(actions.to(models.device).float()[:, :t1], repeats=k, dim=1).contiguous()
    action_error = models.mse(want, action_hat, b, t1 * k * 4, group=b, acc=action_error_acc)
    return {"action_hat": action_hat, "image_errors": image_errors, "image_error_sum": image_error_sum,
            "action_error": action_error}


def closed_loop(models, frames, actions, num_sample, noise, action_error_acc=None, on_step=None):
    """complete_eval.py:91-157 for one loader batch (num_sample 1: the reference's forward-model call needs [B,4]
    actions).  noise: the T-1 flat [B, 1, nz] draws back to back.  Returns the dict of open_loop."""
    if int(num_sample) != 1:
        raise ValueError("closed-loop evaluation needs evaluation.num_sample == 1 (complete_eval.py:138 feeds the "
                         "[B,K,4] actions to the forward model)")
    imgs, b, t = _frames(models, frames)
    t1, nz = t - 1, models.noise_dim
    noise = noise.to(models.device, non_blocking=True)
    goal_code = models.encode(imgs.view(b, t, -1)[:, t1].contiguous().view(b, 3, 128, 128))
    state = imgs.view(b, t, -1)[:, 0].contiguous().view(b, 3, 128, 128)
    steps = torch.empty(t1, b, 4, dtype=torch.float32, device=models.device)
    image_errors = torch.empty(t1, dtype=torch.float32, device=models.device)
    image_error_sum = torch.zeros(1, dtype=torch.float32, device=models.device)
    for image_num in range(t1):
        if on_step is not None:
            on_step(image_num)
        code_in = models.g_input(models.encode(state), 1, goal_code, 1, b)
        act = models.generate(code_in, noise[image_num * b * nz:(image_num + 1) * b * nz])
        steps[image_num].copy_(act)
        pred = models.forward(state, act)
        _step_targets(models, pred, imgs, b, t, image_num, image_errors[image_num:image_num + 1], image_error_sum)
        state = pred
    action_hat = steps.transpose(0, 1).contiguous()       # torch.cat(action_list, dim=1), complete_eval.py:146
    want = actions.to(models.device).float()[:, :t1].contiguous()
    action_error = models.mse(want, action_hat, b, t1 * 4, group=b, acc=action_error_acc)
    return {"action_hat": action_hat, "image_errors": image_errors, "image_error_sum": image_error_sum,
            "action_error": action_error}


# ---------------------------------------------------------------------- cross-entropy refinement of the proposals
class CemSettings:
    """The opt-in planner of mpc_plan / plan_step / MpcController (`cem=`): `iterations` rounds of the cross-entropy
    method after the first population.  Each round refits a diagonal Gaussian over the Th x 4 action sequence to the
    `elites` best rollouts (ndp_plan_cem_update), resamples R - 1 sequences from it beside the best one, and scores them
    with Th open-loop forward-model passes.
      iterations  rounds after population 0 (0: population 0 alone, today's planner bit for bit)
      elites      rollouts the Gaussian is fitted to; None: max(1, R // 4)
      momentum    weight of the previous fit in the smoothed one, 0 <= momentum < 1
      min_std     floor of the fitted deviation
      proposal    population 0: "generator" (the closed-loop generator rollouts) or "uniform" (low + (high - low) * u
                  from the same noise stream, the baseline)
      low, high   bounds of the 4 action components: one number for all, or 4
      weighting   "elites": the `elites` best count equally (the cross-entropy refit); "mppi": they are weighed by
                  exp(-(e - e_best) / temperature) (ndp_plan_update)
      temperature None; with "mppi" required, finite and > 0 (in fp32 too).  It is absolute, on the scale of
                  ndp_eval_score_select's err, the pixel MSE of normalised images; there is no default because nobody has
                  measured one
      warm_start  False; True: a planning step starts from the previous step's fit shifted by one action (ndp_plan_warm):
                  it is the prior the first refit smooths against, and `warm_rows` rows of population 0 are drawn from it.
                  Needs iterations >= 1: without a refit there is no fit to carry
      warm_rows   rows R - W .. R - 1 of population 0 that the carried fit replaces; None: max(1, R // 4); 1 <= W <= R - 1
      warm_std    floor of the carried deviation; None: min_std.  The fit collapses towards min_std within a planning
                  step, so the carried one is widened again to keep exploring
    The defaults are hyperparameters, not measurements."""

    FIELDS = ("iterations", "elites", "momentum", "min_std", "proposal", "low", "high", "weighting", "temperature",
              "warm_start", "warm_rows", "warm_std")

    def __init__(self, iterations=3, elites=None, momentum=0.1, min_std=0.05, proposal="generator", low=-1.0, high=1.0,
                 weighting="elites", temperature=None, warm_start=False, warm_rows=None, warm_std=None):
        def integer(v, name):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError("cem.%s must be an integer, got %r" % (name, v))
            return int(v)

        def four(v, name):
            vals = [float(x) for x in v] if hasattr(v, "__len__") else [float(v)] * 4
            if len(vals) != 4 or any(x != x or x in (float("inf"), float("-inf")) for x in vals):
                raise ValueError("cem.%s must be one finite number or 4, got %r" % (name, v))
            return tuple(vals)

        self.iterations = integer(iterations, "iterations")
        if self.iterations < 0:
            raise ValueError("cem.iterations must be >= 0, got %d" % self.iterations)
        self.elites = None if elites is None else integer(elites, "elites")
        if self.elites is not None and not 1 <= self.elites <= _capi.MAX_SAMPLES:
            raise ValueError("cem.elites must lie in 1..%d (and not above the rollouts), got %d"
                             % (_capi.MAX_SAMPLES, self.elites))
        self.momentum, self.min_std = float(momentum), float(min_std)
        if not 0.0 <= self.momentum < 1.0:
            raise ValueError("cem.momentum must lie in [0, 1), got %r" % (momentum,))
        if not 0.0 <= self.min_std < float("inf"):
            raise ValueError("cem.min_std must be finite and >= 0, got %r" % (min_std,))
        if proposal not in ("generator", "uniform"):
            raise ValueError("cem.proposal must be 'generator' or 'uniform', got %r" % (proposal,))
        self.proposal = proposal
        self.low, self.high = four(low, "low"), four(high, "high")
        if any(lo > hi for lo, hi in zip(self.low, self.high)):
            raise ValueError("cem.low must not exceed cem.high, got %r and %r" % (self.low, self.high))
        if weighting not in WEIGHTINGS:
            raise ValueError("cem.weighting must be 'elites' or 'mppi', got %r" % (weighting,))
        self.weighting = weighting
        self.temperature = None if temperature is None else float(temperature)
        if weighting == "mppi":
            # the kernel reads it as fp32: it must be finite and > 0 there too
            if self.temperature is None or not 0.0 < _capi.c_float(self.temperature).value < float("inf"):
                raise ValueError("cem.weighting 'mppi' needs cem.temperature finite and > 0 (in fp32), got %r" % (temperature,))
        elif self.temperature is not None:
            raise ValueError("cem.temperature is read only with cem.weighting 'mppi', got %r" % (temperature,))
        if not isinstance(warm_start, bool):
            raise ValueError("cem.warm_start must be true or false, got %r" % (warm_start,))
        self.warm_start = warm_start
        if self.warm_start and self.iterations < 1:
            raise ValueError("cem.warm_start needs cem.iterations >= 1: without a refit there is no fit to carry")
        self.warm_rows = None if warm_rows is None else integer(warm_rows, "warm_rows")
        self.warm_std = None if warm_std is None else float(warm_std)
        if not self.warm_start and (self.warm_rows is not None or self.warm_std is not None):
            raise ValueError("cem.warm_rows and cem.warm_std are read only with cem.warm_start")
        if self.warm_rows is not None and not 1 <= self.warm_rows <= _capi.MAX_SAMPLES - 1:
            raise ValueError("cem.warm_rows must lie in 1..%d (and below the rollouts), got %d"
                             % (_capi.MAX_SAMPLES - 1, self.warm_rows))
        if self.warm_std is not None and not 0.0 <= self.warm_std < float("inf"):
            raise ValueError("cem.warm_std must be finite and >= 0, got %r" % (warm_std,))

    @classmethod
    def from_config(cls, mapping):
        """The optional `mpc.cem` mapping of a config (keys: the fields' names); absent or empty: None, the planner off."""
        if mapping is None or (hasattr(mapping, "__len__") and len(mapping) == 0):
            return None
        if not hasattr(mapping, "keys"):
            raise ValueError("mpc.cem must be a mapping of %s, got %r" % (", ".join(cls.FIELDS), mapping))
        unknown = sorted(set(mapping.keys()) - set(cls.FIELDS))
        if unknown:
            raise ValueError("mpc.cem has unknown keys %s (known: %s)" % (unknown, ", ".join(cls.FIELDS)))
        return cls(**{k: mapping[k] for k in mapping.keys()})

    def elite_count(self, rollouts):
        r = int(rollouts)
        if r < 2 or r > _capi.MAX_SAMPLES:
            raise ValueError("the cross-entropy planner needs 2..%d rollouts, got %d" % (_capi.MAX_SAMPLES, r))
        e = max(1, r // 4) if self.elites is None else self.elites
        if e > r:
            raise ValueError("cem.elites=%d exceeds the %d rollouts" % (e, r))
        return e

    def warm_count(self, rollouts):
        """W: the rows of population 0 that a carried fit replaces."""
        r = int(rollouts)
        self.elite_count(r)
        w = max(1, r // 4) if self.warm_rows is None else self.warm_rows
        if not 1 <= w <= r - 1:
            raise ValueError("cem.warm_rows=%d outside 1..%d (the rollouts less one)" % (w, r - 1))
        return w

    def carried_floor(self):
        return self.min_std if self.warm_std is None else self.warm_std

    def __repr__(self):
        return "CemSettings(%s)" % ", ".join("%s=%r" % (f, getattr(self, f)) for f in self.FIELDS)


CEM_MAX_HORIZON = 32
WEIGHTINGS = ("elites", "mppi")                 # NDP_PLAN_ELITES, NDP_PLAN_MPPI
OPTIMIZERS = ("sgd", "adam")                    # NDP_PLAN_SGD, NDP_PLAN_ADAM


class GradSettings:
    """The opt-in gradient stage of mpc_plan / plan_step / MpcController (`grad=`; include/ndp.h "planner: gradient
    refinement"): after the sampling rounds (population 0, and the rounds of `cem` when given) the `rows`
    best action sequences of every trajectory are refined by `iterations` steps of gradient descent on the planner's own
    score, through the forward model's exact input gradients, and replace the `rows` worst ones before the last
    selection.  The originals stay in the population, so the chosen error never rises.  Works with any `cem` or none.
      iterations  J >= 0 gradient steps (0: the planner without the stage, bit for bit)
      rows        G, the sequences refined per trajectory, 1 <= G <= R // 2 (so R >= 2); None: max(1, R // 8)
      lr          step size, finite and > 0 (in fp32 too)
      optimizer   "adam" (moments start at 0 in every planning step) or "sgd"
      beta1, beta2, eps   Adam's, 0 <= beta < 1, eps finite and >= 0
      low, high   bounds of the 4 action components the refined rows are clamped to: one number for all, or 4
    The defaults are hyperparameters, not measurements."""

    FIELDS = ("iterations", "rows", "lr", "optimizer", "beta1", "beta2", "eps", "low", "high")

    def __init__(self, iterations=3, rows=None, lr=0.05, optimizer="adam", beta1=0.9, beta2=0.999, eps=1e-8, low=-1.0,
                 high=1.0):
        def integer(v, name):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError("grad.%s must be an integer, got %r" % (name, v))
            return int(v)

        def four(v, name):
            vals = [float(x) for x in v] if hasattr(v, "__len__") else [float(v)] * 4
            if len(vals) != 4 or any(x != x or x in (float("inf"), float("-inf")) for x in vals):
                raise ValueError("grad.%s must be one finite number or 4, got %r" % (name, v))
            return tuple(vals)

        self.iterations = integer(iterations, "iterations")
        if not 0 <= self.iterations <= 65535:
            raise ValueError("grad.iterations must lie in 0..65535, got %d" % self.iterations)
        self.rows = None if rows is None else integer(rows, "rows")
        if self.rows is not None and not 1 <= self.rows <= _capi.MAX_SAMPLES // 2:
            raise ValueError("grad.rows must lie in 1..%d (and not above half the rollouts), got %d"
                             % (_capi.MAX_SAMPLES // 2, self.rows))
        self.lr = float(lr)
        if not 0.0 < _capi.c_float(self.lr).value < float("inf"):      # the kernel reads it as fp32
            raise ValueError("grad.lr must be finite and > 0 (in fp32), got %r" % (lr,))
        if optimizer not in OPTIMIZERS:
            raise ValueError("grad.optimizer must be 'adam' or 'sgd', got %r" % (optimizer,))
        self.optimizer = optimizer
        self.beta1, self.beta2, self.eps = float(beta1), float(beta2), float(eps)
        for name in ("beta1", "beta2"):
            if not 0.0 <= _capi.c_float(getattr(self, name)).value < 1.0:
                raise ValueError("grad.%s must lie in [0, 1) (in fp32), got %r" % (name, getattr(self, name)))
        if not 0.0 <= self.eps < float("inf"):
            raise ValueError("grad.eps must be finite and >= 0, got %r" % (eps,))
        self.low, self.high = four(low, "low"), four(high, "high")
        if any(lo > hi for lo, hi in zip(self.low, self.high)):
            raise ValueError("grad.low must not exceed grad.high, got %r and %r" % (self.low, self.high))

    @classmethod
    def from_config(cls, mapping):
        """The optional `mpc.grad` mapping of a config (keys: the fields' names); absent or empty: None, the stage off."""
        if mapping is None or (hasattr(mapping, "__len__") and len(mapping) == 0):
            return None
        if not hasattr(mapping, "keys"):
            raise ValueError("mpc.grad must be a mapping of %s, got %r" % (", ".join(cls.FIELDS), mapping))
        unknown = sorted(set(mapping.keys()) - set(cls.FIELDS))
        if unknown:
            raise ValueError("mpc.grad has unknown keys %s (known: %s)" % (unknown, ", ".join(cls.FIELDS)))
        return cls(**{k: mapping[k] for k in mapping.keys()})

    def row_count(self, rollouts):
        """G for R = rollouts."""
        r = int(rollouts)
        if r < 2 or r > _capi.MAX_SAMPLES:
            raise ValueError("the gradient stage needs 2..%d rollouts, got %d" % (_capi.MAX_SAMPLES, r))
        g = max(1, r // 8) if self.rows is None else self.rows
        if g > r // 2:
            raise ValueError("grad.rows=%d exceeds half the %d rollouts (%d): the refined rows replace the worst ones and "
                             "must not reach the best" % (g, r, r // 2))
        return g

    def __repr__(self):
        return "GradSettings(%s)" % ", ".join("%s=%r" % (f, getattr(self, f)) for f in self.FIELDS)


def grad_from_config(config, rollouts=None, horizon=None):
    """The GradSettings of a config's optional `mpc.grad` mapping, checked against mpc.rollouts and mpc.time_horizon;
    None when the key is absent."""
    mpc = config.get("mpc") if hasattr(config, "get") else None
    grad = GradSettings.from_config(mpc.get("grad") if mpc is not None and hasattr(mpc, "get") else None)
    if grad is not None:
        _grad_check(grad, int(mpc.rollouts) if rollouts is None else rollouts,
                    int(mpc.time_horizon) if horizon is None else horizon)
    return grad


def _grad_check(grad, rollouts, horizon, models=None):
    if not isinstance(grad, GradSettings):
        raise TypeError("grad must be an evaluation.GradSettings, got %r" % (grad,))
    grad.row_count(rollouts)
    if int(horizon) > CEM_MAX_HORIZON:
        raise ValueError("the gradient stage takes a horizon of at most %d, got %d" % (CEM_MAX_HORIZON, int(horizon)))
    if models is not None and getattr(models, "fm_precision", "fp32") != "fp32":
        # the gradient stage runs in fp32 (forward_keep / input_grads): its rows would be ranked against bf16 ones
        raise ValueError("grad=%r with an EvalModels of fm_precision=%r: the gradient stage is fp32 only and mixed-precision "
                         "ranking is not offered; plan with fm_precision='fp32' or without grad"
                         % (grad, models.fm_precision))


def cem_normal_floats(batch, rollouts, horizon, iterations, seq_length=None):
    """Standard normal floats the planner consumes with `cem`: iterations * steps * B * R * 4 per planning step.
    seq_length None: one plan_step call (steps = Th); otherwise one mpc_plan call on T = seq_length frames, whose
    planning step i has steps = min(Th, T - 1 - i)."""
    per = int(iterations) * int(batch) * int(rollouts) * 4
    if seq_length is None:
        return per * int(horizon)
    t1 = int(seq_length) - 1
    return per * sum(min(int(horizon), t1 - i) for i in range(t1))


def plan_normal_floats(batch, rollouts, horizon, cem, seq_length=None, prior=False):
    """Standard normal floats the planner consumes with the settings `cem`: cem_normal_floats for the iterations, and
    ahead of them steps * B * W * 4 for ndp_plan_warm in every planning step that starts from a prior.  seq_length None: one
    plan_step call, with or without `prior`; otherwise one mpc_plan call on T = seq_length frames, where with
    cem.warm_start every planning step but the first has one (`prior` is not read)."""
    b, r, th = int(batch), int(rollouts), int(horizon)
    n = cem_normal_floats(b, r, th, cem.iterations, seq_length)
    if seq_length is None:
        return n + (th * b * cem.warm_count(r) * 4 if prior else 0)
    if not cem.warm_start:
        return n
    t1 = int(seq_length) - 1
    return n + b * cem.warm_count(r) * 4 * sum(min(th, t1 - i) for i in range(1, t1))


def cem_from_config(config, rollouts=None, horizon=None):
    """The CemSettings of a config's optional `mpc.cem` mapping, checked against mpc.rollouts and mpc.time_horizon;
    None when the key is absent."""
    mpc = config.get("mpc") if hasattr(config, "get") else None
    cem = CemSettings.from_config(mpc.get("cem") if mpc is not None and hasattr(mpc, "get") else None)
    if cem is not None:
        _cem_check(cem, int(mpc.rollouts) if rollouts is None else rollouts,
                   int(mpc.time_horizon) if horizon is None else horizon)
    return cem


def _cem_check(cem, rollouts, horizon):
    if not isinstance(cem, CemSettings):
        raise TypeError("cem must be an evaluation.CemSettings, got %r" % (cem,))
    cem.elite_count(rollouts)
    if cem.warm_start:
        cem.warm_count(rollouts)
    if int(horizon) > CEM_MAX_HORIZON:
        raise ValueError("the cross-entropy planner takes a horizon of at most %d, got %d" % (CEM_MAX_HORIZON, int(horizon)))


def _cem_normal(models, normal, need, seed):
    if normal is None:
        return models.normal(need, seed)
    if normal.numel() != need:
        raise ValueError("normal has %d floats, the planner needs %d" % (normal.numel(), need))
    return normal.reshape(-1).to(models.device, non_blocking=True).float()


# ---------------------------------------------------------------------- one planning step
def _broadcast(state, rep):
    """rep [B*R,3,128,128] <- every image of state [B,3,128,128] R times, rows [B][R].  Returns rep."""
    b = int(state.shape[0])
    r = int(rep.shape[0]) // b
    rep.view(b, r, IMAGE_VALUES).copy_(state.view(b, 1, IMAGE_VALUES).expand(b, r, IMAGE_VALUES))
    return rep


def _rollout_generator(models, state, goal_code, b, r, steps, noise, rep, seq, warm=None):
    """The closed-loop rollouts of one planning step from `state` [B,3,128,128]: per horizon step encode, the
    generator's input with the goal code, R actions per trajectory (written to seq[ts], [B,R,4]) and the forward model
    on the B * R rows.  At ts = 0 the state is encoded once per trajectory and its code broadcast to the R rows.  noise:
    the step's `steps` pieces of B * R * nz floats.  warm: None, or [steps,B,W,4]: at every horizon step warm[ts] replaces the
    last W rows of seq[ts] after the generator has written them and before the forward model reads them, so those rows cost
    no extra forward-model rows (the generator's later actions for them are computed and discarded).  Returns (the last
    predictions, the ts = 0 predictions)."""
    nz, br = models.noise_dim, b * r
    pred = _broadcast(state, rep)
    for ts in range(steps):
        code_in = models.g_input(models.encode(state if ts == 0 else pred), r if ts == 0 else 1, goal_code, r, br)
        act = models.generate(code_in, noise[ts * br * nz:(ts + 1) * br * nz], out=seq[ts])
        if warm is not None:
            seq[ts, :, r - int(warm.shape[2]):].copy_(warm[ts])       # act is seq[ts]
        pred = models.forward(pred, act)
        if ts == 0:
            pred0 = pred
    return pred, pred0


def _rollout_open(models, state, seq, rep):
    """The open-loop replay of the action sequences seq [steps,B,R,4] from `state`: one forward-model pass on the B * R
    rows per horizon step, the slice seq[ts] as the action operand.  Returns (the last, the ts = 0 predictions)."""
    pred = _broadcast(state, rep)
    for ts in range(int(seq.shape[0])):
        pred = models.forward(pred, seq[ts])
        if ts == 0:
            pred0 = pred
    return pred, pred0


def _uniform_actions(cem, noise, seq, nz):
    """seq [steps,B,R,4] <- low + (high - low) * u, where component c of row i at horizon step ts reads float c % nz of
    that row's piece of `noise` (nz >= 4: four independent draws)."""
    low = torch.tensor(cem.low, dtype=torch.float32).to(seq.device, non_blocking=True)
    high = torch.tensor(cem.high, dtype=torch.float32).to(seq.device, non_blocking=True)
    u = noise[:seq.numel() // 4 * nz].view(*seq.shape[:3], nz)
    u = torch.cat([u] * ((3 + nz) // nz), dim=3)[..., :4]       # component c reads float c % nz
    torch.addcmul(low, u, high - low, out=seq)
    torch.minimum(seq, high, out=seq)                           # low + (high - low) * u can round past high


def _grad_stage(models, grad, grad_io, state, goal, b, r, seq, pred, out_err, out_choice, out_act):
    """The gradient stage of one planning step (GradSettings; include/ndp.h): score the population `seq` [steps,B,R,4]
    whose last predictions are `pred`, gather its G best rows, refine them by J x (open-loop rollout that keeps every
    pass's activations, ndp_plan_goal_grad, the backward chain of ndp_fm_input_grads, ndp_plan_grad_step), and let the last
    step write them over the G worst rows of `seq`, in place.  grad_io: a dict whose curve [J,B,G], src and dst [B,G] are
    written, and which receives "rows" [steps,B,G,4], the last iteration's gradient.  Every buffer of the stage is
    allocated here; nothing synchronises with the host."""
    dev, steps, g = models.device, int(seq.shape[0]), grad.row_count(r)
    models.score_select(pred, b, r, goal, seq[0], None, None, out_err, out_choice, out_act, None)
    seq_g = torch.empty(steps, b, g, 4, dtype=torch.float32, device=dev)
    m, v, rows = torch.empty_like(seq_g), torch.empty_like(seq_g), torch.empty_like(seq_g)
    models.grad_gather(out_err, seq, grad_io["src"], grad_io["dst"], seq_g, m, v)
    start = _broadcast(state, torch.empty(b * g, 3, 128, 128, dtype=torch.float32, device=dev))     # once: no pass writes it
    err_g = torch.empty(b, g, dtype=torch.float32, device=dev)
    for j in range(grad.iterations):
        cur = start
        for ts in range(steps):
            cur = models.forward_keep(cur, seq_g[ts], ts)
        models.goal_grad(cur, goal, g, err_g, cur)             # in place: cur is d err / d (the last predictions)
        for ts in range(steps - 1, -1, -1):
            d_state = torch.empty_like(cur) if ts > 0 else None
            models.input_grads(cur, ts, d_state, rows[ts])
            cur = d_state
        last = j == grad.iterations - 1
        models.grad_step(rows, seq_g, m, v, err_g, j + 1, grad, grad_io["curve"][j], grad_io["dst"] if last else None,
                         seq if last else None)
    grad_io["rows"] = rows


def _grad_buffers(grad, lead, b, r, dev):
    """The stage's results, `lead` the leading dimensions (mpc_plan: one set per planning step): curve [.., J,B,G], src
    and dst [.., B,G] (-1 where the stage does not run)."""
    g = grad.row_count(r)
    return {"curve": torch.empty(*lead, grad.iterations, b, g, dtype=torch.float32, device=dev),
            "src": torch.full((*lead, b, g), -1, dtype=torch.int32, device=dev),
            "dst": torch.full((*lead, b, g), -1, dtype=torch.int32, device=dev)}


def _plan_once(models, cem, state, goal, goal_code, b, r, steps, noise, cem_io, rep, forced, out_err, out_choice, out_act,
               pred_out, prior=None, grad=None, grad_io=None):
    """One planning step from `state` [B,3,128,128], for mpc_plan and plan_step alike.  Population 0 is the generator's
    closed-loop rollouts (_rollout_generator), or with cem.proposal "uniform" a uniform draw replayed open loop; then
    `cem.iterations` x (ndp_eval_score_select, ndp_plan_cem_update, _rollout_open) -- none when `cem` is None --; then the
    last selection, the only one `forced` applies to, which fills out_err [B,R], out_choice [B], out_act [B,4] and
    pred_out (the chosen ts = 0 prediction, or None).  cem_io: None, or with `cem` (normal, curve, best): the step's
    normals [iteration][steps,B,R,4]; curve [I+1,B] receives the chosen row's error per population, best [B] the least of
    them.  Returns (the last population [steps,B,R,4], mean, std [B,steps,4]; None, None without `cem`).
    prior: None, or with cem.warm_start the previous planning step's (mean, std) [B,steps_prev,4], steps <= steps_prev:
    one ndp_plan_warm shifts it into this step's mean / std and draws W = cem.warm_count(R) rows per horizon step from it,
    which replace rows R - W .. R - 1 of population 0; the first update then smooths against the shifted fit (smooth = 1,
    first = 1).  The step's normals are then [steps,B,W,4] ahead of the iterations' blocks.  cem.weighting "mppi" or a
    prior send every update through ndp_plan_update; otherwise the step is ndp_plan_cem_update's, bit for bit.
    grad: None, or a GradSettings with grad_io (_grad_buffers): with iterations > 0, _grad_stage runs between the rounds
    and the last selection, which then scores one more open-loop rollout of the population; mean and std are not touched by
    it, and curve keeps its I + 1 entries (the last is the final population's)."""
    dev, br = models.device, b * r
    seq = torch.empty(steps, b, r, 4, dtype=torch.float32, device=dev)
    mean = std = warm = None
    if prior is not None:
        normal, curve, best = cem_io
        n_warm = steps * b * cem.warm_count(r) * 4
        mean = torch.empty(b, steps, 4, dtype=torch.float32, device=dev)
        std = torch.empty(b, steps, 4, dtype=torch.float32, device=dev)
        warm = torch.empty(steps, b, cem.warm_count(r), 4, dtype=torch.float32, device=dev)
        models.plan_warm(prior[0], prior[1], normal[:n_warm], cem, mean, std, warm)
        cem_io = normal[n_warm:], curve, best
    if cem is not None and cem.proposal == "uniform":
        _uniform_actions(cem, noise, seq, models.noise_dim)
        if warm is not None:
            seq[:, :, r - int(warm.shape[2]):].copy_(warm)
        pred, pred0 = _rollout_open(models, state, seq, rep)
    else:
        pred, pred0 = _rollout_generator(models, state, goal_code, b, r, steps, noise, rep, seq, warm)
    its, per = 0 if cem is None else cem.iterations, steps * br * 4
    if cem is not None:
        normal, curve, best = cem_io
        if prior is None:
            mean = torch.zeros(b, steps, 4, dtype=torch.float32, device=dev)
            std = torch.zeros(b, steps, 4, dtype=torch.float32, device=dev)
    general = cem is not None and (cem.weighting != "elites" or prior is not None)
    for it in range(its):
        # the outputs of the last selection serve the earlier ones too: it overwrites all three
        models.score_select(pred, b, r, goal, seq[0], None, None, out_err, out_choice, out_act, None)
        curve[it].copy_(out_err.gather(1, out_choice.long().view(b, 1)).view(b))
        nxt = torch.empty_like(seq)
        if general:
            models.plan_update(out_err, seq, normal[it * per:(it + 1) * per], cem, it > 0 or prior is not None, it == 0, mean,
                               std, nxt, best)
        else:
            models.cem_update(out_err, seq, normal[it * per:(it + 1) * per], cem, it == 0, mean, std, nxt, best)
        seq = nxt
        pred, pred0 = _rollout_open(models, state, seq, rep)
    if grad is not None and grad.iterations > 0:
        _grad_stage(models, grad, grad_io, state, goal, b, r, seq, pred, out_err, out_choice, out_act)
        pred, pred0 = _rollout_open(models, state, seq, rep)
    models.score_select(pred, b, r, goal, seq[0], pred0 if pred_out is not None else None, forced, out_err, out_choice,
                        out_act, pred_out)
    if cem is not None:
        curve[its].copy_(out_err.gather(1, out_choice.long().view(b, 1)).view(b))
        if its:
            torch.fmin(best, curve[its], out=best)
        else:
            best.copy_(curve[0])
    return seq, mean, std


def mpc_noise_floats(batch, seq_length, rollouts, horizon, noise_dim):
    """Floats of noise one mpc_plan call consumes: B * R * nz per horizon step."""
    t1 = int(seq_length) - 1
    return sum(min(int(horizon), t1 - i) for i in range(t1)) * int(batch) * int(rollouts) * int(noise_dim)


def mpc_plan(models, frames, actions, rollouts, horizon, noise=None, choices=None, seed=0, on_step=None, cem=None,
             normal=None, grad=None):
    """mpc_eval.py:112-184 for B trajectories at once, rows [B][R].

    frames [B,T,3,128,128] float or [B,T,128,128,3] bytes, actions [B,T,4].  noise: None (device draws of
    ndp_uniform_noise with `seed`), or the flat stream of every horizon step's [B*R, nz] piece in order
    (mpc_noise_floats(...) floats; at B = 1 the reference's CPU draws, reference_noise_schedule("mpc", ...)).
    choices: None, or [T-1][B] host indices that replace the rollout rule (teacher forcing).
    Per planning step: encode the current state once per trajectory, R generator rows on the broadcast code and the
    goal code (encoded once), R forward-model rows; then min(Th, T-1-image_num) - 1 more horizon steps on the R
    predictions (mpc_eval.py:131); score against the GOAL image (:161), choose (:159-165), and the chosen rollout's
    ts = 0 prediction is the next state (:167-169).  Nothing synchronises with the host.  Returns device tensors:
    choices [T-1,B] int32, rollout_errors [T-1,B,R], actions [B,T-1,4], image_errors [T-1,B], image_error_sum [B],
    action_error [B].

    cem: None, or a CemSettings: every planning step refines its population by `cem.iterations` rounds of the
    cross-entropy method before it chooses (_plan_once; `choices` replace the last selection only); with 0 iterations and
    the "generator" proposal every result above has the bits of the call without `cem`.  normal: None (device draws of
    ndp_normal_noise with `seed`), or the flat stream [planning step][iteration][steps,B,R,4] (plan_normal_floats(B, R,
    Th, cem, seq_length=T) floats; with cem.warm_start every planning step but the first has [steps,B,W,4] ahead of its
    iterations, and starts from the fit of the step before it, _plan_once's `prior`).  Added results: best_curve
    [T-1,I+1,B] the chosen row's error per population, best_err [T-1,B] the least of them, cem_mean / cem_std [B,steps,4]
    the last planning step's fit (zeros with 0 iterations).

    grad: None, or a GradSettings: every planning step refines its G best rows by gradient descent before it chooses
    (_grad_stage), with or without `cem`; with 0 iterations every result above has the bits of the call without `grad`.
    Added results: grad_curve [T-1,J,B,G] the refined rows' errors before each update, grad_src and grad_dst [T-1,B,G] the
    rows they came from and the rows they replaced (-1 with 0 iterations)."""
    r, th = int(rollouts), int(horizon)
    if r < 1 or th < 1:
        raise ValueError("rollouts and horizon must be >= 1, got %d, %d" % (r, th))
    if cem is not None:
        _cem_check(cem, r, th)
    if grad is not None:
        _grad_check(grad, r, th, models)
    imgs, b, t = _frames(models, frames)
    t1, nz, br = t - 1, models.noise_dim, b * r
    if t1 < 1:
        raise ValueError("trajectories need at least 2 frames")
    dev = models.device
    if noise is None:
        noise = models.uniform(mpc_noise_floats(b, t, r, th, nz), seed)
    else:
        if noise.numel() != mpc_noise_floats(b, t, r, th, nz):
            raise ValueError("noise has %d floats, mpc_plan needs %d" % (noise.numel(), mpc_noise_floats(b, t, r, th, nz)))
        noise = noise.reshape(-1).to(dev, non_blocking=True).float()
    forced = None
    if choices is not None:
        host = torch.as_tensor(choices, dtype=torch.int32).reshape(t1, b)
        if host.min().item() < 0 or host.max().item() >= r:
            raise ValueError("choices must lie in 0..%d" % (r - 1))
        forced = host.to(dev, non_blocking=True)
    per = imgs.view(b, t, IMAGE_VALUES)
    goal = per[:, t1].contiguous().view(b, 3, 128, 128)
    goal_code = models.encode(goal)                                       # once per trajectory
    state = per[:, 0].contiguous().view(b, 3, 128, 128)
    rep = torch.empty(br, 3, 128, 128, dtype=torch.float32, device=dev)
    out_choice = torch.empty(t1, b, dtype=torch.int32, device=dev)
    out_err = torch.empty(t1, b, r, dtype=torch.float32, device=dev)
    out_act = torch.empty(t1, b, 4, dtype=torch.float32, device=dev)
    image_errors = torch.empty(t1, b, dtype=torch.float32, device=dev)
    image_error_sum = torch.zeros(b, dtype=torch.float32, device=dev)     # reset per trajectory (mpc_eval.py:119)
    fut_idx = (torch.arange(b, device=dev, dtype=torch.int32) * t).view(1, b) + \
        torch.arange(1, t, device=dev, dtype=torch.int32).view(t1, 1)      # frame image_num + 1 of every trajectory
    if cem is not None:
        normal = _cem_normal(models, normal, plan_normal_floats(b, r, th, cem, seq_length=t), seed)
        curve = torch.empty(t1, cem.iterations + 1, b, dtype=torch.float32, device=dev)
        best = torch.empty(t1, b, dtype=torch.float32, device=dev)
    if grad is not None:
        grad_all = _grad_buffers(grad, (t1,), b, r, dev)
    off = n_off = 0
    prior = grad_io = None
    for image_num in range(t1):
        if on_step is not None:
            on_step(image_num)
        steps = min(th, t1 - image_num)                                    # mpc_eval.py:131
        n_noise, cem_io = steps * br * nz, None
        if cem is not None:
            n_normal = cem.iterations * steps * br * 4
            if prior is not None:
                n_normal += steps * b * cem.warm_count(r) * 4
            cem_io = normal[n_off:n_off + n_normal], curve[image_num], best[image_num]
            n_off += n_normal
        if grad is not None:
            grad_io = {k: x[image_num] for k, x in grad_all.items()}
        nxt = torch.empty(b, 3, 128, 128, dtype=torch.float32, device=dev)
        _, cem_mean, cem_std = _plan_once(models, cem, state, goal, goal_code, b, r, steps, noise[off:off + n_noise], cem_io,
                                          rep, None if forced is None else forced[image_num], out_err[image_num],
                                          out_choice[image_num], out_act[image_num], nxt, prior, grad, grad_io)
        if cem is not None and cem.warm_start:
            prior = cem_mean, cem_std                                      # shifted by one action at the next step
        off += n_noise
        state = nxt
        # image_error = mse(state_cur_mpc, state_fut) (mpc_eval.py:173-176): frame image_num + 1, the goal at the end
        models.mse(state, imgs, b, IMAGE_VALUES, b_idx=fut_idx[image_num], out=image_errors[image_num], acc=image_error_sum)
    chosen = out_act.transpose(0, 1).contiguous()                         # torch.cat(best_action_list), :178
    want = actions.to(dev).float()[:, :t1].contiguous()
    action_error = models.mse(want, chosen, b, t1 * 4)
    res = {"choices": out_choice, "rollout_errors": out_err, "actions": chosen, "image_errors": image_errors,
           "image_error_sum": image_error_sum, "action_error": action_error}
    if cem is not None:
        res.update(best_curve=curve, best_err=best, cem_mean=cem_mean, cem_std=cem_std)
    if grad is not None:
        res.update(grad_curve=grad_all["curve"], grad_src=grad_all["src"], grad_dst=grad_all["dst"])
    return res


# ---------------------------------------------------------------------- one observation in, one action out
def plan_step_noise_floats(batch, rollouts, horizon, noise_dim):
    """Floats of noise one plan_step call consumes: B * R * nz per horizon step."""
    return int(horizon) * int(batch) * int(rollouts) * int(noise_dim)


def plan_step(models, state, goal, goal_code, rollouts, horizon, noise=None, seed=0, choice=None, cem=None, normal=None,
              prior=None, grad=None):
    """One planning step of MPC_gym_eval.py:183-225 for B environments at once, rows [B][R]: from the observed `state`
    [B,3,128,128], R rollouts of Th steps through encoder, generator and forward model, scored against the goal image.

    The semantics are the live script's, which differ from mpc_eval.py's (mpc_plan) and are reproduced on purpose: the
    horizon is the full Th at every planning step (:188, the shrinking bound is commented out); the rollouts' LAST
    predictions are scored against `goal` [B,3,128,128] (:221); min_error = 10000000000, strict `<` in rollout order,
    so the first minimum wins and a NaN is never chosen (:183, :219-224).  Deduplicated as in mpc_plan: the caller
    encodes the goal once (`goal_code` [B,128]); the state is encoded once and its code broadcast to the R rows at
    ts = 0.  noise: None (device draws of ndp_uniform_noise with `seed`), or the Th pieces [B*R, nz] in order
    (plan_step_noise_floats(...) floats; at B = 1 the reference's draws, noise kind "mpc_gym").  choice: None, or [B]
    int32 indices that replace the rule.  No host synchronisation when the inputs are on the device.  Returns device
    tensors (action [B,4], choice [B] int32, rollout_errors [B,R], actions0 [B,R,4]).

    cem: None, or a CemSettings: `cem.iterations` rounds of the cross-entropy method refine the population before the
    choice (_plan_once; `choice` replaces the last selection only).  normal: None (device draws of ndp_normal_noise with
    `seed`), or the flat stream [iteration][Th,B,R,4] (cem_normal_floats(B, R, Th, I) floats).  With `cem` a fifth
    value follows the four, which describe the last population: a dict of best_curve [I+1,B], best_err [B], cem_mean and
    cem_std [B,Th,4]; with 0 iterations and the "generator" proposal the four have the bits of the call without `cem`.

    prior: None, or with cem.warm_start (anything else: ValueError) the pair (cem_mean, cem_std) [B,steps_prev,4],
    steps_prev >= Th, that the previous call returned: the step starts from that fit shifted by one action (_plan_once),
    and `normal` is then [Th,B,W,4] ahead of the iterations (plan_normal_floats(B, R, Th, cem, prior=True) floats).

    grad: None, or a GradSettings: the gradient stage before the choice (_grad_stage), with or without `cem`.  The dict
    that follows the four values (the fifth value also without `cem`) then carries grad_curve [J,B,G], grad_src and
    grad_dst [B,G] and, with J > 0, grad_rows [Th,B,G,4], the last iteration's gradient; with 0 iterations the four have the
    bits of the call without `grad`."""
    r, th = int(rollouts), int(horizon)
    if r < 1 or th < 1:
        raise ValueError("rollouts and horizon must be >= 1, got %d, %d" % (r, th))
    if cem is not None:
        _cem_check(cem, r, th)
    if grad is not None:
        _grad_check(grad, r, th, models)
    if state.dim() != 4 or tuple(state.shape[1:]) != (3, 128, 128) or tuple(goal.shape) != tuple(state.shape):
        raise _capi.NdpError("state and goal must both be [B,3,128,128], got %s and %s"
                             % (tuple(state.shape), tuple(goal.shape)))
    b, nz, dev = int(state.shape[0]), models.noise_dim, models.device
    br = b * r
    if tuple(goal_code.shape) != (b, 128):
        raise _capi.NdpError("goal_code must be [%d,128], got %s" % (b, tuple(goal_code.shape)))
    need = plan_step_noise_floats(b, r, th, nz)
    if noise is None:
        noise = models.uniform(need, seed)
    else:
        if noise.numel() != need:
            raise ValueError("noise has %d floats, plan_step needs %d" % (noise.numel(), need))
        noise = noise.reshape(-1).to(dev, non_blocking=True).float()
    if prior is not None:
        if cem is None or not cem.warm_start:
            raise ValueError("prior is read only with cem.warm_start")
        prior = tuple(p.to(dev, non_blocking=True).float().contiguous() for p in prior)
        if len(prior) != 2 or any(p.dim() != 3 or int(p.shape[0]) != b or int(p.shape[2]) != 4 or
                                  tuple(p.shape) != tuple(prior[0].shape) for p in prior) or \
                not th <= int(prior[0].shape[1]) <= CEM_MAX_HORIZON:
            raise ValueError("prior must be (mean, std), both [%d,steps_prev,4] with %d <= steps_prev <= %d, got %s"
                             % (b, th, CEM_MAX_HORIZON, [tuple(p.shape) for p in prior]))
    forced = None
    if choice is not None:
        forced = torch.as_tensor(choice, dtype=torch.int32).reshape(b).to(dev, non_blocking=True)
    rep = torch.empty(br, 3, 128, 128, dtype=torch.float32, device=dev)
    err = torch.empty(b, r, dtype=torch.float32, device=dev)
    pick = torch.empty(b, dtype=torch.int32, device=dev)
    action = torch.empty(b, 4, dtype=torch.float32, device=dev)
    cem_io = None
    if cem is not None:
        curve = torch.empty(cem.iterations + 1, b, dtype=torch.float32, device=dev)
        best = torch.empty(b, dtype=torch.float32, device=dev)
        cem_io = _cem_normal(models, normal, plan_normal_floats(b, r, th, cem, prior=prior is not None), seed), curve, best
    # the full horizon (MPC_gym_eval.py:188); nobody reads the chosen rollout's prediction (the environment gives the
    # next state): no pred_out
    grad_io = None if grad is None else _grad_buffers(grad, (), b, r, dev)
    seq, mean, std = _plan_once(models, cem, state.contiguous(), goal.contiguous(), goal_code, b, r, th, noise, cem_io, rep,
                                forced, err, pick, action, None, prior, grad, grad_io)
    if cem is None and grad is None:
        return action, pick, err, seq[0]
    info = {} if cem is None else {"best_curve": curve, "best_err": best, "cem_mean": mean, "cem_std": std}
    if grad is not None:
        info.update(grad_curve=grad_io["curve"], grad_src=grad_io["src"], grad_dst=grad_io["dst"])
        if "rows" in grad_io:
            info["grad_rows"] = grad_io["rows"]
    return action, pick, err, seq[0], info


class MpcController:
    """Closed-loop control of B live environments: camera frames in, actions out.

        ctrl = MpcController(models, rollouts, horizon, frame_shape=(500, 500))
        ctrl.reset(goal_frames)                # bytes [B,128,128,3] or floats [B,3,128,128]: the goal is encoded once
        actions, info = ctrl.act(raw_frames)   # bytes [B,H,W,3], host (numpy / tensor) or device

    act: the frames go through a pinned staging buffer (allocated once) and an asynchronous upload, are resized to
    128x128 on the device exactly as PIL's Image.LANCZOS does (ndp_resize_lanczos_u8: bytes and normalised floats in one
    launch; 128x128 frames take its copy path), plan_step picks the actions, and ONE host synchronisation brings them
    back, because the environment needs them.  `info`: state_u8 [B,128,128,3] (what MPC_gym_eval.get_state resizes to),
    state [B,3,128,128], rollout_errors [B,R], choice [B], actions0 [B,R,4], all on the device."""

    def __init__(self, models, rollouts, horizon, frame_shape=None, seed=0, cem=None, normal=None, grad=None):
        from .resize import LanczosResizer
        self.models, self.rollouts, self.horizon = models, int(rollouts), int(horizon)
        if self.rollouts < 1 or self.horizon < 1:
            raise ValueError("rollouts and horizon must be >= 1")
        if cem is not None:
            _cem_check(cem, self.rollouts, self.horizon)
        # cem: a CemSettings turns plan_step's cross-entropy refinement on for every plan(); `info` then also carries
        # best_curve, best_err, cem_mean, cem_std.  normal: None (device draws, seeded as the noise is), or the flat
        # stream of successive plan() calls since reset(), [call][iteration][Th,B,R,4]; plan(normal=) overrides it.
        # With cem.warm_start every plan() after the first since reset() starts from the fit of the one before it
        # (plan_step's `prior`), and its piece of the stream has [Th,B,W,4] ahead of the iterations
        self.cem, self.normal = cem, normal
        # grad: a GradSettings turns plan_step's gradient stage on for every plan(); `info` then also carries grad_curve,
        # grad_src, grad_dst and grad_rows
        if grad is not None:
            _grad_check(grad, self.rollouts, self.horizon, models)
        self.grad = grad
        self._prior, self._normal_off = None, 0
        self.resizer = LanczosResizer(models.device)
        self.frame_shape = None                               # None: the first frame tells
        if frame_shape is not None:
            self.frame_shape = (int(frame_shape[0]), int(frame_shape[1]))
            self.resizer.tables(*self.frame_shape)            # built and uploaded here, not in the control loop
        self.seed, self.steps = int(seed), 0
        self.goal = self.goal_code = None
        self._staging = self._actions = self._uploaded = None
        self._upload_pending = False
        self._event = torch.cuda.Event()

    def reset(self, goal_frames):
        self.goal = self.models.images(torch.as_tensor(goal_frames))
        self.goal_code = self.models.encode(self.goal)
        b = int(self.goal.shape[0])
        if self._actions is None or int(self._actions.shape[0]) != b:
            self._actions = torch.empty(b, 4, dtype=torch.float32, pin_memory=True)
            self._staging = None
        if self._staging is None and self.frame_shape is not None:
            self._staging = torch.empty((b,) + self.frame_shape + (3,), dtype=torch.uint8, pin_memory=True)
        self.steps = 0
        self._prior, self._normal_off = None, 0               # the next plan() is a first one: no fit to carry

    def observe(self, raw_frames):
        """bytes [B,H,W,3], host or device -> (resized bytes [B,128,128,3], normalised floats [B,3,128,128]) on the
        device.  Host frames pass through the one pinned staging buffer: a call first waits for the previous call's upload
        to have left that buffer -- only where no plan() lay between, whose one synchronisation covers the upload --, then
        nothing waits."""
        if self.goal is None:
            raise _capi.NdpError("MpcController.reset(goal_frames) comes before the first frame")
        raw = torch.as_tensor(raw_frames)
        if raw.dtype != torch.uint8 or raw.dim() != 4 or int(raw.shape[3]) != 3:
            raise _capi.NdpError("frames must be uint8 [B,H,W,3], got %s %s" % (raw.dtype, tuple(raw.shape)))
        if self.frame_shape is None:
            self.frame_shape = (int(raw.shape[1]), int(raw.shape[2]))
        want = (int(self.goal.shape[0]),) + self.frame_shape + (3,)
        if tuple(raw.shape) != want:
            raise _capi.NdpError("frames must be uint8 %s, got %s" % (want, tuple(raw.shape)))
        if not raw.is_cuda:
            if self._staging is None:
                self._staging = torch.empty(want, dtype=torch.uint8, pin_memory=True)
            elif self._upload_pending:
                self._uploaded.synchronize()                  # the last upload has read the buffer
            self._staging.copy_(raw)
            with _capi.on_device(self.models.device):
                raw = self._staging.to(self.models.device, non_blocking=True)
                if self._uploaded is None:
                    self._uploaded = torch.cuda.Event()
                self._uploaded.record()
                self._upload_pending = True
        return self.resizer(raw)

    def plan(self, state, noise=None, choice=None, normal=None):
        """plan_step on `state` and the goal of reset(), then the one host synchronisation.  Returns (actions [B,4] on
        the host, info)."""
        if self.cem is not None:
            per = plan_normal_floats(int(state.shape[0]), self.rollouts, self.horizon, self.cem, prior=self._prior is not None)
            if normal is None and self.normal is not None:
                normal = self.normal.reshape(-1)[self._normal_off:self._normal_off + per]
            self._normal_off += per
        action, pick, err, act0, *extra = plan_step(self.models, state, self.goal, self.goal_code, self.rollouts, self.horizon,
                                                    noise=noise, seed=self.seed + self.steps, choice=choice, cem=self.cem,
                                                    normal=normal, prior=self._prior, grad=self.grad)
        extra = extra[0] if extra else {}                     # with `cem`: best_curve, best_err, cem_mean, cem_std
        if self.cem is not None and self.cem.warm_start:
            self._prior = extra["cem_mean"], extra["cem_std"]
        self.steps += 1
        with _capi.on_device(self.models.device):
            self._actions.copy_(action, non_blocking=True)
            self._event.record()
        self._event.synchronize()                             # the environment needs the action
        self._upload_pending = False                          # the frames' upload came before it on the stream
        return self._actions.clone(), dict(extra, state=state, action=action, rollout_errors=err, choice=pick, actions0=act0)

    def act(self, raw_frames, noise=None, choice=None, normal=None):
        state_u8, state = self.observe(raw_frames)
        actions, info = self.plan(state, noise=noise, choice=choice, normal=normal)
        info["state_u8"] = state_u8
        return actions, info


# ---------------------------------------------------------------------- the reference's per-call loop
def module_loop_mpc(encode, generate, forward, frames, actions, rollouts, horizon, noise, noise_dim):
    """mpc_eval.py's planning loop for ONE trajectory, restated on three callables (encode [n,3,128,128] -> [n,128],
    generate [n,256+nz] -> [n,4], forward (images, actions) -> images), with the reference's call pattern: the goal
    encoded at every horizon step, R copies of the state encoded at ts = 0, one host sync per rollout to choose, one
    more forward-model call for the chosen action.  The baseline scripts/bench_mpc.py times (on the drop-in modules and
    on PyTorch operators) and the tests compare mpc_plan with.  Returns (choices, chosen actions [T-1,4], image errors)."""
    t1 = int(frames.shape[1]) - 1
    images = frames[0]
    goal = images[t1:t1 + 1]
    state_mpc = images[0:1]
    mse = torch.nn.MSELoss()
    choices, chosen, errors = [], [], []
    off = 0
    for image_num in range(t1):
        fut = images[image_num + 1:image_num + 2]
        state_fwd = state_mpc.repeat(rollouts, 1, 1, 1)
        taken = None
        for ts in range(min(horizon, t1 - image_num)):
            codes = torch.cat([encode(state_fwd), encode(goal.repeat(rollouts, 1, 1, 1))], dim=1)
            piece = noise[off:off + rollouts * noise_dim].view(rollouts, noise_dim)
            off += rollouts * noise_dim
            act = generate(torch.cat([codes, piece], dim=1))
            if ts == 0:
                taken = act
            state_fwd = forward(state_fwd, act)
        best, min_error = 0, MIN_ERROR
        for ro in range(rollouts):
            err = mse(state_fwd[ro], goal[0])
            if err < min_error:
                min_error, best = err, ro
        state_mpc = forward(state_mpc, taken[best:best + 1])
        choices.append(best)
        chosen.append(taken[best])
        errors.append(mse(state_mpc, fut))
    return choices, torch.stack(chosen), torch.stack(errors)


# ---------------------------------------------------------------------- differentiating the planner's score
def goal_loss_and_grad(fwd_model, state, goal, actions):
    """The score mpc_eval.py:159-165 gives a sampled action sequence -- the MSE between the forward model's Th-step
    eval-mode rollout from `state` and the goal image -- and its gradient with respect to the actions.
    state, goal [B,3,128,128]; actions [B,Th,4].  Returns (loss [B], d sum(loss) / d actions [B,Th,4]).  The rollout is
    Th forwards of `fwd_model` (a ForwardAutoencoder in eval mode) inside input_gradients() and one backward through
    them (ndp_fm_input_grads per step).  Not used by the drop-in scripts, which reproduce the reference's output."""
    from .input_grad import input_gradients
    if fwd_model.training:
        raise _capi.NdpError("goal_loss_and_grad needs the forward model in eval mode (fwd_model.eval())")
    acts = actions.detach().clone().requires_grad_(True)
    with torch.enable_grad(), input_gradients():
        cur = state.detach()
        for t in range(int(acts.shape[1])):
            cur = fwd_model(cur, acts[:, t])
        loss = ((cur - goal.detach()) ** 2).flatten(1).mean(dim=1)
        grad, = torch.autograd.grad(loss.sum(), acts)
    return loss.detach(), grad


def refine_actions(fwd_model, state, goal, actions, steps, optimizer_factory):
    """`steps` optimiser steps on the actions against goal_loss_and_grad's score; optimizer_factory([actions]) -> a
    torch optimiser (e.g. lambda p: torch.optim.SGD(p, lr=0.1)).  Returns (refined actions, loss [B] before each step)."""
    acts = actions.detach().clone().requires_grad_(True)
    opt = optimizer_factory([acts])
    losses = []
    for _ in range(int(steps)):
        loss, grad = goal_loss_and_grad(fwd_model, state, goal, acts)
        opt.zero_grad()
        acts.grad = grad
        opt.step()
        losses.append(loss)
    return acts.detach(), losses


# ---------------------------------------------------------------------- what the three drop-in scripts share
def eval_settings(kind, config, dataset, generator=None):
    """The scripts' hyperparameters, checked where the reference would fail (with a message instead of a shape error
    deep inside a module).  Returns (random_seed, num_sample, noise_dim, batch_size, rollouts, horizon)."""
    ev = config.evaluation
    seed, k, nz, bs = int(config.random_seed), int(ev.num_sample), int(ev.noise_dim), int(ev.batch_size)
    r = th = None
    t = int(dataset.seq_length)
    if k < 1 or bs < 1:
        raise ValueError("evaluation.num_sample and evaluation.batch_size must be >= 1")
    if t < 2:
        raise ValueError("trajectory_length must be >= 2")
    if generator is not None and int(generator.noise_dim) != nz:
        raise ValueError("evaluation.noise_dim=%d but the generator was trained with noise_dim %d"
                         % (nz, int(generator.noise_dim)))
    if len(dataset) % bs != 0:
        # the scripts view the generator's output as [batch_size, -1, 4] (control_evaluation.py:115,
        # complete_eval.py:135): a short last batch does not fit
        raise ValueError("len(dataset)=%d is not a multiple of evaluation.batch_size=%d" % (len(dataset), bs))
    if kind == "open" and bs * (t - 1) == 1:
        raise ValueError("open-loop evaluation needs batch_size * (trajectory_length - 1) >= 2 (control_evaluation.py:"
                         "108 squeezes a single code row)")
    if kind == "closed" and k != 1:
        raise ValueError("closed-loop evaluation needs evaluation.num_sample == 1 (complete_eval.py:138)")
    if kind == "mpc":
        r, th = int(config.mpc.rollouts), int(config.mpc.time_horizon)
        if bs != 1:
            raise ValueError("mpc_eval needs evaluation.batch_size == 1 (mpc_eval.py:161 scores against state_target[0]); "
                             "batched planning is evaluation.mpc_plan")
        if k != 1:
            raise ValueError("mpc_eval needs evaluation.num_sample == 1 (mpc_eval.py:152 feeds [R,K,4] actions to the "
                             "forward model)")
        if r < 2:
            raise ValueError("mpc_eval needs mpc.rollouts >= 2 (mpc_eval.py:141 squeezes a single rollout's codes)")
        if th < 1:
            raise ValueError("mpc.time_horizon must be >= 1")
    return seed, k, nz, bs, r, th


def make_eval_dataset(config):
    """PushDataset(evaluation_data_path, seq_length=trajectory_length, raw_uint8=True), or `synthetic:<N>:images|frames_u8` seeded
    trajectories as for train_data_path."""
    from .utils.trajectory_loader import open_dataset
    # decoded frames stay bytes (normalised by ndp_eval_frames_u8); `raw_uint8: false` gives the reference's floats;
    # `raw_jpeg: true` yields the JPEG streams, decoded on the device
    frames = {"raw_jpeg": True} if bool(config.get("raw_jpeg", False)) else {"raw_uint8": bool(config.get("raw_uint8", True))}
    return open_dataset(config.evaluation_data_path, seq_length=int(config.trajectory_length), seed=int(config.random_seed),
                        default_mode="images", modes=("images", "frames_u8", "jpeg"),
                        mode_error="evaluation needs images: use synthetic:<N>:images, synthetic:<N>:frames_u8 or "
                                   "synthetic:<N>:jpeg",
                        push=dict(seq_length=int(config.trajectory_length), **frames))


def script_main(fetch, argv=None, add_arguments=None, prepare=None):
    """The scripts' __main__ (control_evaluation.py:160-187 and its twins): CLI, config, dataset, the three whole-module
    pickles, then `fetch`.  Prints the returned tuple.  add_arguments(parser): a script's own flags beside the common ones.
    prepare(namespace): called after parsing and before anything is loaded; what it returns (a tuple, e.g. the parsed
    arguments in front and a live environment behind) is wrapped around fetch's arguments as
    fetch(*before, image_encoder, fwd_model_autoencoder, generator, dataset, config, *after)."""
    from argparse import ArgumentParser

    from .utils.cli_arguments.common_arguments import add_common_arguments
    parser = ArgumentParser(description="Interact with your training script")
    parser = add_common_arguments(parser)
    parser.add_argument("--fm-precision", choices=FM_PRECISIONS, default=None,
                        help="operand precision of the forward model's passes (default: evaluation.fm_precision, else fp32)")
    parser.add_argument("--enc-precision", choices=ENC_PRECISIONS, default=None,
                        help="precision of the image encoder's passes (default: evaluation.enc_precision, else fp32)")
    if add_arguments is not None:
        add_arguments(parser)
    _, config, wrapped = config_cli(parser, argv, "evaluation", prepare)
    before, after = wrapped if prepare is not None else ((), ())
    dataset = make_eval_dataset(config)
    image_encoder, generator, fwd_model_autoencoder, _ = load_eval_models(config)
    result = fetch(*before, image_encoder, fwd_model_autoencoder, generator, dataset, config, *after)
    if len(result) == 2:
        print("avg_action_error, avg_image_loss:", result[0], result[1])
    else:
        print("avg_action_error, avg_image_loss, avg_goal_error, success_rate:", *result)
    return result
